"""CPU: the reconstruct family's host side — the ABI version and symbols, the reference vectors of tests/reconstruct_ref.py
against the oracle's ADC score on a golden input, the mirror's get_embs(indices) / get_knn_scores over a stub index, and the direct
map's hash functions run on the host under the address and undefined-behaviour sanitizers (a stand-alone program)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import reconstruct_ref as ref
import util
from conftest import REPO

F32 = np.float32


def test_version_and_symbols(rsxlib):
    assert rsxlib.lib().rsx_version() >= 1007
    header = open(os.path.join(REPO, "include", "rsx.h")).read()
    for sym in ("rsx_make_direct_map", "rsx_reconstruct_batch"):
        assert sym in rsxlib.ABI_SYMBOLS and re.search(rf"\bint {sym}\(", header), sym
        assert getattr(rsxlib.lib(), sym) is not None
    assert (rsxlib.DirectMap.NoMap, rsxlib.DirectMap.Array, rsxlib.DirectMap.Hashtable) == (0, 1, 2)
    for cls in (rsxlib.Index, rsxlib.IndexPQ, rsxlib.IndexRefineFlat):
        for verb in ("reconstruct", "reconstruct_batch", "reconstruct_n", "search_and_reconstruct", "make_direct_map"):
            assert callable(getattr(cls, verb)), (cls.__name__, verb)


def test_decoded_vector_reproduces_the_adc_score(orc):
    """golden IVF-PQ case (d 64, M 16): <q, xhat> of the decoded vectors = the oracle's ADC score of the golden result, to fp32 rounding.
    Bound: the ADC score is an fp32 dot of d terms (<q, c>) plus M fp32 dots of dsub terms summed in fp32; xhat adds one rounding per
    component: first order (d + M + 2) u S with u = 2^-24, S = sum_j |q_j| (|c_j| + |r^_j|); (d + M + 4) u S leaves the second order."""
    g = util.load_golden("ivfpq_d64_m16")
    x, q = util.regen(orc, g)
    cen, cb = g["centroids"].astype(F32), g["codebooks"].astype(F32)
    x32, q32 = x.astype(F32), q.astype(F32)
    a, _ = orc.assign_ip(cen, x32)
    codes = orc.pq_encode(cb, orc.residuals(cen, x32, a))
    assert util.sha(codes) == g["codes_sha"]
    dec = ref.pq_decode(cb, codes)
    xhat = (cen[a] + dec).astype(F32)
    I, D = g["I"], g["D"]
    assert (I >= 0).all()
    rows = xhat[I].astype(np.float64)                                   # [nq, k, d]
    dots = np.einsum("qd,qkd->qk", q32.astype(np.float64), rows)
    S = np.einsum("qd,qkd->qk", np.abs(q32).astype(np.float64), np.abs(cen[a][I]).astype(np.float64) + np.abs(dec[I]).astype(np.float64))
    tol = (g["d"] + g["M"] + 4) * 2.0 ** -24 * S
    err = np.abs(dots - D.astype(np.float64))
    print(f"max |<q, xhat> - ADC| = {err.max():.3e}, smallest bound {tol.min():.3e}")
    assert (err <= tol).all()
    # the flat decode adds nothing: a -0 entry stays -0
    c = ref.pq_case(64, 16, flat=True)
    assert (ref.bits(c.xhat) == 0x80000000).any() and np.array_equal(ref.bits(c.xhat), ref.bits(ref.pq_decode(c.cb, c.codes)))


def test_mirror_get_embs_and_knn_scores():
    from src.indicies.index_utils import BackendBase
    rng = np.random.RandomState(2)
    table = rng.randn(50, 12).astype(F32)
    calls = []

    class StubIndex:
        d = 12

        def reconstruct_batch(self, keys):
            assert keys.ndim == 1 and keys.dtype == np.int64
            calls.append(len(keys))
            return table[keys]

    b = BackendBase()
    b.index = StubIndex()
    indices = rng.randint(0, 50, (4, 7))
    embs = b.get_embs(indices)
    assert embs.shape == (4, 7, 12) and np.array_equal(embs, table[indices]) and calls == [28]
    assert b.get_embs(indices=np.array([3, 3, 1])).shape == (3, 12)
    q = rng.randn(4, 12).astype(F32)
    scores = b.get_knn_scores(q, indices)
    want = -np.sqrt(np.sum((np.expand_dims(q, 1) - table[indices]) ** 2, -1))      # the reference's formula (ivf_pq.py:119-123)
    assert scores.shape == (4, 7) and np.array_equal(scores, want)
    with pytest.raises(ValueError):
        b.get_embs()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_direct_map_hash_on_the_host(tmp_path):
    exe = str(tmp_path / "directmap_check")
    src = os.path.join(REPO, "tests", "host", "directmap_check.hip")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined",
                           "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "direct map ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
