"""CPU: the host side of the vector transforms — the reference of tests/vt_ref.py against fp64, the random rotation, the
factory's parsing, the RSXT transform records on bytes, the ABI, and the refusal to construct anything without a GPU."""
import os
import re

import numpy as np
import pytest

import vt_ref
from conftest import REPO

F32 = np.float32


@pytest.mark.parametrize("n,d_in,d_out", [(50, 40, 24), (7, 100, 100), (3, 64, 160), (1, 8, 8)])
@pytest.mark.parametrize("bias", [False, True])
def test_reference_apply_against_fp64(orc, n, d_in, d_out, bias):
    """A chain of d_in fmaf steps from +0 errs by at most d_in 2^-24 Σ|a||x| (one rounding of a partial sum bounded by Σ|a||x| per step, to
    first order); the bias adds one more rounding of a value bounded by Σ|a||x| + |b|: (d_in + 1) 2^-24 (Σ|a||x| + |b|) in all."""
    rng = np.random.RandomState(d_in + d_out)
    A = rng.randn(d_out, d_in).astype(F32)
    b = rng.randn(d_out).astype(F32) if bias else None
    x = rng.randn(n, d_in).astype(F32)
    y = vt_ref.apply(A, b, x)
    assert y.dtype == F32 and y.shape == (n, d_out)
    want = x.astype(np.float64) @ A.astype(np.float64).T + (b.astype(np.float64) if bias else 0.0)
    bound = (d_in + 1) * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(A).astype(np.float64).T + (np.abs(b) if bias else 0.0))
    err = np.abs(y - want)
    print(f"max error {err.max():.3e}, smallest slack {(bound - err).min():.3e}")
    assert (err <= bound).all()
    # the chain itself, restated in fp64: the product of two fp32 values is exact there (48 bits); the sum is rounded to 53 bits before the fp32
    # rounding, which differs from fmaf's single rounding only where it lands exactly on an fp32 tie — these seeded inputs hit none
    s = np.zeros((n, d_out), dtype=F32)
    for t in range(d_in):
        s = (s.astype(np.float64) + x[:, t:t + 1].astype(np.float64) * A[None, :, t].astype(np.float64)).astype(F32)
    if bias:
        s = (s + b[None, :]).astype(F32)
    assert np.array_equal(s.view(np.uint32), y.view(np.uint32))


def test_reference_reverse_inverts_a_rotation(orc):
    A = vt_ref.random_rotation(40, 40, 3)
    rng = np.random.RandomState(0)
    b = rng.randn(40).astype(F32)
    x = rng.randn(20, 40).astype(F32)
    back = vt_ref.reverse(A, b, vt_ref.apply(A, b, x))
    assert np.abs(back - x).max() <= 42 * 2.0 ** -23 * np.abs(x).max() * np.sqrt(40)
    assert vt_ref.apply(A, None, np.zeros((0, 40), F32)).shape == (0, 40)


@pytest.mark.parametrize("d_in,d_out", [(8, 8), (64, 64), (100, 24), (64, 160), (768, 256)])
def test_random_rotation_is_orthonormal(rsxlib, d_in, d_out):
    """Rounding an orthonormal matrix once moves an entry of A·Aᵀ by at most 2 · 2^-24 (Cauchy-Schwarz over unit rows): 2^-23; fp64 QR
    adds ~1e-15.  The bound asked is 2^-22."""
    A = vt_ref.random_rotation(d_in, d_out, 12345)
    assert A.dtype == F32 and A.shape == (d_out, d_in)
    A64 = A.astype(np.float64)
    G = A64 @ A64.T if d_out <= d_in else A64.T @ A64
    assert np.abs(G - np.eye(min(d_in, d_out))).max() <= 2.0 ** -22
    import rsx_vt
    assert np.array_equal(rsx_vt._orthonormal_rows(d_in, d_out, 12345).astype(F32), A), "the library's generator and the reference's differ"
    assert not np.array_equal(A, vt_ref.random_rotation(d_in, d_out, 12346))


ACCEPTED = {
    "Flat": ([], 768, ("Flat",), False),
    "IVF4096,Flat": ([], 768, ("IVFFlat", 4096), False),
    "IVF4096,PQ96": ([], 768, ("IVFPQ", 4096, 96), False),
    "IVF4096,PQ96x8": ([], 768, ("IVFPQ", 4096, 96), False),
    "IVF16,SQ8": ([], 768, ("IVFSQ", 16), False),
    "PQ96": ([], 768, ("PQ", 96), False),
    "PQ96x8": ([], 768, ("PQ", 96), False),
    "IVF4096,PQ96,RFlat": ([], 768, ("IVFPQ", 4096, 96), True),
    "PQ64,RFlat": ([], 768, ("PQ", 64), True),
    "Flat,RFlat": ([], 768, ("Flat",), True),
    "IVF8,Flat,RFlat": ([], 768, ("IVFFlat", 8), True),
    "OPQ96,IVF4096,PQ96": ([("OPQ", 96, 768)], 768, ("IVFPQ", 4096, 96), False),
    "OPQ64_256,IVF4096,PQ64": ([("OPQ", 64, 256)], 256, ("IVFPQ", 4096, 64), False),
    "OPQ16,PQ16": ([("OPQ", 16, 768)], 768, ("PQ", 16), False),
    "PCA256,Flat": ([("PCA", 256)], 256, ("Flat",), False),
    "PCAR64,IVF16,SQ8": ([("PCAR", 64)], 64, ("IVFSQ", 16), False),
    "RR768,IVF16,Flat": ([("RR", 768)], 768, ("IVFFlat", 16), False),
    "RR1024,Flat": ([("RR", 1024)], 1024, ("Flat",), False),
    "PCA256,OPQ32,IVF64,PQ32": ([("PCA", 256), ("OPQ", 32, 256)], 256, ("IVFPQ", 64, 32), False),
    " PCA128 , PQ16x8 ": ([("PCA", 128)], 128, ("PQ", 16), False),
}


@pytest.mark.parametrize("desc", sorted(ACCEPTED))
def test_factory_parsing_accepts(rsxlib, desc):
    tr, di, base, refine = ACCEPTED[desc]
    assert rsxlib.parse_index_factory(768, desc) == {"transforms": tr, "d_index": di, "base": base, "refine": refine}


@pytest.mark.parametrize("desc,token", [
    ("HNSW32", "HNSW32"), ("IVF16", "IVF16"), ("IVF16,HNSW", "HNSW"), ("IVF16,PQ7", "PQ7"), ("PQ16x4", "PQ16x4"), ("IVF16,PQ16x12", "PQ16x12"),
    ("Flat,Foo", "Foo"), ("IVF16,Flat,Foo", "Foo"), ("OPQ7,Flat", "OPQ7"), ("OPQ16_1000,Flat", "OPQ16_1000"), ("PCA1000,Flat", "PCA1000"),
    ("PCA0,Flat", "PCA0"), ("ITQ64,Flat", "ITQ64"), ("L2norm,Flat", "L2norm"), ("IVF16,SQ4", "SQ4"), ("IVF0,Flat", "IVF0"),
    ("OPQ16,IVF16,PQ16,RFlat", "RFlat"), ("IVF16,SQ8,RFlat", "RFlat"), ("RFlat", "RFlat"), ("Flat,PCA64", "PCA64"), ("PCA64", "PCA64"), ("Flat,,", ""),
])
def test_factory_parsing_refuses(rsxlib, desc, token):
    with pytest.raises(ValueError) as e:
        rsxlib.parse_index_factory(768, desc)
    assert "index_factory" in str(e.value) and (repr(token) in str(e.value) or (token == "" and "empty token" in str(e.value))), str(e.value)


def _records():
    rng = np.random.RandomState(2)
    A = rng.randn(3, 5).astype(F32)
    yield {"tag": "LTra", "d_in": 5, "d_out": 3, "have_bias": True, "is_orthonormal": False, "is_trained": True, "A": A,
           "b": rng.randn(3).astype(F32), "extra": {}}
    yield {"tag": "RRot", "d_in": 5, "d_out": 3, "have_bias": False, "is_orthonormal": True, "is_trained": True, "A": A,
           "b": np.zeros((0,), F32), "extra": {}}
    yield {"tag": "LTra", "d_in": 5, "d_out": 3, "have_bias": False, "is_orthonormal": False, "is_trained": False, "A": np.zeros((0, 0), F32),
           "b": np.zeros((0,), F32), "extra": {}}
    yield {"tag": "PCAm", "d_in": 5, "d_out": 3, "have_bias": True, "is_orthonormal": False, "is_trained": True, "A": A, "b": rng.randn(3).astype(F32),
           "extra": {"eigen_power": -0.5, "random_rotation": True, "mean": rng.randn(5).astype(F32), "eigenvalues": rng.rand(5),
                     "PCAMat": rng.randn(5, 5).astype(F32)}}
    yield {"tag": "OPQm", "d_in": 6, "d_out": 4, "have_bias": False, "is_orthonormal": True, "is_trained": True, "A": rng.randn(4, 6).astype(F32),
           "b": np.zeros((0,), F32), "extra": {"M": 2, "niter": 8, "max_train_points": 65536}}


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


def test_rsxt_records_round_trip_on_bytes(rsxlib):
    recs = list(_records())
    blob = b"".join(rsxlib.pack_vt_record(r) for r in recs)
    off = 0
    for r in recs:
        got, off = rsxlib.unpack_vt_record(blob, off)
        assert _same(got, r), r["tag"]
        assert rsxlib.pack_vt_record(got) == rsxlib.pack_vt_record(r)
    assert off == len(blob)
    with pytest.raises(RuntimeError, match="truncated"):
        rsxlib.unpack_vt_record(blob[:40], 0)
    with pytest.raises(RuntimeError, match="unknown transform kind"):
        rsxlib.unpack_vt_record(b"XXXX" + blob[4:], 0)
    with pytest.raises(RuntimeError, match="unknown transform kind"):
        rsxlib.pack_vt_record(dict(recs[0], tag="ITQm"))


def test_abi_1008_and_the_transform_symbols(rsxlib):
    L = rsxlib.lib()
    assert L.rsx_version() >= 1008
    header = open(os.path.join(REPO, "include", "rsx.h")).read()
    for sym in ("rsx_vt_create", "rsx_vt_set", "rsx_vt_apply", "rsx_vt_destroy"):
        assert sym in rsxlib.ABI_SYMBOLS and getattr(L, sym) is not None
        assert re.search(r"\b" + sym + r"\s*\(", header)
    for name in ("VectorTransform", "LinearTransform", "RandomRotationMatrix", "PCAMatrix", "OPQMatrix", "IndexPreTransform",
                 "SearchParametersPreTransform", "index_factory", "extract_index_ivf", "downcast_index"):
        assert hasattr(rsxlib, name), name
    assert issubclass(rsxlib.SearchParametersPreTransform, rsxlib.SearchParameters)
    assert issubclass(rsxlib.OPQMatrix, rsxlib.LinearTransform) and issubclass(rsxlib.LinearTransform, rsxlib.VectorTransform)


def test_no_cpu_fallback_for_transforms(rsxlib):
    """Without a GPU every constructor fails loudly; with one this test is vacuous."""
    if rsxlib.get_num_gpus() > 0:
        return
    for make in (lambda: rsxlib.LinearTransform(8, 8), lambda: rsxlib.RandomRotationMatrix(8, 4), lambda: rsxlib.PCAMatrix(8, 4),
                 lambda: rsxlib.OPQMatrix(8, 2), lambda: rsxlib.index_factory(64, "OPQ16,IVF16,PQ16"), lambda: rsxlib.index_factory(64, "PCA32,Flat")):
        with pytest.raises(RuntimeError, match="no HIP device"):
            make()
