"""CPU: the host side of IndexRefineFlat — the FAISS "IxRF" record (rsx_faiss_io), the ABI declaration of rsx_refine and the
k_base = int(k * k_factor) rule of FAISS 1.8.0's IndexRefine::search.  No GPU."""
import os
import re
import struct

import numpy as np
import pytest

from conftest import PKG, REPO


def _flat(d, n, metric=0, seed=0):
    rng = np.random.RandomState(seed)
    return {"kind": "Flat", "d": d, "metric": metric, "ntotal": n, "is_trained": True, "vectors": rng.randn(n, d).astype(np.float32)}


def _ivf(kind, d, n, nlist, M=0, metric=0, seed=1):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, nlist, n)
    ids = [np.nonzero(a == l)[0].astype(np.int64) for l in range(nlist)]
    if kind == "IVFPQ":
        codes = [rng.randint(0, 256, (len(i), M)).astype(np.uint8) for i in ids]
    else:
        codes = [rng.randn(len(i), d).astype(np.float32) for i in ids]
    p = {"kind": kind, "d": d, "metric": metric, "ntotal": n, "is_trained": True, "nlist": nlist, "nprobe": 3,
         "quantizer": {"kind": "Flat", "d": d, "metric": 0, "vectors": rng.randn(nlist, d).astype(np.float32)},
         "invlists": {"nlist": nlist, "codes": codes, "ids": ids}}
    if kind == "IVFPQ":
        p.update(M=M, nbits=8, by_residual=True, codebooks=rng.randn(M, 256, d // M).astype(np.float32))
    return p


def _pq(d, n, M, metric=0, seed=2):
    rng = np.random.RandomState(seed)
    return {"kind": "PQ", "d": d, "metric": metric, "ntotal": n, "is_trained": True, "M": M, "nbits": 8,
            "codebooks": rng.randn(M, 256, d // M).astype(np.float32), "codes": rng.randint(0, 256, (n, M)).astype(np.uint8),
            "search_type": 0, "encode_signs": False, "polysemous_ht": 0}


BASES = {"IVFPQ": lambda m: _ivf("IVFPQ", 32, 300, 5, M=8, metric=m), "PQ": lambda m: _pq(32, 300, 4, metric=m),
         "IVFFlat": lambda m: _ivf("IVFFlat", 32, 300, 5, metric=m), "Flat": lambda m: _flat(32, 300, metric=m, seed=9)}


def _same(a, b, path=""):
    if isinstance(a, dict):
        for key in a:
            if key in ("fourcc",):
                continue
            assert key in b, f"{path}.{key} is missing"
            _same(a[key], b[key], f"{path}.{key}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), path      # (IVF-Flat payloads come back as bytes)
    else:
        assert a == b, f"{path}: {a!r} != {b!r}"


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("base", sorted(BASES))
def test_refine_record_round_trip(base, metric):
    import rsx_faiss_io as fio
    b = BASES[base](metric)
    f = _flat(32, 300, metric=metric, seed=5)
    p = {"kind": "Refine", "d": 32, "metric": metric, "ntotal": 300, "is_trained": True, "base_index": b, "refine_index": f, "k_factor": 4.5}
    data = fio.serialize_faiss(p)
    nested_b, nested_f = fio.serialize_faiss(b), fio.serialize_faiss(f)      # the records as they are written standalone today
    header = struct.pack("<iqqqBi", 32, 300, 1 << 20, 1 << 20, 1, metric)
    assert data[:4] == b"IxRF"
    assert data == b"IxRF" + header + nested_b + nested_f + struct.pack("<f", 4.5)
    assert data[-4:] == struct.pack("<f", 4.5)
    assert nested_f[:4] == (b"IxFI" if metric == 0 else b"IxF2")
    back = fio.parse_faiss(data)
    assert back["kind"] == "Refine" and back["fourcc"] == "IxRF" and back["k_factor"] == 4.5
    assert (back["d"], back["ntotal"], back["is_trained"], back["metric"]) == (32, 300, True, metric)
    assert back["base_index"]["kind"] == base and back["refine_index"]["kind"] == "Flat"
    _same(b, back["base_index"], "base")
    _same(f, back["refine_index"], "refine")
    # parsed records serialise again to the same bytes wherever the nested record does on its own (a parsed IVF-Flat record holds its
    # payload as bytes, which serialize_faiss does not take back)
    assert (fio.serialize_faiss(back) == data) == (fio.serialize_faiss(fio.parse_faiss(nested_b)) == nested_b)
    if base != "IVFFlat":
        assert fio.serialize_faiss(back) == data


def test_refine_record_refuses_what_it_cannot_hold():
    import rsx_faiss_io as fio
    f = _flat(8, 4)
    p = {"kind": "Refine", "d": 8, "metric": 0, "ntotal": 4, "is_trained": True, "base_index": f, "refine_index": _pq(8, 4, 2), "k_factor": 1.0}
    with pytest.raises(RuntimeError, match="IndexRefineFlat"):
        fio.parse_faiss(fio.serialize_faiss(p))                              # a refine store that is not Flat
    ok = dict(p, refine_index=f)
    with pytest.raises(RuntimeError, match="truncated"):
        fio.parse_faiss(fio.serialize_faiss(ok)[:-2])


def test_abi_declares_rsx_refine(rsxlib):
    header = open(os.path.join(REPO, "include", "rsx.h")).read()
    m = re.search(r"int rsx_refine\(([^;]*)\);", header)
    assert m, "include/rsx.h does not declare rsx_refine"
    args = " ".join(m.group(1).split())
    assert args == ("rsx_index_t* flat, int64_t nq, const void* q, int dtype, int kc, const int64_t* labels, int k, float* D, int64_t* I")
    assert "rsx_refine" in rsxlib.ABI_SYMBOLS
    L = rsxlib.lib()
    assert L.rsx_version() >= 1004
    assert hasattr(L, "rsx_refine")


@pytest.mark.parametrize("k,k_factor,k_base", [(1, 1, 1), (10, 10, 100), (100, 1.5, 150), (10, 409.6, 4096), (1000, 4.096, 4096), (10, 1.0, 10),
                                               (10, 4, 40), (7, 1.49, 10), (3, 1.7, 5)])
def test_k_base_rule(rsxlib, k, k_factor, k_base):
    assert rsxlib.refine_k_base(k, k_factor) == k_base == int(k * k_factor)


@pytest.mark.parametrize("k_factor", [0.99, 0, -1.0, float("nan")])
def test_k_factor_below_one_is_rejected(rsxlib, k_factor):
    with pytest.raises(AssertionError, match="k_factor"):
        rsxlib.refine_k_base(10, k_factor)


def test_search_parameters_object(rsxlib):
    p = rsxlib.IndexRefineSearchParameters()
    assert p.k_factor == 1 and p.base_index_params is None and isinstance(p, rsxlib.SearchParameters)
    inner = rsxlib.SearchParametersIVF(nprobe=7)
    p = rsxlib.IndexRefineSearchParameters(k_factor=3.5, base_index_params=inner)
    assert p.k_factor == 3.5 and p.base_index_params is inner
