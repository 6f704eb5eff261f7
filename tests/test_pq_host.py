"""Host side of IndexPQ (faiss.IndexPQ, contriever/src/index.py:19): the FAISS `IxPq` container and the C ABI's declaration.

The `IxPq` bytes are assembled BY HAND here — struct.pack calls in the field order of FAISS 1.8.0 faiss/impl/index_write.cpp
(write_index_header, write_ProductQuantizer, WRITEVECTOR(codes), search_type, encode_signs, polysemous_ht) — not through
rsx_faiss_io's writer, so the reader is checked against an independent statement of the layout.  No FAISS-produced file exists
offline: byte compatibility with real FAISS is unverified, as for the other containers."""
import os
import re
import struct

import numpy as np
import pytest

import rsx_faiss_io as fio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 1 << 20


def _ixpq_bytes(d, M, metric, codebooks, codes, is_trained=True):
    n = len(codes)
    b = b"IxPq"
    # write_index_header: int d; idx_t ntotal; idx_t dummy; idx_t dummy; bool is_trained; int metric_type
    b += struct.pack("<i", d) + struct.pack("<q", n) + struct.pack("<q", DUMMY) + struct.pack("<q", DUMMY)
    b += struct.pack("<?", is_trained) + struct.pack("<i", metric)
    # write_ProductQuantizer: size_t d, M, nbits; WRITEVECTOR(centroids)
    b += struct.pack("<Q", d) + struct.pack("<Q", M) + struct.pack("<Q", 8)
    cb = np.ascontiguousarray(codebooks, dtype="<f4")
    b += struct.pack("<Q", cb.size) + cb.tobytes()
    # WRITEVECTOR(codes): std::vector<uint8_t> of ntotal * code_size bytes
    c = np.ascontiguousarray(codes, dtype=np.uint8)
    b += struct.pack("<Q", c.size) + c.tobytes()
    # Search_type_t search_type (int, ST_PQ = 0); bool encode_signs; int polysemous_ht
    b += struct.pack("<i", 0) + struct.pack("<?", False) + struct.pack("<i", 0)
    return b


@pytest.mark.parametrize("metric", [0, 1])
def test_ixpq_bytes_parse_and_round_trip(metric):
    rng = np.random.default_rng(5)
    d, M, n = 24, 6, 37
    cb = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    b = _ixpq_bytes(d, M, metric, cb, codes)
    p = fio.parse_faiss(b)
    assert p["kind"] == "PQ" and p["fourcc"] == "IxPq"
    assert (p["d"], p["M"], p["nbits"], p["metric"], p["ntotal"], p["is_trained"]) == (d, M, 8, metric, n, True)
    assert p["codebooks"].shape == (M, 256, d // M) and np.array_equal(p["codebooks"], cb)
    assert p["codes"].shape == (n, M) and np.array_equal(p["codes"], codes)
    assert (p["search_type"], p["encode_signs"], p["polysemous_ht"]) == (0, False, 0)
    assert fio.serialize_faiss(p) == b
    for cut in (3, 20, 60, len(b) // 2, len(b) - 1):
        with pytest.raises(RuntimeError, match="truncated"):
            fio.parse_faiss(b[:cut])


def test_ixpq_empty_index_round_trips():
    cb = np.zeros((4, 256, 2), np.float32)
    b = _ixpq_bytes(8, 4, 0, cb, np.zeros((0, 4), np.uint8))
    p = fio.parse_faiss(b)
    assert p["ntotal"] == 0 and p["codes"].shape == (0, 4)
    assert fio.serialize_faiss(p) == b


def test_legacy_pq_magics_stay_unsupported():
    for cc in (b"IxPQ", b"IxPo"):
        with pytest.raises(RuntimeError, match="unsupported FAISS index type"):
            fio.parse_faiss(cc + b"\0" * 64)


def test_pq_create_is_declared_and_listed():
    import rsx
    header = open(os.path.join(REPO, "include", "rsx.h")).read()
    assert re.search(r"\bint\s+rsx_pq_create\s*\(\s*int d, int M, int nbits, int metric, int device, rsx_index_t\*\* out\)", header)
    assert re.search(r"RSX_KIND_PQ\s*=\s*3", header)
    assert "rsx_pq_create" in rsx.ABI_SYMBOLS
    assert rsx.IndexPQ.__mro__[1] is rsx.Index


def test_index_pq_without_a_gpu_raises(rsxlib):
    if rsxlib.get_num_gpus() > 0:
        ix = rsxlib.IndexPQ(16, 4, 8)
        assert ix._get("kind") == 3 and not ix.is_trained and ix.metric_type == rsxlib.METRIC_L2
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        rsxlib.IndexPQ(16, 4, 8)
