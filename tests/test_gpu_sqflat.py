"""GPU: IndexScalarQuantizer (QT_8bit, kind 5) against the oracle's Flat search over the decoded vectors: the int8 GEMM route
(batches of more than 32 queries) and the small-batch route, the staged driver, tile edges, the exact re-run, overflowing stage rows, more
than 2 GiB of codes, training, persistence, transforms and the refusals.  Restatements and expected results: tests/sqflat_ref.py; their
preconditions: tests/test_sqflat_host.py."""
import ctypes
import struct

import numpy as np
import pytest

import sq_ref
import sqflat_ref
from test_sqflat_host import overflow_order, overflow_passing

pytestmark = pytest.mark.gpu
F32 = np.float32
_built = {}


def make_index(gpu, d, metric, trained):
    ix = gpu.IndexScalarQuantizer(d, gpu.ScalarQuantizer.QT_8bit, metric)
    assert not ix.is_trained and ix._get("kind") == 5 and ix.storage_dtype == "sq8"
    ix.set_sq_trained(trained)
    assert ix.is_trained
    return ix


def built(gpu, name, metric):
    """one populated index per (input set, metric), shared by the tests"""
    if (name, metric) not in _built:
        c = sq_ref.inputs(name)
        ix = make_index(gpu, c.d, metric, sqflat_ref.quantised(name)[0])
        ix.add(c.x)
        _built[(name, metric)] = ix
    return _built[(name, metric)]


def search(ix, q, k):
    """-> (D, I, launches of the int8 scan, re-run queries)"""
    ix.set_param("profile", 0)          # clears the counters
    D, I = ix.search(q, k)
    return D, I, ix.get_timing("sqflat_gemm_launches"), ix.get_timing("fallback_queries")


def oracle(orc, xhat, q32, k, metric):
    return orc.flat_search(np.ascontiguousarray(q32, F32), np.ascontiguousarray(xhat, F32), k + 1, metric)


# ------------------------------------------------------------------------------------------ 1. search against the oracle
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", sqflat_ref.SETS)
def test_search_vs_oracle(gpu, name, metric):
    c = sq_ref.inputs(name)
    ix = built(gpu, name, metric)
    for k in c.ks:
        Dk1, Ik1 = sqflat_ref.expected(name, metric, k + 1)
        D, I, launches, fb = search(ix, c.q, k)
        # G and H hold four queries at a row stored 41 times: no certificate clears them at K' <= 32 (test_sqflat_host.py); they are
        # dropped from the capped set
        hopeless = sqflat_ref.uncertifiable(name, metric, k)
        print(f"set {name} metric {metric} k {k}: {launches:.0f} launches, fallback_queries {fb:.0f} of {c.nq} ({hopeless.sum()} beyond any certificate)")
        assert (launches > 0) == (c.nq > 32), "batches of more than 32 queries take the int8 scan (set C has 7)"
        assert fb <= hopeless.sum() + 0.05 * (c.nq - hopeless.sum())
        sq_ref.check_result(D, I, Dk1, Ik1, k, metric, f"set {name} metric {metric} k {k}", capped=~hopeless)


# ------------------------------------------------------------------------------------------ 2. the staged driver at small size
@pytest.mark.parametrize("metric", [0, 1])
def test_staged_driver_small_units(gpu, metric):
    c = sq_ref.inputs("D")
    ix = built(gpu, "D", metric)
    k = 10
    Dk1, Ik1 = sqflat_ref.expected("D", metric, k + 1)
    D0, I0, l0, _ = search(ix, c.q, k)
    try:
        ix.set_param("flat_pre_unit", 1024); ix.set_param("flat_pre_mult", 1); ix.set_param("flat_stages", 3)
        D1, I1, l1, fb = search(ix, c.q, k)
        stages = ix.get_timing("sqflat_stages")
    finally:
        ix.set_param("flat_pre_unit", 0); ix.set_param("flat_pre_mult", 16); ix.set_param("flat_stages", 0)
    # K' = 64 rows fit one 1024-row unit: one launch of the threshold phase, then one launch per stage
    print(f"default: {l0:.0f} launches; small units: {l1:.0f} launches, {stages:.0f} stages, fallback_queries {fb:.0f}")
    assert stages == 3 and l1 == 1 + 3
    assert l0 == 2                     # 16384 rows through the score buffer, the other 3616 in one filtered launch
    assert np.array_equal(D0, D1) and np.array_equal(I0, I1)
    sq_ref.check_result(D0, I0, Dk1, Ik1, k, metric, f"staged driver metric {metric}")


# ------------------------------------------------------------------------------------------ 3. tile edges
@pytest.mark.parametrize("metric", [0, 1])
def test_tile_edges(gpu, orc, metric):
    c = sq_ref.inputs("B")
    t, codes, xhat = sqflat_ref.quantised("B")
    rng = np.random.RandomState(9)
    q300 = np.concatenate([c.q32] * 5)[:300].copy()
    q300[70:] = (q300[70:] * (1 + 1e-2 * rng.randn(230, c.d))).astype(F32)
    for n, ks in ((100, (10, 128)), (257, (10,)), (6000, (10,))):
        ix = make_index(gpu, c.d, metric, t)
        ix.add(c.x32[:n])
        for nq in (33, 300):
            for k in ks:
                Dk1, Ik1 = oracle(orc, xhat[:n], q300[:nq], k, metric)
                D, I, launches, fb = search(ix, q300[:nq], k)
                assert launches > 0, (n, nq, k)
                sq_ref.check_result(D, I, Dk1, Ik1, k, metric, f"n {n} nq {nq} k {k} metric {metric}")
                if k > n:
                    assert (I[:, n:] == -1).all() and (D[:, n:] == (-np.inf if metric == 0 else np.inf)).all()
        if n == 6000:                    # the filtered launches over ragged tiles: a 1024-row threshold phase, then three stages
            for nq in (33, 300):
                D0, I0, _, _ = search(ix, q300[:nq], 10)
                try:
                    ix.set_param("flat_pre_unit", 1024); ix.set_param("flat_pre_mult", 1); ix.set_param("flat_stages", 3)
                    D1, I1, launches, _ = search(ix, q300[:nq], 10)
                finally:
                    ix.set_param("flat_pre_unit", 0); ix.set_param("flat_pre_mult", 16); ix.set_param("flat_stages", 0)
                assert launches == 4 and np.array_equal(D0, D1) and np.array_equal(I0, I1)
        for nq in (8, 32):               # the small-batch route: the one-list scan of the IVF-SQ kind
            Dk1, Ik1 = oracle(orc, xhat[:n], q300[:nq], 10, metric)
            D, I, launches, fb = search(ix, q300[:nq], 10)
            assert launches == 0, (n, nq)
            sq_ref.check_result(D, I, Dk1, Ik1, 10, metric, f"small route n {n} nq {nq} metric {metric}")
    empty = make_index(gpu, c.d, metric, t)
    for nq in (8, 70):
        D, I = empty.search(c.q32[:nq], 5)
        assert (I == -1).all() and (D == (-np.inf if metric == 0 else np.inf)).all()


def test_cuda_tensors_in_and_out_and_batch_splits(gpu):
    import torch
    c = sq_ref.inputs("B")
    ix = built(gpu, "B", 0)
    D0, I0, _, _ = search(ix, c.q, 10)
    Dt, It = ix.search(torch.as_tensor(c.q32).cuda(), 10)
    assert Dt.is_cuda and It.is_cuda and np.array_equal(Dt.cpu().numpy(), D0) and np.array_equal(It.cpu().numpy(), I0)
    try:
        ix.set_param("query_batch", 40)          # 40 through the GEMM, then 30 through the small-batch route
        D1, I1, launches, _ = search(ix, c.q, 10)
    finally:
        ix.set_param("query_batch", 1024)
    assert launches > 0 and np.array_equal(D1, D0) and np.array_equal(I1, I0)


# ------------------------------------------------------------------------------------------ 4. the exact re-run
@pytest.mark.parametrize("metric", [0, 1])
def test_crowd_queries_are_rerun_exactly(gpu, metric):
    c = sq_ref.inputs("E")
    ix = built(gpu, "E", metric)
    ncrowd, others = int(c.is_crowd_q.sum()), int((~c.is_crowd_q).sum())
    crowd_rows = np.concatenate([[c.r0], np.arange(c.n - c.copies, c.n)])
    for k in c.ks:
        Dk1, Ik1 = sqflat_ref.expected("E", metric, k + 1)
        D, I, launches, fb = search(ix, c.q, k)
        print(f"set E metric {metric} k {k}: fallback_queries {fb:.0f}")
        assert launches > 0 and ncrowd == 6 and 6 <= fb <= 6 + 0.05 * others
        assert ix.get_timing("sqflat_exact_queries") >= 6, "the second search's certificate cannot clear them either: exact scores"
        sq_ref.check_result(D, I, Dk1, Ik1, k, metric, f"set E metric {metric} k {k}", capped=~c.is_crowd_q)
        got = I[c.is_crowd_q]
        assert np.isin(got, crowd_rows).all() and (np.diff(got, axis=1) > 0).all(), "equal scores by ascending id"
        assert np.array_equal(got, Ik1[c.is_crowd_q][:, :k])


# ------------------------------------------------------------------------------------------ 5. overflowing stage rows
def test_overflowing_stage_rows_rerun_their_queries_only(gpu, orc):
    c = sq_ref.inputs("D")
    t, codes, xhat = sqflat_ref.quantised("D")
    order = overflow_order()
    passing = overflow_passing()
    ix = make_index(gpu, c.d, 0, t)
    ix.add(c.x32[order])
    k = 10
    Dk1, Ik1 = oracle(orc, xhat[order], c.q32, k, 0)
    ix.set_param("sqflat_cand_cap", 256)
    D, I, launches, fb = search(ix, c.q, k)
    print(f"fallback_queries {fb:.0f}; queries with more than 320 / 200 keys behind the threshold phase: {(passing > 320).sum()} / {(passing > 200).sum()}")
    assert launches == 2, "the batch is not scanned again"
    assert (passing > 320).sum() <= fb <= (passing > 200).sum() + 0.05 * c.nq and fb >= 1
    sq_ref.check_result(D, I, Dk1, Ik1, k, 0, "overflowing stage rows")
    ix.set_param("sqflat_cand_cap", 0)
    D2, I2, _, fb2 = search(ix, c.q, k)
    assert fb2 <= 0.05 * c.nq and np.array_equal(D, D2) and np.array_equal(I, I2)
    other = gpu.IndexIVFScalarQuantizer(None, 16, 2, 0, 0, False)
    with pytest.raises(RuntimeError, match="sqflat_cand_cap.*kind 5"):
        other.set_param("sqflat_cand_cap", 256)


# ------------------------------------------------------------------------------------------ 6. more than 2 GiB of codes
@pytest.mark.parametrize("metric", [0, 1])
def test_past_two_gib_of_codes(gpu, metric):
    import torch
    d, n, chunk = 2048, 1100000, 100000
    mark = (1 << 31) // d                              # the first row whose byte offset needs more than 31 bits
    rng = np.random.RandomState(3)
    planted = np.sort(np.concatenate([rng.choice(mark, 20, replace=False), mark + rng.choice(n - mark, 18, replace=False), [mark, n - 1]]))
    ix = gpu.IndexScalarQuantizer(d, gpu.ScalarQuantizer.QT_8bit, metric)
    gen = torch.Generator(device="cuda")
    rows = {}
    for i0 in range(0, n, chunk):
        gen.manual_seed(1000 + i0)
        x = torch.randn((chunk, d), generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        if i0 == 0:
            ix.train(x[:20000])
        ix.add(x)
        for r in planted[(planted >= i0) & (planted < i0 + chunk)]:
            rows[int(r)] = x[r - i0].float().cpu().numpy()
        del x
    assert ix.ntotal == n and n * d > (1 << 31) and (planted >= mark).sum() == 20
    q = np.stack([rows[int(r)] for r in planted]).astype(F32)
    xhat = ix.reconstruct_batch(planted).astype(np.float64)
    want = (q.astype(np.float64) * xhat).sum(1) if metric == 0 else ((q.astype(np.float64) - xhat) ** 2).sum(1)
    D, I, launches, fb = search(ix, q, 1)
    print(f"metric {metric}: batch of 40: {launches:.0f} launches, fallback_queries {fb:.0f}")
    assert launches > 0 and fb <= 2
    assert np.array_equal(I[:, 0], planted) and np.array_equal(D[:, 0], want.astype(F32))
    for lo in range(0, 40, 8):
        D8, I8, launches, _ = search(ix, q[lo:lo + 8], 1)
        assert launches == 0
        assert np.array_equal(I8[:, 0], planted[lo:lo + 8]) and np.array_equal(D8[:, 0], want.astype(F32)[lo:lo + 8])


# ------------------------------------------------------------------------------------------ 7. training, codes, reconstruction
@pytest.mark.parametrize("name", ["B", "C", "H"])
def test_training_codes_and_reconstruction_bit_for_bit(gpu, name):
    c = sq_ref.inputs(name)
    t, codes, xhat = sqflat_ref.quantised(name)
    ix = gpu.IndexScalarQuantizer(c.d)
    assert ix.metric_type == gpu.METRIC_L2 and ix.sq.qtype == 0 and ix.code_size == c.d
    ix.train(c.x)
    assert ix.is_trained and np.array_equal(ix.sq.trained.view(np.uint32), t.view(np.uint32))
    ix.add(c.x)
    got, ids = ix.get_list(0)
    assert got.dtype == np.uint8 and np.array_equal(got, codes) and np.array_equal(ids, np.arange(c.n))
    assert np.array_equal(ix.list_sizes(), [c.n])
    assert np.array_equal(ix.reconstruct_n(0, c.n).view(np.uint32), sq_ref.decode(t, codes).view(np.uint32))
    assert np.array_equal(ix.reconstruct(c.n - 1).view(np.uint32), xhat[c.n - 1].view(np.uint32)) and ix.direct_map_type == 0
    D0, I0, _, _ = search(ix, c.q, 10)
    three = gpu.IndexScalarQuantizer(c.d)
    three.set_sq_trained(t)
    for lo, hi in ((0, 1000), (1000, 1001), (1001, c.n)):
        three.add(c.x32[lo:hi])
    assert np.array_equal(three.get_list(0)[0], codes)
    D3, I3, _, _ = search(three, c.q, 10)
    assert np.array_equal(D0, D3) and np.array_equal(I0, I3)
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained
    ix.add(c.x)
    D1, I1, _, _ = search(ix, c.q, 10)
    assert np.array_equal(D0, D1) and np.array_equal(I0, I1)
    imp = gpu.IndexScalarQuantizer(c.d)
    imp.set_sq_trained(t)
    imp.add_codes(codes[:700]); imp.add_codes(codes[700:])
    D2, I2, _, _ = search(imp, c.q, 10)
    assert np.array_equal(D0, D2) and np.array_equal(I0, I2)


# ------------------------------------------------------------------------------------------ 8. save / load
HEADER = "<4s11iq"                      # FileHeader: magic, version, kind, d, metric, nlist, M, nbits, trained, storage_f16, custom_ids, nprobe, ntotal
HEADER_V2 = "<qii"                      # ndropped, add_list_mod, add_list_rem


@pytest.mark.parametrize("metric", [0, 1])
def test_save_load_round_trip(gpu, tmp_path, metric):
    c = sq_ref.inputs("B")
    t, codes, _ = sqflat_ref.quantised("B")
    ix = built(gpu, "B", metric)
    D0, I0, _, _ = search(ix, c.q, 10)
    path = tmp_path / "sq.rsx"
    gpu.write_index(ix, path)
    raw = path.read_bytes()
    zero = np.zeros(c.d, F32).tobytes()
    want = (struct.pack(HEADER, b"RSX1", 2, 5, c.d, metric, 1, 0, 8, 1, 1, 0, 1, c.n) + struct.pack(HEADER_V2, 0, 1, 0)
            + struct.pack("<q", c.d) + zero + struct.pack("<q", 0) + struct.pack("<iiq", 0, 0, 2 * c.d) + t.tobytes()
            + struct.pack("<q", c.n) + codes.tobytes() + np.arange(c.n, dtype=np.int64).tobytes())
    assert raw == want
    back = gpu.read_index(path)
    assert isinstance(back, gpu.IndexScalarQuantizer) and back._get("kind") == 5 and back.ntotal == c.n and back.metric_type == metric
    assert np.array_equal(back.sq.trained, t) and np.array_equal(back.get_list(0)[0], codes)
    D1, I1, launches, _ = search(back, c.q, 10)
    assert launches > 0 and np.array_equal(D0, D1) and np.array_equal(I0, I1)
    with pytest.raises(RuntimeError, match="kind 5.*sharded"):
        gpu.read_index(path, devices=[0, 0])


def test_files_of_the_other_kinds_are_byte_for_byte_what_they_were(gpu, tmp_path):
    """a Flat file and an IVF-SQ file against their records written out by hand: nothing of the new kind reaches them"""
    c = sq_ref.inputs("B")
    x = c.x32[:100].astype(np.float16)                       # fp16-representable rows: fp16 storage
    flat = gpu.IndexFlat(c.d, gpu.METRIC_INNER_PRODUCT)
    flat.add(x)
    p = tmp_path / "flat.rsx"
    gpu.write_index(flat, p)
    want = (struct.pack(HEADER, b"RSX1", 2, 0, c.d, 0, 1, 0, 8, 1, 1, 0, 1, 100) + struct.pack(HEADER_V2, 0, 1, 0) + struct.pack("<q", 0) + struct.pack("<q", 0)
            + struct.pack("<q", 100) + x.astype(F32).tobytes() + np.arange(100, dtype=np.int64).tobytes())
    assert p.read_bytes() == want
    t, _, _ = sq_ref.quantised("B", False)
    ivf = gpu.IndexIVFScalarQuantizer(None, c.d, c.nlist, 0, gpu.METRIC_L2, False)
    ivf.set_centroids(c.cen); ivf.set_sq_trained(t)
    ivf.add(c.x32[:100])
    ivf.nprobe = 3
    p = tmp_path / "ivfsq.rsx"
    gpu.write_index(ivf, p)
    codes = sq_ref.encode(t, c.x32[:100])
    want = (struct.pack(HEADER, b"RSX1", 2, 4, c.d, 1, c.nlist, 0, 8, 1, 1, 0, 3, 100) + struct.pack(HEADER_V2, 0, 1, 0)
            + struct.pack("<q", c.cen.size) + c.cen.tobytes() + struct.pack("<q", 0) + struct.pack("<iiq", 0, 0, 2 * c.d) + t.tobytes())
    for l in range(c.nlist):
        rows = np.nonzero(c.assign[:100] == l)[0]
        want += struct.pack("<q", len(rows))
        if len(rows):
            want += codes[rows].tobytes() + rows.astype(np.int64).tobytes()
    assert p.read_bytes() == want
    assert gpu.read_index(p)._get("kind") == 4


# ------------------------------------------------------------------------------------------ 9. transforms
@pytest.mark.parametrize("metric", [0, 1])
def test_factory_and_pretransform(gpu, metric):
    c = sq_ref.inputs("B")
    ix = gpu.index_factory(c.d, "SQ8", metric)
    assert isinstance(ix, gpu.IndexScalarQuantizer) and ix.metric_type == metric and ix.d == c.d
    pt = gpu.index_factory(c.d, "PCAR32,SQ8", metric)
    assert isinstance(pt.index, gpu.IndexScalarQuantizer) and pt.index.d == 32 and pt.d == c.d
    pt.train(c.x32)
    pt.add(c.x32)
    tx = pt.apply_chain(pt._dev(c.x32, "test"))
    tq = pt.apply_chain(pt._dev(c.q32, "test"))
    plain = gpu.IndexScalarQuantizer(32, gpu.ScalarQuantizer.QT_8bit, metric)
    plain.train(tx)
    plain.add(tx)
    assert np.array_equal(plain.sq.trained, pt.index.sq.trained)
    for k in (1, 10):
        D, I = pt.search(c.q32, k)
        Dp, Ip = plain.search(tq, k)
        assert np.array_equal(D, Dp.cpu().numpy()) and np.array_equal(I, Ip.cpu().numpy())
    assert pt.index.get_timing("sqflat_gemm_launches") > 0


# ------------------------------------------------------------------------------------------ 10. refused in this build
def test_refusals_leave_the_handle_untouched(gpu, tmp_path, monkeypatch):
    import torch
    c = sq_ref.inputs("B")
    ix = built(gpu, "B", 0)
    L = gpu.lib()
    D0, I0, _, _ = search(ix, c.q, 10)
    before = ix.get_list(0)
    sel = gpu.IDSelectorRange(0, 100)
    named = "IndexScalarQuantizer.*kind 5"
    with pytest.raises(RuntimeError, match=named):
        ix.add_with_ids(c.x32[:4], np.arange(4))
    ids = np.arange(4, dtype=np.int64)
    x4 = np.ascontiguousarray(c.x32[:4])
    assert L.rsx_add(ix._h, ctypes.c_int64(4), x4.ctypes.data_as(ctypes.c_void_p), 0, ids.ctypes.data_as(ctypes.c_void_p)) != 0
    assert b"kind 5" in L.rsx_last_error()
    with pytest.raises(RuntimeError, match=named):
        ix.search(c.q, 10, params=gpu.SearchParameters(sel=sel))
    with pytest.raises(RuntimeError, match=named):
        ix.remove_ids(sel)
    with pytest.raises(RuntimeError, match=named):
        ix.remove_ids(np.arange(10))
    with pytest.raises(RuntimeError, match=named):
        ix.range_search(c.q, 1.0)
    r = ctypes.c_void_p()
    q = np.ascontiguousarray(c.q32)
    assert L.rsx_range_search(ix._h, ctypes.c_int64(c.nq), q.ctypes.data_as(ctypes.c_void_p), 0, ctypes.c_float(1.0), 0, ctypes.byref(r)) != 0
    assert b"IndexScalarQuantizer" in L.rsx_last_error() and b"kind 5" in L.rsx_last_error()
    with pytest.raises(RuntimeError, match=named):
        ix.search_prepass(c.q, 10)
    tau, ntau = ctypes.c_void_p(), ctypes.c_int64(0)
    qd = torch.as_tensor(c.q32).cuda()
    D = torch.empty((c.nq, 10), dtype=torch.float32, device="cuda"); I = torch.empty((c.nq, 10), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st = L.rsx_search_prepass(ix._h, ctypes.c_int64(c.nq), ctypes.c_void_p(qd.data_ptr()), 0, 10, ctypes.c_void_p(D.data_ptr()),
                              ctypes.c_void_p(I.data_ptr()), ctypes.byref(tau), ctypes.byref(ntau))
    assert st != 0 and b"kind 5" in L.rsx_last_error()
    with pytest.raises(RuntimeError, match=named):
        gpu.IndexScalarQuantizer(c.d, 0, 0, devices=[0, 0])
    h = ctypes.c_void_p()
    arr = (ctypes.c_int * 2)(0, 0)
    assert L.rsx_sharded_create(5, c.d, 1, 0, 8, 0, 2, arr, ctypes.byref(h)) != 0
    assert b"IndexScalarQuantizer" in L.rsx_last_error() and b"kind 5" in L.rsx_last_error()
    path = tmp_path / "sq.rsx"
    gpu.write_index(ix, path)
    with pytest.raises(RuntimeError, match="IndexScalarQuantizer.*kind 5.*sharded"):
        gpu.read_index(path, devices=[0, 0])
    with pytest.raises(RuntimeError, match=named):
        gpu.IndexRefineFlat(ix)
    with pytest.raises(ValueError, match="RFlat"):
        gpu.index_factory(c.d, "SQ8,RFlat")
    monkeypatch.setenv("RSX_INDEX_FORMAT", "faiss")
    with pytest.raises(RuntimeError, match="kind 5.*FAISS"):
        gpu.write_index(ix, tmp_path / "sq.faiss")
    monkeypatch.delenv("RSX_INDEX_FORMAT")
    for qtype in (1, 4):
        with pytest.raises(RuntimeError, match="kind 5.*QT_8bit"):
            gpu.IndexScalarQuantizer(c.d, qtype)
    # no coarse quantiser: nprobe, assign, centroids, list reservation, list shards
    assert L.rsx_set_nprobe(ix._h, 4) != 0 and b"kind 5" in L.rsx_last_error()
    lab = np.zeros(4, np.int64)
    assert L.rsx_assign(ix._h, ctypes.c_int64(4), x4.ctypes.data_as(ctypes.c_void_p), 0, lab.ctypes.data_as(ctypes.c_void_p)) != 0 and b"kind 5" in L.rsx_last_error()
    cen = np.zeros(c.d, F32)
    assert L.rsx_set_centroids(ix._h, cen.ctypes.data_as(ctypes.c_void_p)) != 0 and b"kind 5" in L.rsx_last_error()
    assert L.rsx_get_centroids(ix._h, cen.ctypes.data_as(ctypes.c_void_p)) != 0 and b"kind 5" in L.rsx_last_error()
    cnt = np.array([10 * c.n], np.int64)
    assert L.rsx_reserve_lists(ix._h, cnt.ctypes.data_as(ctypes.c_void_p)) != 0 and b"kind 5" in L.rsx_last_error()
    fresh = make_index(gpu, c.d, 0, sqflat_ref.quantised("B")[0])
    with pytest.raises(RuntimeError, match=named):
        fresh.set_param("add_list_mod", 2)
    with pytest.raises(RuntimeError, match="populated"):
        ix.set_sq_trained(ix.sq.trained)
    after = ix.get_list(0)
    assert ix.ntotal == c.n and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    D1, I1, _, _ = search(ix, c.q, 10)
    assert np.array_equal(D0, D1) and np.array_equal(I0, I1)
