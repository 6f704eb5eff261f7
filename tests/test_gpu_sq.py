"""GPU: IndexIVFScalarQuantizer (QT_8bit, kind 4) against the oracle's IVF-Flat search over the stored (decoded) vectors — codes, trained
parameters, both metrics, both residual settings, the score-row and the filtered scan, both group forms of k_sq_list_scan, edge cases,
list import, persistence and the refusals.  Inputs, expected results and the certificate bound: tests/sq_ref.py; their preconditions:
tests/test_sq_host.py."""
import numpy as np
import pytest

import sq_ref

pytestmark = pytest.mark.gpu
F32 = np.float32
_built = {}


def make_index(gpu, d, nlist, metric, by_residual, cen, trained):
    ix = gpu.IndexIVFScalarQuantizer(None, d, nlist, gpu.ScalarQuantizer.QT_8bit, metric, by_residual)
    assert not ix.is_trained
    ix.set_centroids(cen)
    assert not ix.is_trained, "trained once centroids AND scalar-quantiser parameters are present"
    ix.set_sq_trained(trained)
    assert ix.is_trained
    return ix


def built(gpu, name, metric, by_residual):
    """one populated index per (input set, metric, residual setting), shared by the tests"""
    key = (name, metric, by_residual)
    if key not in _built:
        c = sq_ref.inputs(name)
        t, _, _ = sq_ref.quantised(name, by_residual)
        ix = make_index(gpu, c.d, c.nlist, metric, by_residual, c.cen, t)
        ix.add(c.x)
        ix.nprobe = c.nprobe
        _built[key] = ix
    return _built[key]


def check_result(D, I, Dk1, Ik1, k, metric, what):
    """scores within tol = max |Dref| 2^-23 (the bar for fp32 rows: fp64 sum order), ids equal at every position that is not near-tied,
    near-tied positions at most 2 %"""
    Dref, Iref = Dk1[:, :k], Ik1[:, :k]
    tol = np.abs(Dref[np.isfinite(Dref)]).max() * 2.0 ** -23      # from the k results; the k + 1 oracle result serves the near-tie mask only
    assert np.array_equal(np.isfinite(D), np.isfinite(Dref)), what
    pad = -np.inf if metric == 0 else np.inf
    assert (D[~np.isfinite(Dref)] == pad).all() and (I[~np.isfinite(Dref)] == -1).all(), what
    err = np.abs(np.where(np.isfinite(Dref), D.astype(np.float64) - Dref, 0.0))
    print(f"{what}: max score error {err.max():.3e} (tol {tol:.3e})")
    assert err.max() <= tol, what
    tied = sq_ref.near_tied(Dk1, tol)
    assert tied.mean() <= 0.02, what
    bad = (I != Iref) & ~tied
    assert not bad.any(), f"{what}: ids differ at {np.argwhere(bad)[:4].tolist()}"


def search_and_check(ix, q, k, metric, Dk1, Ik1, filt, what):
    ix.set_param("ivf_filter", filt)
    ix.set_param("profile", 0)          # clears the counters
    D, I = ix.search(q, k)
    assert ix.get_timing("ivfsq_scan_launches") > 0, what
    fb = ix.get_timing("fallback_queries")
    print(f"{what}: fallback_queries {fb:.0f} of {len(q)}")
    assert fb <= 0.05 * len(q), what
    check_result(D, I, Dk1, Ik1, k, metric, what)
    return D, I


def _cases():
    out = [("A", 10, None), ("B", 1, None), ("B", 10, None), ("B", 100, None), ("C", 100, None)]
    out += [("D", k, nq) for k in (10, 1000) for nq in (200, 64, 20)]
    return out


@pytest.mark.parametrize("filt", [0, 2])
@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name,k,nq", _cases())
def test_search_vs_oracle(gpu, name, k, nq, metric, by_residual, filt):
    c = sq_ref.inputs(name)
    ix = built(gpu, name, metric, by_residual)
    Dk1, Ik1 = sq_ref.expected(name, metric, by_residual, k + 1, nq)
    q = c.q if nq is None else c.q[:nq]
    search_and_check(ix, q, k, metric, Dk1, Ik1, filt, f"set {name} k {k} nq {len(q)} metric {metric} by_residual {by_residual} ivf_filter {filt}")


@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_codes_ids_and_order_of_every_list(gpu, name, by_residual):
    c = sq_ref.inputs(name)
    _, codes, _ = sq_ref.quantised(name, by_residual)
    ix = built(gpu, name, 0, by_residual)
    assert ix.ntotal == c.n and ix.code_size == c.d and ix.sq.qtype == 0 and ix.by_residual == by_residual
    assert np.array_equal(ix.list_sizes(), c.sizes)
    for l in range(c.nlist):
        want = np.nonzero(c.assign == l)[0]         # insertion order
        got_codes, got_ids = ix.get_list(l)
        assert got_codes.dtype == np.uint8 and got_codes.shape == (len(want), c.d)
        assert np.array_equal(got_ids, want), f"list {l}"
        assert np.array_equal(got_codes, codes[want]), f"list {l}"


@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_train_parameters_bit_for_bit(gpu, orc, name, by_residual):
    c = sq_ref.inputs(name)
    ix = gpu.IndexIVFScalarQuantizer(None, c.d, c.nlist, 0, gpu.METRIC_INNER_PRODUCT, by_residual)
    ix.train(c.x)
    assert ix.is_trained
    cen = ix.get_centroids()
    y = c.x32
    if by_residual:
        a, _ = orc.assign_ip(cen, c.x32)
        y = orc.residuals(cen, c.x32, a)
    assert np.array_equal(ix.sq.trained.view(np.uint32), sq_ref.train(y).view(np.uint32))


# ------------------------------------------------------------------------------------------ edge cases at shape (B)
def _oracle(orc, cen, x32, ids, trained, by_residual, q32, metric, nprobe, k):
    a, _ = orc.assign_ip(cen, x32)
    y = orc.residuals(cen, x32, a) if by_residual else x32
    codes = sq_ref.encode(trained, y)
    xhat = sq_ref.reconstruct(trained, codes, cen if by_residual else None, a)
    lm = orc.ListMajor(a, ids, xhat, len(cen))
    return orc.ivfflat_search(metric, cen, lm, q32, min(nprobe, len(cen)), k), a, codes


def _edge(gpu, orc, x32, q32, cen, trained, metric, by_residual, nprobe, k, what, ids=None, add=None, filts=(0, 2)):
    n, d = x32.shape
    ids = np.arange(n) if ids is None else ids
    (Dk1, Ik1), a, codes = _oracle(orc, cen, x32, ids, trained, by_residual, q32, metric, nprobe, k + 1)
    ix = make_index(gpu, d, len(cen), metric, by_residual, cen, trained)
    (add or (lambda i: i.add(x32)))(ix)
    ix.nprobe = nprobe
    for f in filts:
        search_and_check(ix, q32, k, metric, Dk1, Ik1, f, f"{what} metric {metric} ivf_filter {f}")
    return ix, a, codes


@pytest.mark.parametrize("metric", [0, 1])
def test_constant_dimension(gpu, orc, metric):
    c = sq_ref.inputs("B")
    x = c.x32.copy(); x[:, 5] = F32(0.375)
    t = sq_ref.train(x)
    assert t[c.d + 5] == 0
    ix, a, codes = _edge(gpu, orc, x, c.q32, c.cen, t, metric, False, 4, 10, "constant dimension")
    assert (codes[:, 5] == 0).all() and all((ix.get_list(l)[0][:, 5] == 0).all() for l in range(c.nlist))


@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
def test_values_outside_the_trained_range_clamp(gpu, orc, metric, by_residual):
    c = sq_ref.inputs("B")
    a, _ = orc.assign_ip(c.cen, c.x32)
    y = orc.residuals(c.cen, c.x32, a) if by_residual else c.x32
    t = sq_ref.train(y[:1500] * F32(0.5))              # a range most values fall out of
    ix, a, codes = _edge(gpu, orc, c.x32, c.q32, c.cen, t, metric, by_residual, 4, 10, f"clamping by_residual {by_residual}")
    assert (codes == 0).mean() > 0.05 and (codes == 255).mean() > 0.05
    got = np.concatenate([ix.get_list(l)[0] for l in range(c.nlist)])
    assert np.array_equal(got, codes[np.argsort(a, kind="stable")])


@pytest.mark.parametrize("metric", [0, 1])
def test_empty_list_short_list_nprobe_past_nlist_and_padding(gpu, orc, metric):
    """two equal centroids (the second one's list stays empty), a list of fewer than 16 rows, nprobe > nlist, and k larger than the probed
    rows: the results are padded with -1 / -+inf"""
    c = sq_ref.inputs("B")
    cen = c.cen.copy(); cen[7] = cen[3]
    a, _ = orc.assign_ip(cen, c.x32)
    assert (a == 7).sum() == 0
    keep = np.ones(c.n, bool)
    l5 = np.nonzero(a == 5)[0]
    keep[l5[5:]] = False                                  # list 5 keeps 5 rows
    x = c.x32[keep]
    t = sq_ref.train(orc.residuals(cen, x, a[keep]))
    _edge(gpu, orc, x, c.q32, cen, t, metric, True, 4, 10, "empty + short list")
    _edge(gpu, orc, x, c.q32, cen, t, metric, True, 1000, 10, "nprobe > nlist")
    small = x[:60]
    ix, _, _ = _edge(gpu, orc, small, c.q32[:9], cen, t, metric, True, 3, 100, "k > probed rows")
    D, I = ix.search(c.q32[:9], 100)
    assert (I == -1).any() and (D[I == -1] == (-np.inf if metric == 0 else np.inf)).all()


@pytest.mark.parametrize("metric", [0, 1])
def test_add_in_three_calls_with_ids_and_reserve(gpu, orc, metric):
    c = sq_ref.inputs("B")
    t, _, _ = sq_ref.quantised("B", True)
    ids = (np.arange(c.n) * 7 + 1000003).astype(np.int64)

    def three(ix):
        for lo, hi in ((0, 1000), (1000, 1001), (1001, c.n)):
            ix.add_with_ids(c.x32[lo:hi], ids[lo:hi])
    ix3, _, _ = _edge(gpu, orc, c.x32, c.q32, c.cen, t, metric, True, 4, 10, "three adds with ids", ids=ids, add=three)

    def reserved(ix):
        ix.reserve_lists(c.sizes)
        ix.add_with_ids(c.x32, ids)
    ixr, _, _ = _edge(gpu, orc, c.x32, c.q32, c.cen, t, metric, True, 4, 10, "reserve_lists + add", ids=ids, add=reserved, filts=(2,))
    for l in range(c.nlist):
        (c3, i3), (cr, ir) = ix3.get_list(l), ixr.get_list(l)
        assert np.array_equal(c3, cr) and np.array_equal(i3, ir)


@pytest.mark.parametrize("metric", [0, 1])
def test_forced_group_forms_agree(gpu, metric):
    """the 16-query and the 64-query form of the scan on the same batch (70 queries fill neither): same results"""
    c = sq_ref.inputs("B")
    ix = built(gpu, "B", metric, True)
    Dk1, Ik1 = sq_ref.expected("B", metric, True, 11)
    try:
        for qt in (0, 4):
            ix.set_param("ivf_qtiles", qt)
            search_and_check(ix, c.q, 10, metric, Dk1, Ik1, 2, f"ivf_qtiles {qt} metric {metric}")
    finally:
        ix.set_param("ivf_qtiles", 1)


@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
def test_add_list_import_and_save_load(gpu, tmp_path, metric, by_residual):
    c = sq_ref.inputs("B")
    t, _, _ = sq_ref.quantised("B", by_residual)
    src = built(gpu, "B", metric, by_residual)
    imp = make_index(gpu, c.d, c.nlist, metric, by_residual, c.cen, t)
    for l in range(c.nlist):
        codes, ids = src.get_list(l)
        imp.add_list(l, codes, ids)
    imp.nprobe = c.nprobe
    Dk1, Ik1 = sq_ref.expected("B", metric, by_residual, 11)
    D0, I0 = search_and_check(imp, c.q, 10, metric, Dk1, Ik1, 2, "add_list import")
    path = tmp_path / "sq.rsx"
    gpu.write_index(imp, path)
    back = gpu.read_index(path)
    assert isinstance(back, gpu.IndexIVFScalarQuantizer) and back.by_residual == by_residual and back.ntotal == c.n and back.nprobe == c.nprobe
    assert np.array_equal(back.sq.trained, t) and back.metric_type == metric
    for l in range(c.nlist):
        (ca, ia), (cb, ib) = src.get_list(l), back.get_list(l)
        assert np.array_equal(ca, cb) and np.array_equal(ia, ib)
    D1, I1 = search_and_check(back, c.q, 10, metric, Dk1, Ik1, 2, "after save / load")
    assert np.array_equal(D0, D1) and np.array_equal(I0, I1)


def test_other_kinds_files_are_unchanged_by_the_new_record(gpu, tmp_path):
    """an IVF-Flat file has no scalar-quantiser record: header, centroid block, empty codebook block, lists"""
    c = sq_ref.inputs("B")
    ix = gpu.IndexIVFFlat(None, c.d, c.nlist, gpu.METRIC_INNER_PRODUCT)
    ix.set_centroids(c.cen)
    ix.add(c.x32[:100])
    p = tmp_path / "flat.rsx"
    gpu.write_index(ix, p)
    header, v2 = 4 + 11 * 4 + 8, 8 + 4 + 4              # FileHeader and FileHeaderV2
    want = header + v2 + 8 + c.cen.size * 4 + 8 + c.nlist * 8 + 100 * (c.d * 4 + 8)
    assert p.stat().st_size == want


# ------------------------------------------------------------------------------------------ refused in this build
def test_refusals_leave_the_handle_untouched(gpu, tmp_path, monkeypatch):
    import ctypes
    c = sq_ref.inputs("B")
    ix = built(gpu, "B", 0, True)
    before = [ix.get_list(l) for l in range(c.nlist)]
    sel = gpu.IDSelectorRange(0, 100)
    with pytest.raises(RuntimeError, match="IndexIVFScalarQuantizer.*kind 4"):
        ix.search(c.q, 10, params=gpu.SearchParametersIVF(sel=sel))
    with pytest.raises(RuntimeError, match="IndexIVFScalarQuantizer.*kind 4"):
        ix.remove_ids(sel)
    with pytest.raises(RuntimeError, match="IndexIVFScalarQuantizer.*kind 4"):
        ix.remove_ids(np.arange(10))
    with pytest.raises(RuntimeError, match="IndexIVFScalarQuantizer.*kind 4"):
        ix.search_prepass(c.q, 10)
    import torch
    tau, ntau = ctypes.c_void_p(), ctypes.c_int64(0)
    qd = torch.as_tensor(c.q32).cuda()
    D = torch.empty((c.nq, 10), dtype=torch.float32, device="cuda"); I = torch.empty((c.nq, 10), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st = gpu.lib().rsx_search_prepass(ix._h, ctypes.c_int64(c.nq), ctypes.c_void_p(qd.data_ptr()), 0, 10, ctypes.c_void_p(D.data_ptr()),
                                      ctypes.c_void_p(I.data_ptr()), ctypes.byref(tau), ctypes.byref(ntau))
    assert st != 0 and b"kind 4" in gpu.lib().rsx_last_error()
    with pytest.raises(RuntimeError, match="IndexIVFScalarQuantizer.*kind 4"):
        gpu.IndexRefineFlat(ix)
    with pytest.raises(RuntimeError, match="kind 4.*sharded"):
        gpu.IndexIVFScalarQuantizer(None, c.d, c.nlist, 0, gpu.METRIC_INNER_PRODUCT, True, devices=[0, 0])
    h = ctypes.c_void_p()
    arr = (ctypes.c_int * 2)(0, 0)
    assert gpu.lib().rsx_sharded_create(4, c.d, c.nlist, 0, 8, 0, 2, arr, ctypes.byref(h)) != 0
    assert b"kind 4" in gpu.lib().rsx_last_error()
    path = tmp_path / "sq.rsx"
    gpu.write_index(ix, path)
    with pytest.raises(RuntimeError, match="kind 4.*sharded"):
        gpu.read_index(path, devices=[0, 0])
    monkeypatch.setenv("RSX_INDEX_FORMAT", "faiss")
    with pytest.raises(RuntimeError, match="kind 4.*FAISS"):
        gpu.write_index(ix, tmp_path / "sq.faiss")
    monkeypatch.delenv("RSX_INDEX_FORMAT")
    with pytest.raises(RuntimeError, match="kind 4"):
        ix.set_param("scan_chunk", 256)
    with pytest.raises(RuntimeError, match="populated"):
        ix.set_sq_trained(ix.sq.trained)
    after = [ix.get_list(l) for l in range(c.nlist)]
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before, after))
    Dk1, Ik1 = sq_ref.expected("B", 0, True, 11)
    search_and_check(ix, c.q, 10, 0, Dk1, Ik1, 2, "after the refusals")
