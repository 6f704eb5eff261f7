"""GPU: range_search (rsx_range_search) against the oracle's complete result cut at the radius (tests/range_ref.py):
lims, ids and score bits, through the numpy path and the CUDA-tensor path."""
import numpy as np
import pytest

import range_ref as rr
import sq_ref

pytestmark = pytest.mark.gpu
F32 = np.float32


def same(got, want, what):
    lims, D, I = (np.asarray(a) for a in got)
    wl, wD, wI = want
    assert lims.dtype == np.int64 and D.dtype == F32 and I.dtype == np.int64, what
    assert lims.shape == wl.shape and lims[0] == 0, what
    bad = np.nonzero(np.diff(lims) != np.diff(wl))[0]
    assert len(bad) == 0, f"{what}: result sizes differ for {len(bad)} queries, first {bad[:3]}: got {np.diff(lims)[bad[:3]]} want {np.diff(wl)[bad[:3]]}"
    assert np.array_equal(I, wI), f"{what}: ids differ at {np.nonzero(I != wI)[0][:5]}"
    assert np.array_equal(D.view(np.int32), wD.view(np.int32)), f"{what}: score bits differ at {np.nonzero(D.view(np.int32) != wD.view(np.int32))[0][:5]}"


def both_paths(ix, q, radius, want, what, **kw):
    """numpy in -> numpy out and CUDA tensor in -> CUDA tensors out, each against the reference"""
    import torch
    got = ix.range_search(q, radius, **kw)
    assert all(isinstance(a, np.ndarray) for a in got), what
    same(got, want, what + " (numpy)")
    tq = torch.as_tensor(np.ascontiguousarray(q)).cuda()
    tg = ix.range_search(tq, radius, **kw)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in tg), what
    same([a.cpu().numpy() for a in tg], want, what + " (CUDA tensors)")
    return got


@pytest.fixture(scope="module")
def flat_ix(gpu):
    x, _ = rr.flat_inputs()
    out = {}
    for metric in (0, 1):
        ix = gpu.IndexFlat(rr.FLAT["d"], metric, device=0)
        ix.add(x)
        assert ix.storage_dtype == "float16"
        out[metric] = ix
    return out


@pytest.fixture(scope="module")
def ivf_ix(gpu):
    c = rr.ivf_inputs()
    ids = 7 * np.arange(c.n, dtype=np.int64) + 1000003
    out = {}
    for metric in (0, 1):
        ix = gpu.IndexIVFFlat(None, c.d, c.nlist, metric, device=0)
        ix.set_centroids(c.cen)
        ix.add_with_ids(c.x, ids)
        out[metric] = ix
    return out


# ------------------------------------------------------------------------------------------ Flat
@pytest.mark.parametrize("nq", [300, 5])
@pytest.mark.parametrize("ridx", [0, 1, 2])
@pytest.mark.parametrize("metric", [0, 1])
def test_flat_vs_oracle(flat_ix, metric, ridx, nq):
    _, q = rr.flat_inputs()
    radius = rr.FLAT_RADII[metric][ridx]
    both_paths(flat_ix[metric], q[:nq], radius, rr.flat_expected(metric, radius, nq), f"Flat metric {metric} radius {radius} nq {nq}")


@pytest.mark.parametrize("metric", [0, 1])
def test_flat_capacity_second_pass(flat_ix, metric):
    """first-pass rows of 1024 keys on the large radius: every query overflows and is scanned again, in several groups under a small temp
    budget; the result is the default-capacity run's"""
    _, q = rr.flat_inputs()
    ix, radius = flat_ix[metric], rr.FLAT_RADII[metric][2]
    want = rr.flat_expected(metric, radius)
    base = ix.range_search(q, radius)
    ov0 = ix.get_timing("range_overflow_queries")
    ix.set_param("range_cand_cap", 1024)
    ix.set_param("temp_budget_mb", 64)
    try:
        got = both_paths(ix, q, radius, want, f"Flat metric {metric}, range_cand_cap 1024")
    finally:
        ix.set_param("range_cand_cap", 0)
        ix.set_param("temp_budget_mb", 16384)
    assert ix.get_timing("range_overflow_queries") > ov0
    for a, b in zip(got, base):
        assert np.array_equal(a.view(np.int32) if a.dtype == F32 else a, b.view(np.int32) if b.dtype == F32 else b)


def test_flat_query_batch_split(flat_ix):
    _, q = rr.flat_inputs()
    ix, radius = flat_ix[0], rr.FLAT_RADII[0][1]
    ix.set_param("query_batch", 128)
    try:
        both_paths(ix, q, radius, rr.flat_expected(0, radius), "Flat, query_batch 128")
    finally:
        ix.set_param("query_batch", 1024)


def test_flat_timing_keys(flat_ix):
    _, q = rr.flat_inputs()
    ix, radius = flat_ix[0], rr.FLAT_RADII[0][1]
    ix.set_param("profile", 1)
    try:
        lims, _, _ = ix.range_search(q, radius)
        assert ix.get_timing("range_results") == lims[-1]
        assert ix.get_timing("range_candidates") >= lims[-1]
        assert ix.get_timing("range_overflow_queries") == 0
        assert ix.get_timing("range_ms") > 0
    finally:
        ix.set_param("profile", 0)


# ------------------------------------------------------------------------------------------ IVF-Flat
@pytest.mark.parametrize("qtiles", [0, 4])
@pytest.mark.parametrize("nprobe", [1, 6, 40])
@pytest.mark.parametrize("metric", [0, 1])
def test_ivf_vs_oracle(ivf_ix, metric, nprobe, qtiles):
    c = rr.ivf_inputs()
    ix = ivf_ix[metric]
    ix.nprobe = nprobe
    ix.set_param("ivf_qtiles", qtiles)
    try:
        for radius in rr.IVF_RADII[metric]:
            want = rr.ivf_expected("ivf", metric, nprobe, radius, True)
            both_paths(ix, c.q, radius, want, f"IVF-Flat metric {metric} nprobe {nprobe} ivf_qtiles {qtiles} radius {radius}")
            if nprobe == c.nlist:      # every list probed: the Flat result on the same vectors
                ids = 7 * np.arange(c.n, dtype=np.int64) + 1000003
                fl = rr.flat_expected_of(c.q32, c.x32, metric, radius, ids)
                assert all(np.array_equal(a, b) for a, b in zip(want, fl))
    finally:
        ix.set_param("ivf_qtiles", 1)


@pytest.mark.parametrize("metric", [0, 1])
def test_ivf_nprobe_from_params(ivf_ix, metric, gpu):
    c = rr.ivf_inputs()
    ix, radius = ivf_ix[metric], rr.IVF_RADII[metric][0]
    ix.nprobe = 1
    got = ix.range_search(c.q, radius, params=gpu.SearchParametersIVF(nprobe=6))
    same(got, rr.ivf_expected("ivf", metric, 6, radius, True), "nprobe from SearchParametersIVF")
    assert ix.nprobe == 1


@pytest.mark.parametrize("metric", [0, 1])
def test_ivf_capacity_second_pass(ivf_ix, metric):
    c = rr.ivf_inputs()
    ix, radius = ivf_ix[metric], rr.IVF_RADII[metric][1]
    ix.nprobe = 6
    want = rr.ivf_expected("ivf", metric, 6, radius, True)
    assert np.diff(want[0]).max() > 1024
    ov0 = ix.get_timing("range_overflow_queries")
    ix.set_param("range_cand_cap", 1024)
    try:
        both_paths(ix, c.q, radius, want, f"IVF-Flat metric {metric}, range_cand_cap 1024")
    finally:
        ix.set_param("range_cand_cap", 0)
    assert ix.get_timing("range_overflow_queries") > ov0


@pytest.mark.parametrize("metric", [0, 1])
def test_ivf_d768_takes_a_filtered_form(gpu, metric):
    """d = 768, 50 probing queries per list: `search` would take the 128-query list scan, which has no filtered output"""
    c = sq_ref.inputs("D")
    ix = gpu.IndexIVFFlat(None, c.d, c.nlist, metric, device=0)
    ix.set_centroids(c.cen)
    ix.add(c.x)
    ix.nprobe = c.nprobe
    radius = rr.IVF768_RADII[metric]
    want = rr.ivf_expected("D", metric, c.nprobe, radius)
    assert 0 < np.median(np.diff(want[0])) < 5000
    both_paths(ix, c.q, radius, want, f"IVF-Flat d 768 metric {metric}")


@pytest.mark.parametrize("metric", [0, 1])
def test_ivf_two_phase_probe_selection(gpu, metric):
    """nlist = 12 800: the coarse selection runs over four segments of centroid scores, i.e. in its two-phase form (select_rows, nseg >= 4);
    the probes, and with them the result, must be the oracle's.  Radius: the median over the queries of the 20th best oracle score."""
    c = rr.wide_inputs()
    ix = gpu.IndexIVFFlat(None, c.d, c.nlist, metric, device=0)
    ix.set_centroids(c.cen)
    ix.add(c.x)
    ix.nprobe = c.nprobe
    D, _ = rr.ivf_full("wide", metric, c.nprobe)
    radius = float(np.median(D[:, 19]))
    want = rr.ivf_expected("wide", metric, c.nprobe, radius)
    counts = np.diff(want[0])
    print(f"metric {metric}: radius {radius}, results per query median {np.median(counts)} max {counts.max()}, non-empty lists {(c.sizes > 0).sum()}")
    assert 0 < np.median(counts) < 5000
    both_paths(ix, c.q, radius, want, f"IVF-Flat nlist {c.nlist} metric {metric}")


@pytest.mark.parametrize("qtiles", [2, 3, 8, 9])
def test_ivf_forced_group_sizes(ivf_ix, qtiles):
    """"ivf_qtiles" 2 and 3 ask for groups of 32 probing queries, 8 and 9 for more than the filtered scans have: 64"""
    c = rr.ivf_inputs()
    ix, radius = ivf_ix[0], rr.IVF_RADII[0][0]
    ix.nprobe = 6
    ix.set_param("ivf_qtiles", qtiles)
    try:
        both_paths(ix, c.q, radius, rr.ivf_expected("ivf", 0, 6, radius, True), f"IVF-Flat ivf_qtiles {qtiles}")
    finally:
        ix.set_param("ivf_qtiles", 1)


# ------------------------------------------------------------------------------------------ ties and edges
@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_ties_come_back_in_id_order(gpu, kind):
    """64 copies of one row score equal; with explicit ids in descending order the scan's index order is the reverse of the id order"""
    x, q = rr.flat_inputs()
    x = np.ascontiguousarray(x[:3000]).copy()
    dup = np.arange(100, 100 + 64 * 40, 40)
    x[dup] = x[7]
    ids = (5000 - np.arange(len(x))).astype(np.int64)
    if kind == "flat":
        ix = gpu.IndexFlatIP(x.shape[1], device=0)
    else:
        ix = gpu.IndexIVFFlat(None, x.shape[1], 4, 0, device=0)
        ix.set_centroids(x[[0, 1, 2, 3]].astype(F32))
        ix.nprobe = 4
    ix.add_with_ids(x, ids)
    qq = np.ascontiguousarray(x[[7, 9]])
    full = rr.flat_expected_of(qq, x, 0, -1e30, ids)
    s_dup = full[1][np.nonzero(full[2] == ids[7])[0][0]]
    radius = float(np.nextafter(s_dup, F32(-np.inf)))
    want = rr.flat_expected_of(qq, x, 0, radius, ids)
    assert (want[1][:want[0][1]] == s_dup).sum() == 65
    both_paths(ix, qq, radius, want, f"ties, {kind}")


def test_edges(flat_ix, gpu):
    _, q = rr.flat_inputs()
    ix = flat_ix[0]
    D, I = rr.flat_full(0)
    # a radius equal to an occurring fp32 score excludes that score
    radius = float(D[3, 5])
    assert D[3, 4] > D[3, 5]
    got = both_paths(ix, q[:8], radius, rr.flat_expected(0, radius, 8), "radius = an occurring score")
    assert got[0][4] - got[0][3] == 5
    # beyond the best score: empty rows
    top = float(D[:, 0].max())
    lims, Dg, Ig = ix.range_search(q, top)
    assert np.array_equal(lims, np.zeros(len(q) + 1, np.int64)) and len(Dg) == 0 and len(Ig) == 0
    # a query with a NaN component owns nothing
    qn = q[:6].astype(F32).copy()
    qn[2, 17] = np.nan
    want = list(rr.flat_expected(0, rr.FLAT_RADII[0][1], 6))
    n2 = want[0][3] - want[0][2]
    keep = np.ones(len(want[1]), bool)
    keep[want[0][2]:want[0][3]] = False
    want = (np.concatenate([want[0][:3], want[0][3:] - n2]), want[1][keep], want[2][keep])
    both_paths(ix, qn, rr.FLAT_RADII[0][1], want, "NaN query")
    # nq = 0, an empty index, a non-finite radius
    import torch
    empty = (np.zeros(1, np.int64), np.zeros(0, F32), np.zeros(0, np.int64))
    both_paths(ix, np.zeros((0, ix.d), F32), 1.0, empty, "nq = 0")
    both_paths(ix, np.zeros((0, ix.d), np.float16), 1.0, empty, "nq = 0, fp16")
    e = gpu.IndexFlatL2(ix.d, device=0)
    both_paths(e, q[:7], 10.0, (np.zeros(8, np.int64), empty[1], empty[2]), "empty index")
    both_paths(e, np.zeros((0, ix.d), F32), 10.0, empty, "empty index, nq = 0")
    for bad in (np.inf, -np.inf, np.nan):
        for qq in (q[:4], torch.as_tensor(np.ascontiguousarray(q[:4])).cuda()):
            with pytest.raises(RuntimeError, match="range_search"):
                ix.range_search(qq, bad)
    # everything beyond the best score, CUDA tensors
    tl, tD, tI = ix.range_search(torch.as_tensor(np.ascontiguousarray(q)).cuda(), top)
    assert tl.is_cuda and tD.is_cuda and tI.is_cuda and tl.dtype == torch.int64 and tD.dtype == torch.float32 and tI.dtype == torch.int64
    assert tl.cpu().tolist() == [0] * (len(q) + 1) and tD.numel() == 0 and tI.numel() == 0


# ------------------------------------------------------------------------------------------ fp32 storage
@pytest.mark.parametrize("metric", [0, 1])
def test_fp32_storage(gpu, metric):
    """values fp16 cannot represent: rows kept as fp32, queries rounded to fp16 inside the scan.  The fp64 sums may round differently from the
    oracle's: scores within 1 ulp, and with no oracle score within 8 ulp of the radius the id sets are equal"""
    x, q, radius = rr.fp32_case(metric)
    ix = gpu.IndexFlat(x.shape[1], metric, device=0)
    ix.add(x)
    assert ix.storage_dtype == "float32"
    D, I = rr._orc().flat_search(q, x, len(x), metric)
    assert rr.ulp_distance(D, np.full_like(D, radius)).min() > 8, "precondition: no oracle score within 8 ulp of the radius"
    wl, wD, wI = rr.cut(D, I, radius, metric)
    assert 100 < np.median(np.diff(wl)) < 2000
    import torch
    for got in (ix.range_search(q, radius), [a.cpu().numpy() for a in ix.range_search(torch.as_tensor(q).cuda(), radius)]):
        lims, Dg, Ig = got
        assert np.array_equal(lims, wl)
        for i in range(len(q)):
            a, b = slice(lims[i], lims[i + 1]), slice(wl[i], wl[i + 1])
            og, ow = np.argsort(Ig[a], kind="stable"), np.argsort(wI[b], kind="stable")
            assert np.array_equal(Ig[a][og], wI[b][ow])
            assert rr.ulp_distance(Dg[a][og], wD[b][ow]).max(initial=0) <= 1
            # best first, equal scores by id
            dd = Dg[a] if metric == 1 else -Dg[a]
            assert np.all((np.diff(dd) > 0) | ((np.diff(dd) == 0) & (np.diff(Ig[a]) > 0)))


# ------------------------------------------------------------------------------------------ after remove_ids
@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_after_remove_ids(gpu, kind):
    c = rr.ivf_inputs()
    n, metric, radius = 20000, 1, 30.0
    x, q = c.x[:n], c.q[:50]

    def make(rows, ids):
        if kind == "flat":
            ix = gpu.IndexFlat(c.d, metric, device=0)
        else:
            ix = gpu.IndexIVFFlat(None, c.d, c.nlist, metric, device=0)
            ix.set_centroids(c.cen)
            ix.nprobe = 6
        if ids is None:
            ix.add(rows)
        else:
            ix.add_with_ids(rows, ids)
        return ix
    ix = make(x, None)
    assert ix.remove_ids(gpu.IDSelectorRange(1500, 9000)) == 7500
    surv = np.concatenate([np.arange(1500), np.arange(9000, n)])
    # Flat renumbers the survivors 0 .. ntotal - 1; the IVF lists keep their ids
    fresh = make(np.ascontiguousarray(x[surv]), None if kind == "flat" else surv.astype(np.int64))
    got, want = ix.range_search(q, radius), fresh.range_search(q, radius)
    assert want[0][-1] > 0
    same(got, want, f"after remove_ids, {kind}")
    if kind == "flat":
        same(got, rr.flat_expected_of(q, x[surv], metric, radius), "after remove_ids, Flat against the oracle")


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_untouched(gpu, ivf_ix):
    import torch
    c = rr.ivf_inputs()
    x, q = np.ascontiguousarray(c.x[:4096]), c.q[:16]

    def refused(ix, call=None, q=q):
        before = ix.search(q, 5)
        with pytest.raises(RuntimeError, match="range_search"):
            (call or (lambda: ix.range_search(q, 1.0)))()
        after = ix.search(q, 5)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])

    pq = gpu.IndexIVFPQ(None, c.d, 8, 8, 8, 0, device=0)
    pq.train(x)
    pq.add(x)
    refused(pq)
    fpq = gpu.IndexPQ(c.d, 8, 8, 0, device=0)
    fpq.train(x)
    fpq.add(x)
    refused(fpq)
    sq = gpu.IndexIVFScalarQuantizer(None, c.d, 8, gpu.ScalarQuantizer.QT_8bit, 0, device=0)
    sq.train(x)
    sq.add(x)
    refused(sq)
    sh = gpu.IndexFlatIP(c.d, devices=[0, 0])
    sh.add(x)
    assert sh.nshards == 2
    refused(sh)
    rf = gpu.IndexRefineFlat(gpu.IndexFlatIP(c.d, device=0))
    rf.add(x)
    refused(rf)
    fl = rf.base_index
    refused(fl, lambda: fl.range_search(q, 1.0, params=gpu.SearchParameters(sel=gpu.IDSelectorRange(0, 100))))
    # an IVF-Flat index whose rows had to be widened to fp32
    x32, _, _ = rr.fp32_case(0)
    w = gpu.IndexIVFFlat(None, x32.shape[1], 4, 0, device=0)
    w.set_centroids(x32[:4])
    w.add(x32)
    assert w.storage_dtype == "float32"
    refused(w, q=x32[:16])
    # an open two-call search
    ix = ivf_ix[0]
    ix.nprobe = 6
    before = ix.search(q, 5)
    tq = torch.as_tensor(np.ascontiguousarray(q)).cuda()
    ix.search_prepass(tq, 5)
    try:
        with pytest.raises(RuntimeError, match="range_search"):
            ix.range_search(q, 1.0)
    finally:
        D2, I2 = ix.search_scan()
    assert np.array_equal(D2.cpu().numpy(), before[0]) and np.array_equal(I2.cpu().numpy(), before[1])
    after = ix.search(q, 5)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
