"""GPU: the routes of IndexIVFScalarQuantizer (kind 4) that the input sets of test_gpu_sq.py never take, each forced by its own input set
and proved by a counter: the exact re-run of queries the certificate cannot clear (k_sq_exact_scores), candidate rows that overflow (per
query and through the unfiltered rescan), rows scanned in several and in ragged slices at d % 4 != 0, and k_finalize at K' 4096 / 8192.
Every result is compared with the oracle's IVF-Flat search over the stored vectors.  Inputs, expected results and the id rule:
tests/sq_ref.py; their preconditions: tests/test_sq_routes_host.py."""
import numpy as np
import pytest

import sq_ref
import test_gpu_sq as base

pytestmark = pytest.mark.gpu
F32 = np.float32
_built = {}
COMBOS = pytest.mark.parametrize("metric,by_residual", [(m, r) for m in (0, 1) for r in (False, True)])


def built(gpu, name, metric, by_residual):
    """one populated index per (route set, metric, residual setting); the crowd sets carry their own ids"""
    key = (name, metric, by_residual)
    if key not in _built:
        c = sq_ref.inputs(name)
        t, _, _ = sq_ref.quantised(name, by_residual)
        ix = base.make_index(gpu, c.d, c.nlist, metric, by_residual, c.cen, t)
        if hasattr(c, "ids"):
            ix.add_with_ids(c.x, c.ids)
        else:
            ix.add(c.x)
        ix.nprobe = c.nprobe
        _built[key] = ix
    return _built[key]


def search(ix, q, k, metric, Dk1, Ik1, filt, what, fb_min, fb_max, cap=0.02, capped=None):
    """one search with cleared counters: the kind's scan ran, fallback_queries within [fb_min, fb_max], the result the oracle's"""
    ix.set_param("ivf_filter", filt)
    ix.set_param("profile", 0)          # clears the counters
    D, I = ix.search(q, k)
    assert ix.get_timing("ivfsq_scan_launches") > 0, what
    fb = ix.get_timing("fallback_queries")
    print(f"{what}: fallback_queries {fb:.0f} of {len(q)} (wanted {fb_min} .. {fb_max:.1f})")
    assert fb_min <= fb <= fb_max, what
    sq_ref.check_result(D, I, Dk1, Ik1, k, metric, what, cap, capped)
    return D, I


def crowd_bounds(c):
    """every crowd query is re-run; of the others at most the kind's 5 %"""
    n = int(c.is_crowd_q.sum())
    return n, n + 0.05 * (c.nq - n)


# ------------------------------------------------------------------------------------------ 1. the exact re-run, forced (set E)
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("nprobe", [4, 1000])
@pytest.mark.parametrize("filt", [0, 2])
@COMBOS
def test_crowd_queries_are_rerun_exactly(gpu, metric, by_residual, filt, nprobe, k):
    """300 copies of a stored row with DESCENDING ids: the scan keeps the first K' of them by column, the certificate cannot clear the six
    queries at the crowd, and the exact re-run returns the copies by ascending id"""
    c = sq_ref.inputs("E")
    ix = built(gpu, "E", metric, by_residual)
    Dk1, Ik1 = sq_ref.expected("E", metric, by_residual, k + 1, None, nprobe)
    try:
        ix.nprobe = nprobe
        search(ix, c.q, k, metric, Dk1, Ik1, filt, f"set E k {k} nprobe {nprobe} metric {metric} by_residual {by_residual} ivf_filter {filt}",
               *crowd_bounds(c), capped=~c.is_crowd_q)
    finally:
        ix.nprobe = c.nprobe


@pytest.mark.parametrize("nq", [40, 6])
@COMBOS
def test_batches_of_crowd_queries_only(gpu, metric, by_residual, nq):
    """every query of the batch takes the re-run: 40 behind the fast coarse quantiser, 6 (fewer than 32) behind the exact one"""
    c = sq_ref.inputs("E")
    ix = built(gpu, "E", metric, by_residual)
    Dk1, Ik1 = sq_ref.expected("E", metric, by_residual, 11, nq, None, "crowd")
    for filt in (0, 2):
        search(ix, c.qsets["crowd"][:nq], 10, metric, Dk1, Ik1, filt, f"set E, {nq} crowd queries, metric {metric} by_residual {by_residual} ivf_filter {filt}",
               nq, nq, capped=np.zeros(nq, bool))


@pytest.mark.parametrize("metric", [0, 1])
def test_rerun_walks_empty_short_and_ragged_lists(gpu, orc, metric):
    """test_gpu_sq.py's two equal centroids (the second one's list stays empty) and a list cut to 5 rows, under the crowd and with every
    list probed: the re-run's 16-column walk crosses an empty list, a list shorter than 16 rows and lists whose length is no multiple of 16"""
    c = sq_ref.inputs("E")
    cen = c.cen.copy(); cen[7] = cen[3]
    a, _ = orc.assign_ip(cen, c.x32)
    assert (a == 7).sum() == 0 and a[c.r0] != 5
    keep = np.ones(c.n, bool)
    keep[np.nonzero(a == 5)[0][5:]] = False               # list 5 keeps 5 rows
    x, ids = c.x32[keep], c.ids[keep]
    sizes = np.bincount(a[keep], minlength=c.nlist)
    assert sizes[7] == 0 and sizes[5] == 5 and (sizes % 16 != 0).sum() >= 8
    t = sq_ref.train(orc.residuals(cen, x, a[keep]))
    (Dk1, Ik1), _, _ = base._oracle(orc, cen, x, ids, t, True, c.q32, metric, c.nlist, 11)
    ix = base.make_index(gpu, c.d, c.nlist, metric, True, cen, t)
    ix.add_with_ids(x, ids)
    ix.nprobe = c.nlist
    assert np.array_equal(ix.list_sizes(), sizes)
    for filt in (0, 2):
        search(ix, c.q32, 10, metric, Dk1, Ik1, filt, f"crowd + empty + short list, metric {metric} ivf_filter {filt}", *crowd_bounds(c),
               capped=~c.is_crowd_q)


@pytest.mark.parametrize("metric", [0, 1])
def test_cuda_tensor_queries_and_split_calls_return_the_same_bits(gpu, metric):
    import torch
    c = sq_ref.inputs("E")
    ix = built(gpu, "E", metric, True)
    Dk1, Ik1 = sq_ref.expected("E", metric, True, 11, None, 4)
    lo, hi = crowd_bounds(c)
    what = f"set E metric {metric}"
    D0, I0 = search(ix, c.q, 10, metric, Dk1, Ik1, 2, what, lo, hi, capped=~c.is_crowd_q)
    ix.set_param("profile", 0)
    Dc, Ic = ix.search(torch.as_tensor(c.q).cuda(), 10)
    assert Dc.is_cuda and Ic.is_cuda and Dc.dtype == torch.float32 and Ic.dtype == torch.int64
    assert lo <= ix.get_timing("fallback_queries") <= hi
    assert np.array_equal(Dc.cpu().numpy().view(np.uint32), D0.view(np.uint32)) and np.array_equal(Ic.cpu().numpy(), I0), f"{what}: CUDA tensor queries"
    try:
        ix.set_param("query_batch", 16)            # five internal batches, the crowd queries spread over four of them
        ix.set_param("profile", 0)
        Ds, Is = ix.search(c.q, 10)
        assert lo <= ix.get_timing("fallback_queries") <= hi
    finally:
        ix.set_param("query_batch", 1024)
    assert np.array_equal(Ds.view(np.uint32), D0.view(np.uint32)) and np.array_equal(Is, I0), f"{what}: query_batch 16"


# ------------------------------------------------------------------------------------------ 2. overflowing candidate rows (set F)
@COMBOS
def test_overflow_of_two_queries_is_settled_per_query(gpu, metric, by_residual):
    """IVF-Flat's test_ivfflat_filter_overflow_of_a_few_queries_is_settled_per_query for this kind: k_finalize flags the two overflowed rows'
    queries and they alone join the exact re-run"""
    c = sq_ref.inputs("F")
    ix = built(gpu, "F", metric, by_residual)
    Dk1, Ik1 = sq_ref.expected("F", metric, by_residual, 11, None, None, "a")
    search(ix, c.qsets["a"], 10, metric, Dk1, Ik1, 2, f"set F, two overflowing rows, metric {metric} by_residual {by_residual}", 2, 2 + 0.05 * (c.nq - 2))
    assert ix.get_timing("ivf_filter_overflow_queries") == 2, "exactly the two adversarial queries overflow"
    assert ix.get_timing("ivfsq_scan_launches") == 2, "the pre-pass and the filtered scan"


@COMBOS
def test_overflow_of_five_queries_rescans_the_batch_or_is_settled_on_request(gpu, metric, by_residual):
    """five overflowed rows are more than max(2, nq / 128): the batch leaves through the unfiltered rescan (three scan launches: pre-pass,
    filtered scan, unfiltered scan) — or, with ivf_overflow_max 8, the five queries join the exact re-run"""
    c = sq_ref.inputs("F")
    ix = built(gpu, "F", metric, by_residual)
    Dk1, Ik1 = sq_ref.expected("F", metric, by_residual, 11, None, None, "b")
    what = f"set F, five overflowing rows, metric {metric} by_residual {by_residual}"
    search(ix, c.qsets["b"], 10, metric, Dk1, Ik1, 2, what + ", rescan", 0, 0.05 * c.nq)
    assert ix.get_timing("ivf_filter_overflow_queries") == 0
    assert ix.get_timing("ivfsq_scan_launches") == 3, "pre-pass, filtered scan, unfiltered scan"
    try:
        ix.set_param("ivf_overflow_max", 8)
        search(ix, c.qsets["b"], 10, metric, Dk1, Ik1, 2, what + ", ivf_overflow_max 8", 5, 5 + 0.05 * (c.nq - 5))
        assert ix.get_timing("ivf_filter_overflow_queries") == 5
        assert ix.get_timing("ivfsq_scan_launches") == 2
    finally:
        ix.set_param("ivf_overflow_max", 0)


# ------------------------------------------------------------------------------------------ 3. long and ragged rows (sets G, H)
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("filt", [0, 2])
@pytest.mark.parametrize("qtiles", [0, 4])
@COMBOS
@pytest.mark.parametrize("name", ["G", "H"])
def test_rows_of_several_and_of_ragged_slices(gpu, name, metric, by_residual, qtiles, filt, k):
    """G (rows of 1152 bytes): slices of 1024 + 128 dimensions in the 16-query form, 4 x 256 + 128 in the 64-query form.  H (320 bytes,
    d = 301): one slice of five K steps, or 256 + 64.  The crowd of 40 sends four queries through k_sq_exact_scores and the second re-score of
    k_finalize at these widths."""
    c = sq_ref.inputs(name)
    ix = built(gpu, name, metric, by_residual)
    Dk1, Ik1 = sq_ref.expected(name, metric, by_residual, k + 1, None, None)
    try:
        ix.set_param("ivf_qtiles", qtiles)
        search(ix, c.q, k, metric, Dk1, Ik1, filt, f"set {name} k {k} ivf_qtiles {qtiles} metric {metric} by_residual {by_residual} ivf_filter {filt}",
               *crowd_bounds(c), capped=~c.is_crowd_q)
    finally:
        ix.set_param("ivf_qtiles", 1)


@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("name", ["G", "H"])
def test_codes_ids_and_order_of_every_list(gpu, name, by_residual):
    c = sq_ref.inputs(name)
    _, codes, _ = sq_ref.quantised(name, by_residual)
    ix = built(gpu, name, 0, by_residual)
    assert ix.ntotal == c.n and ix.code_size == c.d and ix.by_residual == by_residual
    assert np.array_equal(ix.list_sizes(), c.sizes)
    for l in range(c.nlist):
        want = np.nonzero(c.assign == l)[0]         # insertion order
        got_codes, got_ids = ix.get_list(l)
        assert got_codes.dtype == np.uint8 and got_codes.shape == (len(want), c.d)
        assert np.array_equal(got_ids, c.ids[want]), f"list {l}"
        assert np.array_equal(got_codes, codes[want]), f"list {l}"


@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("name", ["G", "H"])
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


@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("name", ["G", "H"])
def test_reconstruct_batch(gpu, name, by_residual):
    c = sq_ref.inputs(name)
    _, _, xhat = sq_ref.quantised(name, by_residual)
    ix = built(gpu, name, 1, by_residual)
    rows = np.concatenate([np.random.RandomState(3).choice(c.n - c.copies, 90, replace=False), c.n - 1 - np.arange(10)])
    got = ix.reconstruct_batch(c.ids[rows])
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), xhat[rows].view(np.uint32))


# ------------------------------------------------------------------------------------------ 4. large k (set D)
def _large_k(gpu, metric, by_residual, filt, nprobe, k, nq):
    c = sq_ref.inputs("D")
    ix = base.built(gpu, "D", metric, by_residual)
    Dk1, Ik1 = sq_ref.expected("D", metric, by_residual, k + 1, nq, nprobe)
    try:
        ix.nprobe = nprobe
        D, I = search(ix, c.q[:nq], k, metric, Dk1, Ik1, filt, f"set D k {k} nq {nq} nprobe {nprobe} metric {metric} by_residual {by_residual} ivf_filter {filt}",
                      0, 0.05 * nq, cap=0.05)
    finally:
        ix.nprobe = c.nprobe
    return D, I


@pytest.mark.parametrize("k", [3000, 4096])
@pytest.mark.parametrize("nprobe", [8, 16])
@pytest.mark.parametrize("filt", [0, 2])
@COMBOS
def test_large_k(gpu, metric, by_residual, filt, nprobe, k):
    """K' = 4096, and K' = 8192 where k_finalize no longer holds the probe table in LDS; nprobe 8 leaves many results padded, nprobe 16 fills
    the state rows"""
    D, I = _large_k(gpu, metric, by_residual, filt, nprobe, k, 40)
    if nprobe == 8:
        assert (I == -1).any() and (D[I == -1] == (-np.inf if metric == 0 else np.inf)).all()
    else:
        assert (I[:, -1] >= 0).mean() >= 0.9


@COMBOS
def test_large_k_in_the_64_query_form(gpu, metric, by_residual):
    _large_k(gpu, metric, by_residual, 0, 16, 4096, 200)
