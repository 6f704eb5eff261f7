"""GPU: filtered search (rsx_search_sel: FAISS SearchParameters with an IDSelector).

The bar: a filtered search on the full index returns, bit for bit, what an unfiltered search returns on an index that holds
only the selected vectors — same trained parameters (set_centroids / set_codebooks), same ids, same insertion order.  That
subset index is searched through its own (fast, certified) routes, so every route knob forced on both sides checks the
filtered route against each of them; the CPU oracle on the selected rows anchors every index kind."""
import numpy as np
import pytest

from util import assert_same_results

pytestmark = pytest.mark.gpu

N, NQ, NLIST, NPROBE = 12000, 48, 32, 6
# kind -> (d, M, metric)
KINDS = {
    "flat_ip": (96, 0, 0), "flat_l2": (96, 0, 1),
    "ivfflat_ip": (96, 0, 0), "ivfflat_l2": (96, 0, 1),
    "ivfpq_m96": (768, 96, 0),        # sliced code layout
    "ivfpq_m64": (512, 64, 0),        # rotated code layout
    "ivfpq_m16": (768, 16, 0),        # dsub = 48
    "ivfpq_l2": (256, 32, 1),
}
_DATA = {}


def _data(gpu, d):
    if d not in _DATA:
        x = gpu.synth_vectors(d, 16, 1234, 10000, 0.5, 0, N)
        q = gpu.synth_queries(d, 16, 1234, 10000, 0.5, N, 999, 0.1, 0, NQ)
        x[500:520] = x[7]            # exact score ties across selected and unselected rows
        _DATA[d] = (x, q)
    return _DATA[d]


def _new(gpu, kind):
    d, M, metric = KINDS[kind]
    if kind.startswith("flat"):
        return gpu.IndexFlat(d, metric, device=0)
    if kind.startswith("ivfflat"):
        return gpu.IndexIVFFlat(None, d, NLIST, metric, device=0)
    return gpu.IndexIVFPQ(None, d, NLIST, M, 8, metric, device=0)


_FULL = {}


def _full(gpu, kind):
    if kind not in _FULL:
        x, _ = _data(gpu, KINDS[kind][0])
        ix = _new(gpu, kind)
        if not kind.startswith("flat"):
            ix.train(x[:6000])
            ix.nprobe = NPROBE
        ix.add(x)
        _FULL[kind] = ix
    return _FULL[kind]


def _subset(gpu, kind, keep, like):
    """unfiltered index of the selected rows only: the full index's parameters, ids and insertion order"""
    x, _ = _data(gpu, KINDS[kind][0])
    ix = _new(gpu, kind)
    if not kind.startswith("flat"):
        ix.set_centroids(like.get_centroids())
        if kind.startswith("ivfpq"):
            ix.set_codebooks(like.get_codebooks())
        ix.nprobe = like.nprobe
    ids = np.nonzero(keep)[0]
    if len(ids):
        ix.add_with_ids(x[ids], ids.astype(np.int64))
    return ix


def _selectors(gpu):
    rng = np.random.default_rng(3)
    ids = np.arange(N)
    half = rng.choice(N, N // 2, replace=False)
    one = rng.choice(N, N // 100, replace=False)
    tiny = np.array([11, 4000])                                  # 0.01 %: fewer than k -> padding
    bits = rng.random(N + 5) < 0.3
    bm = np.packbits(bits, bitorder="little")
    return {
        "all": (gpu.IDSelectorRange(0, N), np.ones(N, bool)),
        "batch50": (gpu.IDSelectorBatch(np.concatenate([half, half[:100]])), np.isin(ids, half)),
        "batch1": (gpu.IDSelectorBatch(np.concatenate([one, [N + 7, -3]])), np.isin(ids, one)),
        "batch001": (gpu.IDSelectorBatch(tiny), np.isin(ids, tiny)),
        "range": (gpu.IDSelectorRange(N // 4, N // 2), (ids >= N // 4) & (ids < N // 2)),
        "bitmap": (gpu.IDSelectorBitmap(bm), bits[:N]),
        "not_range": (gpu.IDSelectorNot(gpu.IDSelectorRange(1000, 9000)), ~((ids >= 1000) & (ids < 9000))),
        "empty": (gpu.IDSelectorBatch(np.zeros(0, np.int64)), np.zeros(N, bool)),
    }


def _params(gpu, kind, sel, nprobe=None):
    if kind.startswith("flat"):
        return gpu.SearchParameters(sel=sel)
    return gpu.SearchParametersIVF(sel=sel, nprobe=NPROBE if nprobe is None else nprobe)


@pytest.mark.parametrize("kind", list(KINDS))
def test_subset_equivalence(gpu, kind):
    import torch
    full = _full(gpu, kind)
    _, q = _data(gpu, KINDS[kind][0])
    for name, (sel, keep) in _selectors(gpu).items():
        sub = _subset(gpu, kind, keep, full)
        p = _params(gpu, kind, sel)
        for k in (1, 10, 100, 1000):
            D, I = full.search(q, k, params=p)
            Ds, Is = sub.search(q, k)
            assert_same_results(D, I, Ds, Is, f"{kind} {name} k={k}")
            assert np.isin(I[I >= 0], np.nonzero(keep)[0]).all()
            if keep.sum() < k:
                assert (I[:, keep.sum():] == -1).all()
                assert np.isinf(D[:, keep.sum():]).all() and (np.sign(D[:, keep.sum():]) == (1 if KINDS[kind][2] else -1)).all()
        qt = torch.from_numpy(q).cuda()
        D, I = full.search(qt, 10, params=p)
        Ds, Is = sub.search(q, 10)
        assert D.is_cuda and I.is_cuda
        assert_same_results(D.cpu().numpy(), I.cpu().numpy(), Ds, Is, f"{kind} {name} cuda queries")


@pytest.mark.parametrize("kind", ["flat_ip", "ivfflat_ip", "ivfpq_m96"])
def test_k4096(gpu, kind):
    full = _full(gpu, kind)
    _, q = _data(gpu, KINDS[kind][0])
    sel, keep = _selectors(gpu)["batch50"]
    sub = _subset(gpu, kind, keep, full)
    D, I = full.search(q[:8], 4096, params=_params(gpu, kind, sel))
    Ds, Is = sub.search(q[:8], 4096)
    assert_same_results(D, I, Ds, Is, f"{kind} k=4096")


@pytest.mark.parametrize("kind", list(KINDS))
def test_oracle_anchor(gpu, orc, kind):
    """the filtered search equals the CPU oracle run on the selected rows alone"""
    d, M, metric = KINDS[kind]
    full = _full(gpu, kind)
    x, q = _data(gpu, d)
    sel, keep = _selectors(gpu)["batch50"]
    ids = np.nonzero(keep)[0]
    k = 50
    D, I = full.search(q, k, params=_params(gpu, kind, sel))
    x32, q32 = x.astype(np.float32), q.astype(np.float32)
    if kind.startswith("flat"):
        Dr, Ir = orc.flat_search(q32, x32[ids], k, metric, ids=ids.astype(np.int64))
    else:
        cen = full.get_centroids()
        a, _ = orc.assign_ip(cen, x32[ids])
        if kind.startswith("ivfflat"):
            lm = orc.ListMajor(a, ids, x32[ids], NLIST)
            Dr, Ir = orc.ivfflat_search(metric, cen, lm, q32, NPROBE, k)
        else:
            cb = full.get_codebooks()
            lm = orc.ListMajor(a, ids, orc.pq_encode(cb, orc.residuals(cen, x32[ids], a)), NLIST)
            Dr, Ir = orc.ivfpq_search(cen, cb, lm, q32, NPROBE, k, metric=metric)
    assert_same_results(D, I, Dr, Ir, f"{kind} vs oracle")


ROUTES = {
    "flat_ip": [("flat_filter", 0), ("flat_filter", 1), ("flat_cert", 0)],
    "ivfflat_ip": [("ivf_filter", 0), ("ivf_filter", 1), ("ivf_filter", 2)],
    "ivfpq_m96": [("scan_kernel", 0), ("scan_kernel", 1), ("scan_kernel", 2), ("pq_fast", 0), ("pq_fast", 1), ("pq_filter", 0),
                  ("pq_filter", 1), ("pq_q8", 0), ("pq_q8", 2), ("pq_final_tab", 0), ("pq_final_tab", 2), ("pq_plain_codes", 0),
                  ("pq_plain_codes", 1), ("pq_fast_kp", 64), ("pq_log_cap", 256)],
    "ivfpq_m64": [("scan_kernel", 1), ("scan_kernel", 2), ("pq_fast", 0), ("pq_filter", 0), ("pq_final_tab", 2), ("pq_fast_kp", 64)],
}


@pytest.mark.parametrize("kind,knob,value", [(k, n, v) for k, lst in ROUTES.items() for n, v in lst])
def test_every_route(gpu, kind, knob, value):
    """each route knob forced on the full (filtered) and the subset (unfiltered) index alike.  A filtered search turns the in-scan
    candidate filters off (flat_filter / ivf_filter / pq_filter) and takes the score-row routes the other knobs still select, so
    this checks those filtered routes against every unfiltered route of the subset index"""
    _, q = _data(gpu, KINDS[kind][0])
    full = _subset(gpu, kind, np.ones(N, bool), _full(gpu, kind))      # a copy of the shared index that takes the knob
    sels = _selectors(gpu)
    full.set_param(knob, value)
    for name in ("batch50", "batch1", "batch001"):
        sel, keep = sels[name]
        sub = _subset(gpu, kind, keep, full)
        sub.set_param(knob, value)
        for k in (10, 100):
            D, I = full.search(q, k, params=_params(gpu, kind, sel))
            Ds, Is = sub.search(q, k)
            assert_same_results(D, I, Ds, Is, f"{kind} {knob}={value} {name} k={k}")


@pytest.mark.parametrize("kind", ["flat_ip", "ivfpq_m96", "ivfflat_l2"])
def test_mask_cache_and_staleness(gpu, kind):
    d = KINDS[kind][0]
    x, q = _data(gpu, d)
    n0 = 8000
    ix = _new(gpu, kind)
    if not kind.startswith("flat"):
        ix.train(x[:6000])
        ix.nprobe = NPROBE
    ix.add(x[:n0])
    sel = gpu.IDSelectorBitmap(np.packbits(np.arange(N) % 3 == 0, bitorder="little"))
    p = _params(gpu, kind, sel)
    builds0 = ix.get_timing("sel_mask_builds")
    for b in range(3):                           # one selector over several batches: ONE mask build
        ix.search(q[b * 16:(b + 1) * 16], 10, params=p)
    assert ix.get_timing("sel_mask_builds") == builds0 + 1
    assert ix.get_timing("filtered_queries") >= 48
    keep = np.arange(N) % 3 == 0
    D0, I0 = ix.search(q, 20, params=p)
    Ds, Is = _subset(gpu, kind, keep & (np.arange(N) < n0), ix).search(q, 20)
    assert_same_results(D0, I0, Ds, Is, f"{kind} before add")
    ix.add(x[n0:])                               # the next filtered search sees the grown index
    D1, I1 = ix.search(q, 20, params=p)
    assert ix.get_timing("sel_mask_builds") == builds0 + 2
    Ds, Is = _subset(gpu, kind, keep, ix).search(q, 20)
    assert_same_results(D1, I1, Ds, Is, f"{kind} after add")
    # a new selector object: a new mask; unfiltered searches are unaffected by a cached mask
    ix.search(q, 20, params=_params(gpu, kind, gpu.IDSelectorRange(0, 100)))
    assert ix.get_timing("sel_mask_builds") == builds0 + 3
    Du, Iu = ix.search(q, 20)
    Dr, Ir = _subset(gpu, kind, np.ones(N, bool), ix).search(q, 20)
    assert_same_results(Du, Iu, Dr, Ir, f"{kind} unfiltered after filtered")


def test_nprobe_override(gpu):
    full = _full(gpu, "ivfpq_m96")
    _, q = _data(gpu, 768)
    sel, _ = _selectors(gpu)["batch50"]
    assert full.nprobe == NPROBE
    D, I = full.search(q, 20, params=gpu.SearchParametersIVF(sel=sel, nprobe=11))
    assert full.nprobe == NPROBE
    full.nprobe = 11
    try:
        Dr, Ir = full.search(q, 20, params=gpu.SearchParametersIVF(sel=sel, nprobe=11))
        assert_same_results(D, I, Dr, Ir, "override = index.nprobe")
        Du, Iu = full.search(q, 20)
        D2, I2 = full.search(q, 20, params=gpu.SearchParametersIVF(nprobe=11))      # no selector: only the override
        assert_same_results(D2, I2, Du, Iu, "nprobe only")
    finally:
        full.nprobe = NPROBE
    # the FAISS default nprobe = 1 of SearchParametersIVF, and the type rule
    full.nprobe = 1
    try:
        Dr, Ir = full.search(q, 20, params=gpu.SearchParametersIVF(sel=sel))
    finally:
        full.nprobe = NPROBE
    D1, I1 = full.search(q, 20, params=gpu.SearchParametersIVF(sel=sel))
    assert_same_results(D1, I1, Dr, Ir, "default nprobe 1")
    assert full.nprobe == NPROBE
    with pytest.raises(RuntimeError, match="IndexIVF params have incorrect type"):
        full.search(q, 20, params=gpu.SearchParameters(sel=sel))
    with pytest.raises(RuntimeError):            # an error inside the library also restores index.nprobe
        full.search(q, 5000, params=gpu.SearchParametersIVF(sel=sel, nprobe=3))
    assert full.nprobe == NPROBE


@pytest.mark.parametrize("kind", ["flat_ip", "ivfpq_m96"])
def test_in_process_sharded_handle(gpu, kind):
    d = KINDS[kind][0]
    x, q = _data(gpu, d)
    full = _full(gpu, kind)
    sh = gpu.IndexFlatIP(d, devices=[0, 0]) if kind == "flat_ip" else gpu.IndexIVFPQ(None, d, NLIST, KINDS[kind][1], 8, 0, devices=[0, 0])
    if kind != "flat_ip":
        sh.set_centroids(full.get_centroids()); sh.set_codebooks(full.get_codebooks()); sh.nprobe = NPROBE
    sh.add(x)
    for name in ("batch50", "batch001", "range"):
        sel, _ = _selectors(gpu)[name]
        p = _params(gpu, kind, sel)
        D, I = sh.search(q, 30, params=p)
        Dr, Ir = full.search(q, 30, params=p)
        assert_same_results(D, I, Dr, Ir, f"sharded {kind} {name}")


def test_sharded_searcher_id_range_and_list_shards(gpu):
    """ShardedSearcher's translation in one process (local_params + a host merge; tests/test_gpu_selector_ranks.py runs
    ShardedSearcher.search itself with two real ranks): two id-range ranks (local ids, selector shifted by id_offset) and two list-shard ranks
    (two-call form: the filtered pre-pass) searched on one GPU and merged == the single filtered index"""
    import torch
    import sharded
    kind = "ivfpq_m96"
    x, q = _data(gpu, 768)
    full = _full(gpu, kind)
    cut = 5003
    for name in ("batch50", "bitmap", "not_range", "batch001"):
        sel, _ = _selectors(gpu)[name]
        p = _params(gpu, kind, sel)
        Dr, Ir = full.search(q, 25, params=p)
        # id-range ranks
        outs = []
        for lo, hi in ((0, cut), (cut, N)):
            r = _new(gpu, kind)
            r.set_centroids(full.get_centroids()); r.set_codebooks(full.get_codebooks()); r.nprobe = NPROBE
            r.add(x[lo:hi])
            s = sharded.ShardedSearcher.__new__(sharded.ShardedSearcher)
            s.index, s.id_offset = r, lo
            D, I = r.search(q, 25, params=s.local_params(p))
            outs.append((D, np.where(I >= 0, I + lo, -1)))
        Dm, Im = sharded.merge_topk_host(np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), 0)
        assert_same_results(Dm, Im, Dr, Ir, f"id-range ranks {name}")
        # list-shard ranks, two-call form
        ranks = []
        for rem in range(2):
            r = _new(gpu, kind)
            r.set_param("add_list_mod", 2); r.set_param("add_list_rem", rem)
            r.set_centroids(full.get_centroids()); r.set_codebooks(full.get_codebooks()); r.nprobe = NPROBE
            r.add(x)
            ranks.append(r)
        qt = torch.from_numpy(q).cuda()
        taus = [r.search_prepass(qt, 25, p) for r in ranks]
        sharded.raise_thresholds(taus)
        res = [r.search_scan() for r in ranks]
        Dm, Im = sharded.merge_topk_host(np.stack([a.cpu().numpy() for a, _ in res]), np.stack([b.cpu().numpy() for _, b in res]), 0)
        assert_same_results(Dm, Im, Dr, Ir, f"list-shard ranks {name}")
