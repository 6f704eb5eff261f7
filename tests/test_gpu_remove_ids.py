"""GPU: Index.remove_ids (rsx_remove_ids, FAISS 1.8.0 semantics).

The bar, for every index kind and selector: the lists after the removal are the ones FAISS's own loops leave (restated here),
and a search of the index after the removal is, bit for bit, (a) the search of a fresh index built from those lists with the
same trained parameters and (b) the filtered search of the index before the removal with the complement selector.  One case
per kind is anchored on the CPU oracle over the surviving rows."""
import os

import numpy as np
import pytest

from util import assert_same_results

pytestmark = pytest.mark.gpu

N, NQ, NLIST, NPROBE = 12000, 48, 32, 6
# kind -> (d, M, metric, pq_layout or None)
KINDS = {
    "flat_ip": (96, 0, 0, None), "flat_l2": (96, 0, 1, None), "flat_ids": (96, 0, 0, None),
    "ivfflat_ip": (96, 0, 0, None), "ivfflat_l2": (96, 0, 1, None),
    "ivfpq_m96": (768, 96, 0, 2),      # sliced code layout
    "ivfpq_m64": (512, 64, 0, 1),      # rotated code layout
    "ivfpq_m96g": (768, 96, 0, 0),     # granule code layout
    "ivfpq_m16": (768, 16, 0, None),
    "ivfpq_l2": (256, 32, 1, None),
}
_DATA, _TRAINED = {}, {}


def _data(gpu, d):
    if d not in _DATA:
        x = gpu.synth_vectors(d, 16, 1234, 10000, 0.5, 0, N)
        q = gpu.synth_queries(d, 16, 1234, 10000, 0.5, N, 999, 0.1, 0, NQ)
        x[500:520] = x[7]            # exact score ties
        _DATA[d] = (x, q)
    return _DATA[d]


def _flat_ids():
    return (np.arange(N, dtype=np.int64) * 7 + 3)[::-1].copy()      # explicit ids: not positions, not sorted


def _new(gpu, kind, devices=None):
    d, M, metric, layout = KINDS[kind]
    dev = {"devices": devices} if devices else {"device": 0}
    if kind.startswith("flat"):
        return gpu.IndexFlat(d, metric, **dev)
    if kind.startswith("ivfflat"):
        ix = gpu.IndexIVFFlat(None, d, NLIST, metric, **dev)
    else:
        ix = gpu.IndexIVFPQ(None, d, NLIST, M, 8, metric, **dev)
        if layout is not None:
            ix.set_param("pq_layout", layout)
    if kind not in _TRAINED:
        x, _ = _data(gpu, d)
        ix.train(x[:6000])
        _TRAINED[kind] = (ix.get_centroids(), ix.get_codebooks() if kind.startswith("ivfpq") else None)
    else:
        ix.set_centroids(_TRAINED[kind][0])
        if kind.startswith("ivfpq"):
            ix.set_codebooks(_TRAINED[kind][1])
    ix.nprobe = NPROBE
    return ix


def _full(gpu, kind, devices=None):
    x, _ = _data(gpu, KINDS[kind][0])
    ix = _new(gpu, kind, devices)
    if kind == "flat_ids":
        ix.add_with_ids(x, _flat_ids())
    else:
        ix.add(x)
    return ix


def _lists(ix, kind):
    if kind.startswith("flat"):
        return [ix.get_list(0)]
    return [ix.get_list(l) for l in range(NLIST)]


def faiss_ivf_list_remove(ids, removed_fn):
    """DirectMap::remove_ids (NoMap): the literal loop -> the list's positions in their new order"""
    entry = list(range(len(ids)))
    j, l = 0, len(ids)
    while j < l:
        if removed_fn(ids[entry[j]]):
            l -= 1
            entry[j] = entry[l]
        else:
            j += 1
    return np.array(entry[:l], dtype=np.int64)


def _expected(kind, before, removed_mask_of):
    """lists after the removal: removed_mask_of(ids) -> bool array (what the selector says of each stored id / position)"""
    out = []
    if kind.startswith("flat"):
        payload, ids = before[0]
        rm = removed_mask_of(np.arange(len(ids)) if kind != "flat_ids" else ids)
        keep = np.nonzero(~rm)[0]
        new_ids = np.arange(len(keep), dtype=np.int64) if kind != "flat_ids" else ids[keep]
        return [(payload[keep], new_ids)]
    for payload, ids in before:
        rm = removed_mask_of(ids)
        pos = faiss_ivf_list_remove(ids, lambda i, s=dict(zip(ids.tolist(), rm.tolist())): s[int(i)])
        out.append((payload[pos], ids[pos]))
    return out


def _fresh(gpu, kind, lists):
    ix = _new(gpu, kind)
    if kind.startswith("flat"):
        payload, ids = lists[0]
        if len(ids):
            if kind == "flat_ids":
                ix.add_with_ids(payload, ids)
            else:
                ix.add(payload)
        return ix
    for l, (payload, ids) in enumerate(lists):
        if len(ids):
            ix.add_list(l, payload, ids)
    return ix


def _params(gpu, kind, sel):
    return gpu.SearchParameters(sel=sel) if kind.startswith("flat") else gpu.SearchParametersIVF(sel=sel, nprobe=NPROBE)


def _selectors(gpu, kind):
    """name -> (argument of remove_ids, selector of the same ids, removed(ids) as numpy)"""
    rng = np.random.default_rng(7)
    space = _flat_ids() if kind == "flat_ids" else np.arange(N, dtype=np.int64)
    some = rng.choice(space, N // 10, replace=False)
    batch = np.concatenate([some, some[:50], [-5, 10 ** 9]])           # duplicates and absent ids
    bits = rng.random(8 * N + 64) < 0.3
    bm = np.packbits(bits, bitorder="little")
    lo, hi = int(np.sort(space)[N // 4]), int(np.sort(space)[N // 2])
    arr = rng.choice(space, N // 100, replace=False)
    return {
        "range": (gpu.IDSelectorRange(lo, hi), gpu.IDSelectorRange(lo, hi), lambda i: (i >= lo) & (i < hi)),
        "batch": (gpu.IDSelectorBatch(batch), gpu.IDSelectorBatch(batch), lambda i: np.isin(i, batch)),
        "bitmap": (gpu.IDSelectorBitmap(bm), gpu.IDSelectorBitmap(bm),
                   lambda i: np.where((i >= 0) & (i < bits.size), bits[np.clip(i, 0, bits.size - 1)], False)),
        "not": (gpu.IDSelectorNot(gpu.IDSelectorRange(lo, hi)), gpu.IDSelectorNot(gpu.IDSelectorRange(lo, hi)),
                lambda i: ~((i >= lo) & (i < hi))),
        "array": (arr, gpu.IDSelectorBatch(arr), lambda i: np.isin(i, arr)),
    }


def _check_lists(ix, kind, want, what):
    got = _lists(ix, kind)
    for l, ((gp, gi), (wp, wi)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi), f"{what}: ids of list {l}"
        assert np.array_equal(gp, wp), f"{what}: payload of list {l}"


def _oracle(orc, kind, ix_lists, q, k):
    d, M, metric, _ = KINDS[kind]
    q32 = q.astype(np.float32)
    if kind.startswith("flat"):
        payload, ids = ix_lists[0]
        return orc.flat_search(q32, payload, k, metric, ids)
    cen, cb = _TRAINED[kind]
    assign = np.concatenate([np.full(len(i), l, np.int32) for l, (_, i) in enumerate(ix_lists)])
    ids = np.concatenate([i for _, i in ix_lists])
    payload = np.concatenate([p for p, _ in ix_lists])
    lm = orc.ListMajor(assign, ids, payload, NLIST)
    if kind.startswith("ivfflat"):
        return orc.ivfflat_search(metric, cen, lm, q32, NPROBE, k)
    return orc.ivfpq_search(cen, cb, lm, q32, NPROBE, k, metric=metric)


@pytest.mark.parametrize("kind", list(KINDS))
def test_remove_matches_faiss_and_fresh_index(gpu, orc, kind):
    _, q = _data(gpu, KINDS[kind][0])
    for name, (arg, sel, removed_of) in _selectors(gpu, kind).items():
        ix = _full(gpu, kind)
        what = f"{kind} {name}"
        before = _lists(ix, kind)
        ix.search(q, 1000)                          # IVF-PQ: the row-major code copy of this index state exists now
        filt = {k: ix.search(q, k, params=_params(gpu, kind, gpu.IDSelectorNot(sel))) for k in (10, 1000)}
        want = _expected(kind, before, removed_of)
        nrm = ix.remove_ids(arg)
        n_want = sum(len(i) for _, i in want)
        assert nrm == N - n_want and ix.ntotal == n_want, what
        _check_lists(ix, kind, want, what)
        fresh = _fresh(gpu, kind, want)
        for k in (10, 1000):
            D, I = ix.search(q, k)
            Df, If = fresh.search(q, k)
            assert_same_results(D, I, Df, If, f"{what} k={k} vs fresh")
            Ds, Is = filt[k]
            if kind in ("flat_ip", "flat_l2"):      # sequential ids: the survivors are renumbered in order
                old = np.nonzero(~removed_of(np.arange(N)))[0]
                Is = np.where(Is >= 0, np.searchsorted(old, np.maximum(Is, 0)), -1)
            assert_same_results(D, I, Ds, Is, f"{what} k={k} vs filtered search before")
            if name == "range" and k == 10:
                Do, Io = _oracle(orc, kind, want, q, k)
                assert_same_results(D, I, Do, Io, f"{what} vs oracle")
        assert ix.get_timing("remove_calls") >= 1 and ix.get_timing("removed") == nrm


@pytest.mark.parametrize("kind", ["flat_l2", "flat_ids", "ivfflat_l2", "ivfpq_m96", "ivfpq_m64"])
def test_remove_twice_everything_nothing_and_add(gpu, kind):
    x, q = _data(gpu, KINDS[kind][0])
    ix = _full(gpu, kind)
    space = _flat_ids() if kind == "flat_ids" else np.arange(N)
    first, second = space[::3], space[1::5]
    removed = np.isin(space, first) | np.isin(space, second)
    assert ix.remove_ids(first) == len(first)
    cur = ix.ntotal
    exp2 = np.isin(space, second) & ~np.isin(space, first)
    if kind in ("flat_l2",):        # sequential ids: the second selector sees the NEW positions
        exp2 = np.isin(np.arange(cur), second)
    assert ix.remove_ids(gpu.IDSelectorBatch(second)) == int(exp2.sum())
    if kind != "flat_l2":
        fresh = _fresh(gpu, kind, _expected_after_two(gpu, kind, first, second))
        for k in (10, 1000):
            assert_same_results(*ix.search(q, k), *fresh.search(q, k), f"{kind} twice k={k}")
        assert ix.ntotal == int((~removed).sum())
    # nothing: 0, index untouched
    n0 = ix.ntotal
    D0, I0 = ix.search(q, 100)
    assert ix.remove_ids(np.array([10 ** 12, -1])) == 0 and ix.ntotal == n0
    assert ix.remove_ids(gpu.IDSelectorRange(5, 5)) == 0
    assert_same_results(*ix.search(q, 100), D0, I0, f"{kind} nothing")
    # add without ids (sequential kinds): ids start at the new ntotal
    if kind != "flat_ids":
        ix.add(x[:100])
        _, ids = (ix.get_list(0) if kind.startswith("flat") else
                  (None, np.concatenate([ix.get_list(l)[1] for l in range(NLIST)])))
        assert set(range(n0, n0 + 100)) <= set(ids.tolist())
        n0 += 100
    # everything
    assert ix.remove_ids(gpu.IDSelectorNot(gpu.IDSelectorBatch(np.zeros(0, np.int64)))) == n0
    assert ix.ntotal == 0 and ix.remove_ids(np.arange(10)) == 0
    D, I = ix.search(q, 10)
    assert (I == -1).all() and np.isinf(D).all() and (np.sign(D) == (1 if KINDS[kind][2] else -1)).all()


def _expected_after_two(gpu, kind, first, second):
    ix = _full(gpu, kind)
    b = _lists(ix, kind)
    w = _expected(kind, b, lambda i: np.isin(i, first))
    return _expected(kind, w, lambda i: np.isin(i, second))


def test_stale_caches_mask_and_code_copy(gpu):
    """a filtered search with selector S, a removal, the same S again: the cached mask of S must not survive the removal;
    the k = 1000 search before the removal built the row-major code copy, which must not be reused"""
    kind = "ivfpq_m96"
    _, q = _data(gpu, KINDS[kind][0])
    ix = _full(gpu, kind)
    S = gpu.IDSelectorRange(0, N // 2)
    p = _params(gpu, kind, S)
    ix.search(q, 10, params=p)
    ix.search(q, 1000)
    rm = np.arange(0, N, 4)
    want = _expected(kind, _lists(ix, kind), lambda i: np.isin(i, rm))
    assert ix.remove_ids(rm) == len(rm)
    fresh = _fresh(gpu, kind, want)
    assert_same_results(*ix.search(q, 10, params=p), *fresh.search(q, 10, params=p), "filtered after removal")
    assert_same_results(*ix.search(q, 1000), *fresh.search(q, 1000), "k=1000 after removal")


def test_skewed_list_longer_than_a_tile(gpu):
    """one list of 60000 entries (a workgroup's tile is 8192 slots) next to short ones"""
    d, M = 64, 16
    rng = np.random.default_rng(3)
    ix = gpu.IndexIVFPQ(None, d, 8, M, 8, 0, device=0)
    cen = rng.standard_normal((8, d)).astype(np.float32)
    cb = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    ix.set_centroids(cen); ix.set_codebooks(cb); ix.nprobe = 8
    sizes = [60000, 5, 0, 700, 64, 65, 1, 3000]
    lists, nid = [], 0
    for l, n in enumerate(sizes):
        codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
        ids = np.arange(nid, nid + n, dtype=np.int64)
        nid += n
        lists.append((codes, ids))
        if n:
            ix.add_list(l, codes, ids)
    rm = rng.choice(nid, nid * 3 // 10, replace=False)
    before = [ix.get_list(l) for l in range(8)]
    assert nid == sum(sizes)
    assert ix.remove_ids(rm) == len(rm)
    for l, (p, i) in enumerate(before):
        pos = faiss_ivf_list_remove(i, lambda v, s=set(rm.tolist()): int(v) in s)
        gp, gi = ix.get_list(l)
        assert np.array_equal(gi, i[pos]) and np.array_equal(gp, p[pos]), f"list {l}"
    fresh = gpu.IndexIVFPQ(None, d, 8, M, 8, 0, device=0)
    fresh.set_centroids(cen); fresh.set_codebooks(cb); fresh.nprobe = 8
    for l in range(8):
        p, i = ix.get_list(l)
        if len(i):
            fresh.add_list(l, p, i)
    qq = rng.standard_normal((16, d)).astype(np.float32)
    for k in (10, 1000):
        assert_same_results(*ix.search(qq, k), *fresh.search(qq, k), f"skewed k={k}")


@pytest.mark.parametrize("kind", ["flat_ids", "ivfflat_l2", "ivfpq_m96", "ivfpq_m64"])
def test_round_trips_after_removal(gpu, tmp_path, kind):
    from rsx_faiss_io import write_faiss_index
    _, q = _data(gpu, KINDS[kind][0])
    ix = _full(gpu, kind)
    ix.remove_ids(np.arange(0, 20 * N, 3))
    ref = {k: ix.search(q, k) for k in (10, 1000)}
    gpu.write_index(ix, str(tmp_path / "a.rsx"))
    paths = [str(tmp_path / "a.rsx")]
    if kind != "flat_ids":
        write_faiss_index(ix, str(tmp_path / "a.faiss"))
        paths.append(str(tmp_path / "a.faiss"))
    for p in paths:
        back = gpu.read_index(p, device=0)
        if not kind.startswith("flat"):
            back.nprobe = NPROBE
        assert back.ntotal == ix.ntotal
        for k in (10, 1000):
            assert_same_results(*back.search(q, k), *ref[k], f"{kind} {os.path.basename(p)} k={k}")


@pytest.mark.parametrize("kind", ["flat_ids", "ivfflat_ip", "ivfpq_m96"])
def test_two_shard_handle(gpu, kind):
    _, q = _data(gpu, KINDS[kind][0])
    single, sh = _full(gpu, kind), _full(gpu, kind, devices=[0, 0])
    assert sh.nshards == 2
    space = _flat_ids() if kind == "flat_ids" else np.arange(N)
    sel = gpu.IDSelectorBatch(space[::7])
    assert sh.remove_ids(sel) == single.remove_ids(sel) == len(space[::7])
    assert sh.ntotal == single.ntotal
    for k in (10, 1000):
        assert_same_results(*sh.search(q, k), *single.search(q, k), f"{kind} two shards k={k}")
    assert sh.get_timing("removed") == len(space[::7])
    if kind != "flat_ids":          # later sequential adds: both number from the new ntotal
        x, _ = _data(gpu, KINDS[kind][0])
        sh.add(x[:50]); single.add(x[:50])
        assert_same_results(*sh.search(q, 20), *single.search(q, 20), f"{kind} two shards add after removal")


def test_refusals(gpu):
    import torch
    x, q = _data(gpu, 96)
    seq = gpu.IndexFlat(96, 0, devices=[0, 0])
    seq.add(x)
    with pytest.raises(RuntimeError, match="sequential ids"):
        seq.remove_ids(np.arange(10))
    assert seq.ntotal == N
    ls = _new(gpu, "ivfflat_ip")
    ls2 = gpu.IndexIVFFlat(None, 96, NLIST, 0, device=0)
    ls2.set_param("add_list_mod", 2); ls2.set_param("add_list_rem", 0)
    ls2.set_centroids(ls.get_centroids())
    ls2.add(x)
    with pytest.raises(RuntimeError, match="list shard"):
        ls2.remove_ids(np.arange(10))
    kind = "ivfpq_m96"
    _, q = _data(gpu, 768)
    ix = _full(gpu, kind)
    qt = torch.from_numpy(q).cuda()
    ix.search_prepass(qt, 25)
    try:
        with pytest.raises(RuntimeError, match="two-call"):
            ix.remove_ids(np.arange(10))
    finally:
        ix.search_scan()
    assert ix.ntotal == N and ix.remove_ids(np.arange(10)) == 10


def test_ivfpq_one_million(gpu):
    """about 1M vectors: lists of ~4000, 10 % removed at random; lists, counts and searches against a fresh index"""
    d, M, nlist, n = 256, 32, 256, 1 << 20
    x = gpu.synth_vectors(d, 64, 77, 10000, 0.5, 0, n)
    q = gpu.synth_queries(d, 64, 77, 10000, 0.5, n, 5, 0.1, 0, 64)
    ix = gpu.IndexIVFPQ(None, d, nlist, M, 8, 0, device=0)
    ix.train(x[:65536])
    ix.add(x)
    ix.nprobe = 16
    rng = np.random.default_rng(1)
    rm = rng.choice(n, n // 10, replace=False)
    before = [ix.get_list(l) for l in range(nlist)]
    ix.search(q, 1000)
    assert ix.remove_ids(rm) == len(rm) and ix.ntotal == n - len(rm)
    rmset = np.zeros(n, bool)
    rmset[rm] = True
    fresh = gpu.IndexIVFPQ(None, d, nlist, M, 8, 0, device=0)
    fresh.set_centroids(ix.get_centroids()); fresh.set_codebooks(ix.get_codebooks()); fresh.nprobe = 16
    for l, (p, i) in enumerate(before):
        pos = faiss_ivf_list_remove(i, lambda v: rmset[v])
        gp, gi = ix.get_list(l)
        assert np.array_equal(gi, i[pos]) and np.array_equal(gp, p[pos]), f"list {l}"
        if len(pos):
            fresh.add_list(l, p[pos], i[pos])
    for k in (10, 1000):
        assert_same_results(*ix.search(q, k), *fresh.search(q, k), f"1M k={k}")
