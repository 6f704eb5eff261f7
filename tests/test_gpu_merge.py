"""GPU: Index.merge_from / IndexIVF.copy_subset_to (rsx_merge_from, rsx_copy_subset_to; FAISS 1.8.0 semantics).

The bar: an index merged from parts is indistinguishable from ONE index that was fed all the rows — ntotal, every list's payload and
ids bit for bit, search results bit for bit — and a subset copy holds exactly the entries the numpy statement of FAISS's rules
(merge_ref.py) selects, in list order, while its source stays as it was.  The single index of every kind is built once and never
changed."""
import numpy as np
import pytest

import merge_ref
from util import assert_same_results

pytestmark = pytest.mark.gpu

N, NQ, NPROBE = 12000, 48, 6
PARTS = (5000, 1, 0, 6999)
# kind -> (family, d, M, metric, pq_layout or None, nlist, by_residual)
KINDS = {
    "flat_ip": ("flat", 96, 0, 0, None, 1, None), "flat_l2": ("flat", 96, 0, 1, None, 1, None), "flat_ids": ("flat", 96, 0, 0, None, 1, None),
    "ivfflat_ip": ("ivfflat", 96, 0, 0, None, 32, None), "ivfflat_l2": ("ivfflat", 96, 0, 1, None, 32, None),
    "ivfpq_m96": ("ivfpq", 768, 96, 0, 2, 8, None),       # sliced code layout: lists of ~1500 rows span three 512-row groups
    "ivfpq_m64": ("ivfpq", 512, 64, 0, 1, 8, None),       # rotated
    "ivfpq_m96g": ("ivfpq", 768, 96, 0, 0, 8, None),      # granule
    "ivfpq_m96r": ("ivfpq", 768, 96, 0, 1, 8, None),      # rotated, M = 96 (half phase)
    "ivfpq_m64g": ("ivfpq", 512, 64, 0, 0, 8, None),
    "ivfpq_m16": ("ivfpq", 768, 16, 0, None, 8, None),
    "ivfpq_m32_l2": ("ivfpq", 256, 32, 1, None, 8, None),
    "ivfsq_res": ("ivfsq", 96, 0, 1, None, 32, True), "ivfsq_nores": ("ivfsq", 96, 0, 0, None, 32, False),
    "pq": ("pq", 256, 32, 0, None, 1, None), "sq": ("sq", 96, 0, 1, None, 1, None),
}
MERGE_KINDS = [k for k in KINDS if k not in ("ivfpq_m96r", "ivfpq_m64g")]
_DATA, _TRAINED, _FULL = {}, {}, {}


def _data(gpu, d):
    if d not in _DATA:
        x = gpu.synth_vectors(d, 16, 1234, 10000, 0.5, 0, N)
        q = gpu.synth_queries(d, 16, 1234, 10000, 0.5, N, 999, 0.1, 0, NQ)
        x[500:520] = x[7]            # a run of exact duplicates: score ties across the parts' boundary rules
        _DATA[d] = (x, q)
    return _DATA[d]


def _flat_ids():
    return (np.arange(N, dtype=np.int64) * 7 + 3)[::-1].copy()      # explicit ids: not positions, not sorted


def _is_ivf(kind):
    return KINDS[kind][0] in ("ivfflat", "ivfpq", "ivfsq")


def _new(gpu, kind, layout="kind", **dev):
    fam, d, M, metric, lay, nlist, byres = KINDS[kind]
    dev = dev or {"device": 0}
    if fam == "flat":
        return gpu.IndexFlat(d, metric, **dev)
    if fam == "ivfflat":
        ix = gpu.IndexIVFFlat(None, d, nlist, metric, **dev)
    elif fam == "ivfpq":
        ix = gpu.IndexIVFPQ(None, d, nlist, M, 8, metric, **dev)
    elif fam == "ivfsq":
        ix = gpu.IndexIVFScalarQuantizer(None, d, nlist, 0, metric, byres, **dev)
    elif fam == "pq":
        ix = gpu.IndexPQ(d, M, 8, metric, **dev)
    else:
        ix = gpu.IndexScalarQuantizer(d, 0, metric, **dev)
    lay = lay if layout == "kind" else layout
    if fam in ("ivfpq", "pq") and lay is not None:
        ix.set_param("pq_layout", lay)
    key = (fam, d, M, metric, nlist, byres)      # trained once per parameter set, shared by every handle (and every code layout) of it
    if key not in _TRAINED:
        ix.train(_data(gpu, d)[0][:6000])
        _TRAINED[key] = (ix.get_centroids() if _is_ivf(kind) else None, ix.get_codebooks() if fam in ("ivfpq", "pq") else None,
                         ix.sq.trained.copy() if fam in ("ivfsq", "sq") else None)
    else:
        cen, cb, sq = _TRAINED[key]
        if cen is not None:
            ix.set_centroids(cen)
        if cb is not None:
            ix.set_codebooks(cb)
        if sq is not None:
            ix.set_sq_trained(sq)
    if _is_ivf(kind):
        ix.nprobe = NPROBE
    return ix


def _add(ix, kind, lo, hi):
    x = _data(None, KINDS[kind][1])[0]
    if hi <= lo:
        return
    if kind == "flat_ids":
        ix.add_with_ids(x[lo:hi], _flat_ids()[lo:hi])
    else:
        ix.add(x[lo:hi])


def _lists(ix):
    return [ix.get_list(l) for l in range(len(ix.list_sizes()))]


def _searches(ix, q):
    import torch
    out = {}
    for k in (10, 100):
        out[k] = ix.search(q, k)
    D, I = ix.search(torch.from_numpy(np.ascontiguousarray(q)).cuda(), 10)
    out["cuda"] = (D.cpu().numpy(), I.cpu().numpy())
    return out


def _full(gpu, kind):
    """the index that was fed all rows at once, its lists and its search results: built once, never changed"""
    if kind not in _FULL:
        _data(gpu, KINDS[kind][1])
        ix = _new(gpu, kind)
        _add(ix, kind, 0, N)
        _FULL[kind] = (ix, _lists(ix), _searches(ix, _data(gpu, KINDS[kind][1])[1]))
    return _FULL[kind]


def _assert_lists_equal(got, want, what):
    assert len(got) == len(want), what
    for l, ((pg, ig), (pw, iw)) in enumerate(zip(got, want)):
        assert np.array_equal(ig, iw), f"{what}: ids of list {l} differ"
        assert pg.dtype == pw.dtype and pg.shape == pw.shape and np.array_equal(pg.view(np.uint8), pw.view(np.uint8)), f"{what}: payload of list {l} differs"


def _assert_same_index(ix, full, q, what):
    fx, flists, fres = full
    assert ix.ntotal == fx.ntotal, what
    assert np.array_equal(ix.list_sizes(), fx.list_sizes()), what
    _assert_lists_equal(_lists(ix), flists, what)
    res = _searches(ix, q)
    for key in fres:
        assert_same_results(res[key][0], res[key][1], fres[key][0], fres[key][1], f"{what} search {key}")


def _parts(gpu, kind, layouts=None, sizes=PARTS):
    """the rows split into parts of `sizes`, one index per part (layouts: per-part code layout, else the kind's)"""
    _data(gpu, KINDS[kind][1])
    out, lo = [], 0
    for i, n in enumerate(sizes):
        ix = _new(gpu, kind) if layouts is None else _new(gpu, kind, layout=layouts[i])
        _add(ix, kind, lo, lo + n)
        out.append(ix)
        lo += n
    return out


def _merge_all(kind, parts):
    dst = parts[0]
    for src in parts[1:]:
        dst.merge_from(src, dst.ntotal if _is_ivf(kind) else 0)
    return dst


def _assert_emptied(gpu, kind, src, q):
    assert src.ntotal == 0 and int(src.list_sizes().sum()) == 0 and src.is_trained
    D, I = src.search(q, 10)
    assert (I == -1).all(), "an emptied source returns only padding"
    _add(src, kind, 0, 10)
    assert src.ntotal == 10


# ---------------------------------------------------------------------------------------------------------
# 1. merge equals one index
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MERGE_KINDS)
def test_merge_equals_one_index(gpu, orc, kind):
    full = _full(gpu, kind)
    x, q = _data(gpu, KINDS[kind][1])
    parts = _parts(gpu, kind)
    dst = _merge_all(kind, parts)
    _assert_same_index(dst, full, q, kind)
    assert dst.get_timing("merge_rows") == N - PARTS[0]
    if kind != "flat_ids":
        assert dst._get("explicit_ids") == 0, "sequential adds merged with add_id = ntotal are sequential ids"
    for src in parts[1:]:
        _assert_emptied(gpu, kind, src, q)
    if kind.startswith("ivfflat"):      # ... and directly against the CPU oracle over the concatenated rows
        metric, nlist = KINDS[kind][3], KINDS[kind][5]
        cen = dst.get_centroids()
        xf = x.astype(np.float32)
        a, _ = orc.assign_ip(cen, xf)
        lm = orc.ListMajor(a, np.arange(N), xf, nlist)
        D, I = dst.search(q, 10)
        Dr, Ir = orc.ivfflat_search(metric, cen, lm, q.astype(np.float32), NPROBE, 10)
        assert np.array_equal(I, Ir)
        assert np.allclose(D, Dr, rtol=0, atol=max(1e-30, np.abs(Dr[np.isfinite(Dr)]).max() * 2 ** -22))


# ---------------------------------------------------------------------------------------------------------
# 2. source and destination in different code layouts
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dst_layout,src_layout", [("ivfpq_m96", 2, 0), ("ivfpq_m64g", 0, 1), ("ivfpq_m96r", 1, 2), ("ivfpq_m96g", 0, 2)])
def test_merge_across_code_layouts(gpu, kind, dst_layout, src_layout):
    full = _full(gpu, kind)      # (the kind's own layout is the destination's)
    assert KINDS[kind][4] == dst_layout
    q = _data(gpu, KINDS[kind][1])[1]
    parts = _parts(gpu, kind, layouts=[dst_layout, src_layout, src_layout, src_layout])
    assert parts[0]._get("pq_layout") == dst_layout and parts[3]._get("pq_layout") == src_layout
    _assert_same_index(_merge_all(kind, parts), full, q, f"{kind} {src_layout}->{dst_layout}")


# ---------------------------------------------------------------------------------------------------------
# 3. a reserved destination is not laid out again
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ivfflat_ip", "ivfpq_m96"])
def test_reserved_destination_needs_no_relayout(gpu, kind):
    full = _full(gpu, kind)
    q = _data(gpu, KINDS[kind][1])[1]
    # a destination holding a quarter of the rows: its lists' headroom (1.5 x for rows, 2 x + 64 for codes) cannot take the other three
    sizes = (3000, 1, 0, 8999)
    plain = _parts(gpu, kind, sizes=sizes)
    _merge_all(kind, plain)
    assert plain[0].get_timing("merge_relayouts") >= 1
    reserved = _parts(gpu, kind, sizes=sizes)
    reserved[0].reserve_lists(full[0].list_sizes())
    _merge_all(kind, reserved)
    assert reserved[0].get_timing("merge_relayouts") == 0
    _assert_same_index(reserved[0], full, q, f"{kind} reserved")
    _assert_same_index(plain[0], full, q, f"{kind} re-laid-out")


# ---------------------------------------------------------------------------------------------------------
# 4. fp16 and fp32 rows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat_l2", "ivfflat_ip"])
@pytest.mark.parametrize("f32_first", [False, True])
def test_merge_widens_rows(gpu, kind, f32_first):
    x, q = _data(gpu, KINDS[kind][1])
    half = N // 2
    x16 = x[:half] if not f32_first else x[half:]
    x32 = (x[half:] if not f32_first else x[:half]).astype(np.float32) * np.float32(1.0001)      # not fp16 values
    assert not np.array_equal(x32, x32.astype(np.float16).astype(np.float32))
    first, second = (x32, x16) if f32_first else (x16, x32)
    one = _new(gpu, kind)
    one.add(first)
    one.add(second)
    assert one.storage_dtype == "float32"
    dst, src = _new(gpu, kind), _new(gpu, kind)
    dst.add(first)
    src.add(second)
    assert dst.storage_dtype == ("float32" if f32_first else "float16") and src.storage_dtype == ("float16" if f32_first else "float32")
    dst.merge_from(src, dst.ntotal if _is_ivf(kind) else 0)
    assert dst.storage_dtype == "float32"
    _assert_same_index(dst, (one, _lists(one), _searches(one, q)), q, f"{kind} widening")
    # a later add keeps the certificate's maximum of both sides
    dst.add(x[:64]); one.add(x[:64])
    assert_same_results(*dst.search(q, 10), *one.search(q, 10), f"{kind} add after the widening merge")


# ---------------------------------------------------------------------------------------------------------
# 5. add_id
# ---------------------------------------------------------------------------------------------------------
def test_add_id_shifts_the_sources_ids(gpu):
    kind = "ivfflat_ip"
    parts = _parts(gpu, kind)
    dst, src = parts[0], parts[3]
    before_d, before_s = _lists(dst), _lists(src)
    dst.merge_from(src, 10 ** 12)
    _assert_lists_equal(_lists(dst), merge_ref.merged_lists(before_d, before_s, 10 ** 12), "add_id")
    assert dst._get("explicit_ids") == 1
    ids = np.concatenate([i for _, i in _lists(dst)])
    assert (ids >= 10 ** 12).sum() == PARTS[3] and (ids < PARTS[0]).sum() == PARTS[0]


@pytest.mark.parametrize("kind", ["flat_ip", "pq", "sq"])
def test_flat_codes_refuse_add_id(gpu, kind):
    q = _data(gpu, KINDS[kind][1])[1]
    dst, src = _new(gpu, kind), _new(gpu, kind)
    _add(dst, kind, 0, 300); _add(src, kind, 300, 700)
    rd, rs = dst.search(q, 10), src.search(q, 10)
    with pytest.raises(RuntimeError, match="cannot set ids in FlatCodes index"):
        dst.merge_from(src, 5)
    assert dst.ntotal == 300 and src.ntotal == 400
    assert_same_results(*dst.search(q, 10), *rd, kind); assert_same_results(*src.search(q, 10), *rs, kind)


def test_flat_id_modes(gpu):
    kind = "flat_ids"
    x, q = _data(gpu, KINDS[kind][1])
    seq, expl, empty = _new(gpu, kind), _new(gpu, kind), _new(gpu, kind)
    seq.add(x[:100])
    expl.add_with_ids(x[100:300], _flat_ids()[100:300])
    with pytest.raises(RuntimeError, match="explicit ids"):
        seq.merge_from(expl)
    with pytest.raises(RuntimeError, match="explicit ids"):
        expl.merge_from(seq)
    assert seq.ntotal == 100 and expl.ntotal == 200
    empty.merge_from(expl, 1000)      # an empty destination adopts the source's id mode
    payload, ids = empty.get_list(0)
    assert np.array_equal(ids, _flat_ids()[100:300] + 1000) and np.array_equal(payload, x[100:300].astype(np.float32))
    assert expl.ntotal == 0 and empty._get("explicit_ids") == 1


# ---------------------------------------------------------------------------------------------------------
# 6. copy_subset_to
# ---------------------------------------------------------------------------------------------------------
SUBSET_KINDS = ["ivfflat_l2", "ivfpq_m96", "ivfsq_res"]


@pytest.mark.parametrize("kind", SUBSET_KINDS)
def test_copy_subset_matches_the_rules(gpu, kind):
    src, src_lists, src_res = _full(gpu, kind)
    q = _data(gpu, KINDS[kind][1])[1]
    IL = gpu.InvertedLists
    for st, a1, a2 in ((IL.SUBSET_TYPE_ID_RANGE, 2500, 9001), (IL.SUBSET_TYPE_ID_MOD, 3, 1), (IL.SUBSET_TYPE_ELEMENT_RANGE, 4000, 9500),
                       (IL.SUBSET_TYPE_ID_RANGE, 0, N), (IL.SUBSET_TYPE_ELEMENT_RANGE, 0, 1)):
        dst = _new(gpu, kind)
        src.copy_subset_to(dst, st, a1, a2)
        want = merge_ref.subset_lists(src_lists, st, a1, a2)
        _assert_lists_equal(_lists(dst), want, f"{kind} subset type {st}")
        assert dst.ntotal == sum(len(i) for _, i in want)
        # behind the destination's own entries
        src.copy_subset_to(dst, IL.SUBSET_TYPE_ID_MOD, 5, 2)
        _assert_lists_equal(_lists(dst), merge_ref.merged_lists(want, merge_ref.subset_lists(src_lists, 1, 5, 2)), f"{kind} second subset")
    # the source is unchanged
    _assert_same_index(src, (src, src_lists, src_res), q, f"{kind} source after copy_subset_to")
    # an empty selection leaves the destination untouched
    dst = _new(gpu, kind)
    _add(dst, kind, 0, 500)
    before = _lists(dst)
    src.copy_subset_to(dst, IL.SUBSET_TYPE_ID_RANGE, N + 5, N + 9)
    src.copy_subset_to(dst, IL.SUBSET_TYPE_ELEMENT_RANGE, 77, 77)
    assert dst.ntotal == 500
    _assert_lists_equal(_lists(dst), before, f"{kind} empty selection")


@pytest.mark.parametrize("kind", SUBSET_KINDS)
def test_split_and_merge_back(gpu, kind):
    full = _full(gpu, kind)
    src, src_lists, src_res = full
    q = _data(gpu, KINDS[kind][1])[1]
    IL = gpu.InvertedLists
    # three consecutive element ranges, merged back in order: the original lists bit for bit
    cuts = [0, N // 3, 2 * N // 3, N]
    pieces = []
    for p in range(3):
        ix = _new(gpu, kind)
        src.copy_subset_to(ix, IL.SUBSET_TYPE_ELEMENT_RANGE, cuts[p], cuts[p + 1])
        assert ix.ntotal == cuts[p + 1] - cuts[p]
        pieces.append(ix)
    for p in (1, 2):
        pieces[0].merge_from(pieces[p], 0)
    _assert_same_index(pieces[0], full, q, f"{kind} element ranges merged back")
    # the three residues of id % 3, merged back: the same id sets per list and the same search results
    res = []
    for r in range(3):
        ix = _new(gpu, kind)
        src.copy_subset_to(ix, IL.SUBSET_TYPE_ID_MOD, 3, r)
        res.append(ix)
    assert sum(ix.ntotal for ix in res) == N
    for r in (1, 2):
        res[0].merge_from(res[r], 0)
    assert res[0].ntotal == N
    for (pg, ig), (pw, iw) in zip(_lists(res[0]), src_lists):
        og, ow = np.argsort(ig, kind="stable"), np.argsort(iw, kind="stable")
        assert np.array_equal(ig[og], iw[ow]) and np.array_equal(pg[og], pw[ow])
    got = _searches(res[0], q)
    for key in src_res:
        assert_same_results(got[key][0], got[key][1], src_res[key][0], src_res[key][1], f"{kind} residues merged back, search {key}")


# ---------------------------------------------------------------------------------------------------------
# 7. derived state of before the merge is not served afterwards
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ivfpq_m96", "ivfflat_l2"])
def test_stale_state_is_dropped(gpu, kind):
    full = _full(gpu, kind)
    fx = full[0]
    q = _data(gpu, KINDS[kind][1])[1]
    sel = gpu.IDSelectorRange(1000, 9000)
    params = gpu.SearchParametersIVF(sel=sel, nprobe=NPROBE)
    parts = _parts(gpu, kind)
    dst = parts[0]
    dst.search(q, 10, params=params)      # the selector's slot mask, cached per directory generation
    dst.search(q, 300)                    # sliced layout: builds the row-major copy of the codes
    keys = np.array([0, 4999, 5000, 5001, N - 1, 7], dtype=np.int64)
    dst.reconstruct_batch(keys[[0, 1, 5]])       # the direct map
    _merge_all(kind, parts)
    assert_same_results(*dst.search(q, 10, params=params), *fx.search(q, 10, params=params), f"{kind} filtered search after the merge")
    assert_same_results(*dst.search(q, 300), *fx.search(q, 300), f"{kind} k = 300 after the merge")
    assert np.array_equal(dst.reconstruct_batch(keys), fx.reconstruct_batch(keys))
    _assert_same_index(dst, full, q, f"{kind} after stale-state searches")


@pytest.mark.parametrize("kind", ["ivfpq_m64", "ivfflat_ip", "flat_ids"])
def test_remove_then_merge(gpu, kind):
    x, q = _data(gpu, KINDS[kind][1])
    a, b = 5000, 9000
    rm = _flat_ids()[100:1700] if kind == "flat_ids" else np.arange(100, 1700, dtype=np.int64)
    one = _new(gpu, kind)
    _add(one, kind, 0, a)
    assert one.remove_ids(rm) == 1600
    if kind == "flat_ids":
        one.add_with_ids(x[a:b], _flat_ids()[a:b])
    else:
        one.add_with_ids(x[a:b], np.arange(a, b, dtype=np.int64))
    dst, src = _new(gpu, kind), _new(gpu, kind)
    _add(dst, kind, 0, a)
    _add(src, kind, a, b)
    assert dst.remove_ids(rm) == 1600
    dst.merge_from(src, a if _is_ivf(kind) else 0)
    _assert_same_index(dst, (one, _lists(one), _searches(one, q)), q, f"{kind} remove then merge")


# ---------------------------------------------------------------------------------------------------------
# 8. files
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MERGE_KINDS)
def test_merged_index_survives_a_file(gpu, kind, tmp_path, monkeypatch):
    full = _full(gpu, kind)
    q = _data(gpu, KINDS[kind][1])[1]
    dst = _merge_all(kind, _parts(gpu, kind))
    # (no FAISS-format writer: IVF-SQ, IndexScalarQuantizer, Flat with explicit ids)
    formats = ["rsx1"] + (["faiss"] if KINDS[kind][0] in ("flat", "ivfflat", "ivfpq", "pq") and kind != "flat_ids" else [])
    for fmt in formats:
        if fmt == "faiss":
            monkeypatch.setenv("RSX_INDEX_FORMAT", "faiss")
        path = str(tmp_path / f"{kind}.{fmt}")
        gpu.write_index(dst, path)
        back = gpu.read_index(path, device=0)
        if _is_ivf(kind):
            back.nprobe = NPROBE
        assert back.ntotal == N
        for k in (10, 100):
            assert_same_results(*back.search(q, k), *full[2][k], f"{kind} {fmt} k={k}")


# ---------------------------------------------------------------------------------------------------------
# 9. refusals leave both handles untouched
# ---------------------------------------------------------------------------------------------------------
def _pair_state(gpu, ix, q):
    return (ix.ntotal, ix.list_sizes().copy(), ix.search(q, 10)) if ix.ntotal or ix.is_trained else (ix.ntotal, None, None)


def _refused(gpu, call, dst, src, qd, qs, match):
    sd = _pair_state(gpu, dst, qd) if not dst.nshards else None
    ss = _pair_state(gpu, src, qs) if not src.nshards else None
    with pytest.raises(RuntimeError, match=match):
        call()
    for ix, st, q in ((dst, sd, qd), (src, ss, qs)):
        if st is None:
            continue
        assert ix.ntotal == st[0]
        if st[1] is not None:
            assert np.array_equal(ix.list_sizes(), st[1])
            assert_same_results(*ix.search(q, 10), *st[2], "after a refused call")


def test_refusals_leave_both_handles_untouched(gpu):
    kind = "ivfflat_ip"
    x, q = _data(gpu, 96)
    IL = gpu.InvertedLists

    def filled(k=kind, lo=0, hi=600, **kw):
        ix = _new(gpu, k, **kw)
        _add(ix, k, lo, hi)
        return ix
    dst, src = filled(), filled(lo=600, hi=1500)
    cen = dst.get_centroids()

    def other(d=96, nlist=32, metric=0, cent=None, train=True):
        ix = gpu.IndexIVFFlat(None, d, nlist, metric, device=0)
        if train:
            c = np.zeros((nlist, d), np.float32)
            c[:min(nlist, 32), :min(d, 96)] = cen[:min(nlist, 32), :min(d, 96)]
            ix.set_centroids(c if cent is None else cent)
            ix.nprobe = NPROBE
            xx = np.zeros((200, d), np.float16)
            xx[:, :min(d, 96)] = x[:200, :min(d, 96)]
            ix.add(xx)
        return ix, (np.zeros((NQ, d), np.float16) + q[:, :1] if d != 96 else q)

    for what, (o, qo), match in (("d", other(d=128), "differ in d"), ("nlist", other(nlist=16), "differ in nlist"),
                                 ("metric", other(metric=1), "differ in metric")):
        _refused(gpu, lambda: dst.merge_from(o), dst, o, q, qo, match)
        _refused(gpu, lambda: o.merge_from(src), o, src, qo, q, match)
        _refused(gpu, lambda: src.copy_subset_to(o, 0, 0, 10), o, src, qo, q, match)
    # another kind
    fl = filled("flat_ip")
    _refused(gpu, lambda: dst.merge_from(fl), dst, fl, q, q, "differ in kind")
    _refused(gpu, lambda: fl.merge_from(src), fl, src, q, q, "differ in kind")
    # M
    x256, q256 = _data(gpu, 256)
    p32 = filled("ivfpq_m32_l2")
    p16 = gpu.IndexIVFPQ(None, 256, 8, 16, 8, 1, device=0)
    p16.train(x256[:3000]); p16.add(x256[:300]); p16.nprobe = NPROBE
    _refused(gpu, lambda: p32.merge_from(p16), p32, p16, q256, q256, "differ in M")
    # centroids differing in one bit
    c1 = cen.copy()
    c1.view(np.uint32)[17, 5] ^= 1
    o, _ = other(cent=c1)
    _refused(gpu, lambda: dst.merge_from(o), dst, o, q, q, "centroids differ")
    _refused(gpu, lambda: o.copy_subset_to(dst, 1, 2, 0), dst, o, q, q, "centroids differ")
    # an untrained side
    un, _ = other(train=False)
    _refused(gpu, lambda: dst.merge_from(un), dst, un, q, q, "trained")
    _refused(gpu, lambda: un.merge_from(src), un, src, q, q, "trained")
    # the same handle
    _refused(gpu, lambda: dst.merge_from(dst), dst, dst, q, q, "same handle")
    _refused(gpu, lambda: dst.copy_subset_to(dst, 0, 0, 5), dst, dst, q, q, "same handle")
    # a sharded handle on either side
    sh = filled(devices=[0, 0])
    _refused(gpu, lambda: dst.merge_from(sh), dst, sh, q, q, "sharded")
    _refused(gpu, lambda: sh.merge_from(src), sh, src, q, q, "sharded")
    _refused(gpu, lambda: sh.copy_subset_to(dst, 0, 0, 5), dst, sh, q, q, "sharded")
    # a list shard
    ls = _new(gpu, kind)
    ls.set_param("add_list_mod", 2)
    _add(ls, kind, 0, 600)
    _refused(gpu, lambda: dst.merge_from(ls), dst, ls, q, q, "list shard")
    _refused(gpu, lambda: ls.merge_from(src), ls, src, q, q, "list shard")
    # subset types 3 / 4, bad a1 / a2
    _refused(gpu, lambda: src.copy_subset_to(dst, IL.SUBSET_TYPE_INVLIST_FRACTION, 0, 1), dst, src, q, q, "subset type 3")
    _refused(gpu, lambda: src.copy_subset_to(dst, IL.SUBSET_TYPE_INVLIST, 0, 1), dst, src, q, q, "subset type 4")
    _refused(gpu, lambda: src.copy_subset_to(dst, 7, 0, 1), dst, src, q, q, "subset type 7")
    _refused(gpu, lambda: src.copy_subset_to(dst, IL.SUBSET_TYPE_ID_RANGE, 9, 3), dst, src, q, q, "a1 <= a2")
    _refused(gpu, lambda: src.copy_subset_to(dst, IL.SUBSET_TYPE_ID_MOD, 0, 0), dst, src, q, q, "a1 > 0")
    _refused(gpu, lambda: src.copy_subset_to(dst, IL.SUBSET_TYPE_ID_MOD, 3, 3), dst, src, q, q, "a2 < a1")
    _refused(gpu, lambda: src.copy_subset_to(dst, IL.SUBSET_TYPE_ELEMENT_RANGE, 0, src.ntotal + 1), dst, src, q, q, "ntotal")
    # copy_subset_to on a Flat kind
    f2 = filled("flat_ip", lo=600, hi=900)
    with pytest.raises(AttributeError):
        fl.copy_subset_to(f2, 0, 0, 5)
    assert gpu.lib().rsx_copy_subset_to(fl._h, f2._h, 0, 0, 5) != 0 and "IVF indexes only" in gpu.lib().rsx_last_error().decode()
    assert fl.ntotal == 600 and f2.ntotal == 300
    # an open two-call search
    import torch
    qt = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    ref = dst.search(q, 10)
    dst.search_prepass(qt, 10)
    try:
        with pytest.raises(RuntimeError, match="two-call search"):
            dst.merge_from(src)
        with pytest.raises(RuntimeError, match="two-call search"):
            src.merge_from(dst)
        with pytest.raises(RuntimeError, match="two-call search"):
            src.copy_subset_to(dst, 0, 0, 5)
    finally:
        D, I = dst.search_scan()
    assert_same_results(D.cpu().numpy(), I.cpu().numpy(), *ref, "the two-call search finishes as if nothing had been asked")
    assert dst.ntotal == 600 and src.ntotal == 900
    # after all the refusals the pair still merges
    dst.merge_from(src, 600)
    assert dst.ntotal == 1500 and src.ntotal == 0


def test_pretransform_merge(gpu):
    import rsx_vt
    d = 96
    x, q = _data(gpu, d)
    q = q.astype(np.float32)

    def make(seed):
        rr = rsx_vt.RandomRotationMatrix(d, d, device=0)
        rr.init(seed)
        ix = rsx_vt.IndexPreTransform(rr, _new(gpu, "ivfflat_ip"))
        return ix
    one, a, b, c = make(5), make(5), make(5), make(6)
    xf = x.astype(np.float32)
    one.add(xf[:3000])
    a.add(xf[:1000]); b.add(xf[1000:3000]); c.add(xf[1000:3000])
    ra, rc = a.search(q, 10), c.search(q, 10)
    with pytest.raises(RuntimeError, match="chains differ|transform 0"):
        a.merge_from(c, 1000)
    assert a.ntotal == 1000 and c.ntotal == 2000
    assert_same_results(*a.search(q, 10), *ra, "after a refused call"); assert_same_results(*c.search(q, 10), *rc, "after a refused call")
    with pytest.raises(RuntimeError, match="IndexPreTransform"):
        a.merge_from(a.index)
    a.merge_from(b, 1000)
    assert a.ntotal == 3000 and b.ntotal == 0
    assert_same_results(*a.search(q, 10), *one.search(q, 10), "IndexPreTransform merge")


def test_refine_flat_refuses_merge(gpu):
    base = _new(gpu, "ivfflat_ip")
    ix = gpu.IndexRefineFlat(base)
    with pytest.raises(RuntimeError, match="IndexRefineFlat"):
        ix.merge_from(gpu.IndexRefineFlat(_new(gpu, "ivfflat_ip")))
