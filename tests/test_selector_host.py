"""CPU: filtered-search host layers — the id selectors (rsx_selector_create / rsx_selector_is_member need no GPU) against a
numpy membership reference, the FAISS 1.8.0 parameter rules, the global -> local translation of id-range shards, and the
mirror's params pass-through and datastore_subsample_p key (test-double engine)."""
import json
import os

import numpy as np
import pytest


def _bitmap_ref(bm, ids):
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < 8 * bm.size)
    out = np.zeros(ids.shape, bool)
    j = ids[ok]
    out[ok] = (bm[j >> 3] >> (j & 7)) & 1 == 1
    return out


def test_abi_version_has_filtered_search(rsxlib):
    assert rsxlib.lib().rsx_version() >= 1001


def test_range_bounds(rsxlib):
    ids = np.arange(-5, 40, dtype=np.int64)
    for lo, hi in [(0, 10), (3, 4), (7, 7), (9, 2), (-3, 5), (30, 1 << 62)]:
        s = rsxlib.IDSelectorRange(lo, hi)
        assert np.array_equal(s.is_member(ids), (ids >= lo) & (ids < hi)), (lo, hi)
        assert np.array_equal(rsxlib.IDSelectorNot(s).is_member(ids), ~((ids >= lo) & (ids < hi)))
    assert not rsxlib.IDSelectorRange(0, 10).is_member([10])[0] and rsxlib.IDSelectorRange(0, 10).is_member([0])[0]


def test_batch_duplicates_and_absent_ids(rsxlib):
    rng = np.random.default_rng(5)
    batch = np.concatenate([rng.integers(0, 1000, 300), [7, 7, 7, -4, 1 << 40]])
    s = rsxlib.IDSelectorBatch(batch)
    ids = np.arange(-10, 1100, dtype=np.int64)
    want = np.isin(ids, batch)
    assert np.array_equal(s.is_member(ids), want)
    assert s.is_member([1 << 40])[0]
    assert np.array_equal(rsxlib.IDSelectorNot(s).is_member(ids), ~want)
    assert np.array_equal(rsxlib.IDSelectorNot(rsxlib.IDSelectorNot(s)).is_member(ids), want)
    # the (n, ids) form takes the first n
    assert np.array_equal(rsxlib.IDSelectorBatch(3, np.array([1, 2, 3, 4])).is_member([1, 2, 3, 4]), [True, True, True, False])
    assert not rsxlib.IDSelectorBatch(np.zeros(0, np.int64)).is_member(np.arange(5)).any()


def test_bitmap_bit_order(rsxlib):
    bm = np.array([0b00000001, 0b10000000, 0b00100100], np.uint8)
    s = rsxlib.IDSelectorBitmap(bm)
    # least significant bit first: id 0 <- byte 0 bit 0, id 15 <- byte 1 bit 7, ids 18 / 21 <- byte 2 bits 2 / 5
    assert list(np.nonzero(s.is_member(np.arange(-3, 40)))[0] - 3) == [0, 15, 18, 21]
    rng = np.random.default_rng(1)
    bm = rng.integers(0, 256, 97).astype(np.uint8)
    ids = np.arange(-20, 8 * 97 + 50, dtype=np.int64)
    assert np.array_equal(rsxlib.IDSelectorBitmap(bm).is_member(ids), _bitmap_ref(bm, ids))
    assert np.array_equal(rsxlib.IDSelectorNot(rsxlib.IDSelectorBitmap(bm)).is_member(ids), ~_bitmap_ref(bm, ids))
    with pytest.raises(TypeError):
        rsxlib.IDSelectorBitmap(np.zeros(4, np.int32))


def test_selector_create_rejects_bad_arguments(rsxlib):
    import ctypes
    h = ctypes.c_void_p()
    L = rsxlib.lib()
    assert L.rsx_selector_create(7, None, ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), 0, ctypes.byref(h)) != 0
    assert "selector kind" in L.rsx_last_error().decode()
    assert L.rsx_selector_create(1, None, ctypes.c_int64(4), ctypes.c_int64(0), ctypes.c_int64(0), 0, ctypes.byref(h)) != 0


def test_params_type_rules(rsxlib):
    sel = rsxlib.IDSelectorRange(0, 10)
    # IndexIVF::search: a params object that is not SearchParametersIVF is refused (FAISS 1.8.0)
    with pytest.raises(RuntimeError, match="IndexIVF params have incorrect type"):
        rsxlib._resolve_params(rsxlib.SearchParameters(sel=sel), True)
    with pytest.raises(TypeError):
        rsxlib._resolve_params({"sel": sel}, False)
    with pytest.raises(TypeError):
        rsxlib._resolve_params(rsxlib.SearchParameters(sel=np.arange(3)), False)
    # max_codes / quantizer_params are refused, never ignored
    with pytest.raises(NotImplementedError, match="max_codes"):
        rsxlib._resolve_params(rsxlib.SearchParametersIVF(sel=sel, nprobe=4, max_codes=100), True)
    with pytest.raises(NotImplementedError, match="max_codes"):
        rsxlib._resolve_params(rsxlib.SearchParametersIVF(sel=sel, max_codes=100), False)
    with pytest.raises(ValueError):
        rsxlib._resolve_params(rsxlib.SearchParametersIVF(sel=sel, nprobe=0), True)
    # SearchParametersIVF.nprobe defaults to 1 (FAISS 1.8.0) and is the override; Flat takes either class and has no nprobe
    p = rsxlib.SearchParametersIVF(sel=sel)
    assert p.nprobe == 1 and p.max_codes == 0
    h, nprobe, _ = rsxlib._resolve_params(p, True)
    assert h is not None and nprobe == 1
    assert rsxlib._resolve_params(rsxlib.SearchParametersIVF(nprobe=7), True)[:2] == (None, 7)
    assert rsxlib._resolve_params(rsxlib.SearchParametersIVF(sel=sel, nprobe=7), False)[1] == 0
    assert rsxlib._resolve_params(rsxlib.SearchParameters(), False)[:2] == (None, 0)


@pytest.mark.parametrize("offset", [0, 8, 13, 1000])
def test_id_range_shard_translation(rsxlib, offset):
    """An id-range shard stores local ids [0, n_local) for the global ids [offset, offset + n_local): the shifted selector
    selects local id i exactly when the global selector selects i + offset."""
    import sharded
    rng = np.random.default_rng(offset)
    n_local = 700
    bm = rng.integers(0, 256, 300).astype(np.uint8)
    batch = rng.integers(0, 2500, 400)
    sels = [rsxlib.IDSelectorRange(offset + 50, offset + 400), rsxlib.IDSelectorRange(0, 20), rsxlib.IDSelectorBatch(batch),
            rsxlib.IDSelectorBitmap(bm), rsxlib.IDSelectorNot(rsxlib.IDSelectorRange(offset + 10, offset + 600)),
            rsxlib.IDSelectorNot(rsxlib.IDSelectorBitmap(bm)), rsxlib.IDSelectorNot(rsxlib.IDSelectorBatch(batch))]
    local = np.arange(n_local, dtype=np.int64)

    class _Local:
        ntotal = n_local

    srch = sharded.ShardedSearcher.__new__(sharded.ShardedSearcher)
    srch.index, srch.id_offset = _Local(), offset
    for s in sels:
        want = s.is_member(local + offset)
        assert np.array_equal(s.shifted(offset, n_local).is_member(local), want), type(s).__name__
        lp = srch.local_params(rsxlib.SearchParametersIVF(sel=s, nprobe=3))
        assert lp.nprobe == 3 and np.array_equal(lp.sel.is_member(local), want)
    p = rsxlib.SearchParameters()
    assert srch.local_params(p) is p and srch.local_params(None) is None


# ---------------- mirror (src/): params pass-through and the datastore_subsample_p key ----------------

_CALLS = []


def _flat_ip_sel():
    """the test-double engine's Flat index, with a search that takes params (filter = search of the selected rows); defined at
    module level so that the engine's write_index can pickle it"""
    import fake_engine
    from oracle import oracle as o

    global FlatIPSel

    class FlatIPSel(fake_engine.IndexFlatIP):
        def search(self, q, k, params=None):
            _CALLS.append(params)
            if params is None:
                return super().search(q, k)
            keep = np.nonzero(params.sel.is_member(np.arange(self.ntotal)))[0]
            D, I = o.flat_search(np.asarray(q, np.float32), self.x[keep], k, 0)
            return D, np.where(I >= 0, keep[np.maximum(I, 0)], -1)
    FlatIPSel.__qualname__ = "FlatIPSel"
    return FlatIPSel


@pytest.fixture()
def fake_sel(monkeypatch, orc):
    import fake_engine
    import rsx
    for name in ("IndexIVFFlat", "IndexIVFPQ", "read_index", "write_index"):
        monkeypatch.setattr(rsx, name, getattr(fake_engine, name))
    monkeypatch.setattr(rsx, "IndexFlatIP", _flat_ip_sel())
    _CALLS.clear()
    return _CALLS


def test_indexer_passes_params_through(tmp_path, orc, fake_sel):
    from test_host_logic import make_cfg, write_datastore
    import rsx
    from src.indicies.base import Indexer
    embs = write_datastore(str(tmp_path), orc)
    ix = Indexer(make_cfg(str(tmp_path), "Flat", [0]))
    q = embs[0][3:5]
    s0, p0, d0 = ix.search(q, 4)
    assert fake_sel[-1] is None                       # default: the reference's call
    params = rsx.SearchParameters(sel=rsx.IDSelectorRange(100, 200))
    s1, p1, d1 = ix.search(q, 4, params=params)
    assert fake_sel[-1] is params
    for row in d1:
        assert all(db[0] == 0 and 100 <= db[1] < 200 for db in row)
    keep = np.arange(100, 200)
    D, I = orc.flat_search(q.astype(np.float32), embs[0][keep].astype(np.float32), 4, 0)
    assert [[db[1] for db in row] for row in d1] == (keep[I]).tolist()


def test_datastore_subsample_key(tmp_path, orc, fake_sel):
    from test_host_logic import NS, make_cfg, write_datastore
    import src.search as S
    tmp = str(tmp_path)
    embs = write_datastore(tmp, orc)
    data = [{"raw_query": "a"}, {"raw_query": "b"}]
    q = np.concatenate([embs[0][1:2], embs[0][2:3]], 0)
    # absent key / p >= 1: no params, the reference's call
    assert S.datastore_subsample_params(NS(n_docs=3), None) is None
    assert S.datastore_subsample_params(NS(n_docs=3, datastore_subsample_p=1.0), None) is None
    cfg = make_cfg(tmp, "Flat", [0])
    cfg.evaluation.search.datastore_subsample_p = 0.25
    S.search_dense_topk(cfg, data=data, questions_embedding=q)
    params = fake_sel[-1]
    assert params is not None and params.sel is not None
    keep = np.random.default_rng(1000).random(400) < 0.25           # subsample_seed defaults to 1000
    assert np.array_equal(params.sel.is_member(np.arange(400)), keep)
    rows = [json.loads(l) for l in open(S.get_search_output_path(cfg, [0]))]
    kept = np.nonzero(keep)[0]
    D, I = orc.flat_search(q.astype(np.float32), embs[0][kept].astype(np.float32), 3, 0)
    for qi, row in enumerate(rows):
        assert len(row["ctxs"]) == 3                                  # a full n_docs from the smaller datastore
        assert [c["id"] for c in row["ctxs"]] == [[0, int(kept[i])] for i in I[qi]]
    # IVF indexes keep their own nprobe (SearchParametersIVF alone would default to 1); the seed is honoured

    class _IVF:
        ntotal, nprobe = 50, 6
    import rsx
    p3 = S.datastore_subsample_params(NS(datastore_subsample_p=0.5), _IVF())
    assert isinstance(p3, rsx.SearchParametersIVF) and p3.nprobe == 6
    p4 = S.datastore_subsample_params(NS(datastore_subsample_p=0.5, subsample_seed=7), _IVF())
    assert np.array_equal(p4.sel.is_member(np.arange(50)), np.random.default_rng(7).random(50) < 0.5)
    with pytest.raises(ValueError):
        S.datastore_subsample_params(NS(datastore_subsample_p=-0.5), _IVF())
