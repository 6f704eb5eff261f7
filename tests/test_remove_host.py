"""CPU: remove_ids host layers — the FAISS 1.8.0 removal loops restated literally, checked against the closed form the device plan
(k_remove.hip) computes; the ABI version and argument checks (no GPU needed); the array -> IDSelectorBatch conversion."""
import ctypes

import numpy as np
import pytest


def faiss_ivf_list_remove(ids, removed):
    """DirectMap::remove_ids, NoMap branch, one list: the literal loop.  -> kept positions in their new order."""
    entry = list(range(len(ids)))
    j, l = 0, len(ids)
    while j < l:
        if removed[ids[entry[j]]]:
            l -= 1
            entry[j] = entry[l]
        else:
            j += 1
    return entry[:l]


def faiss_flat_remove(n, removed):
    """IndexFlatCodes::remove_ids / IndexIDMap::remove_ids: stable compaction.  -> kept positions in order."""
    j = 0
    out = list(range(n))
    for i in range(n):
        if not removed[i]:
            out[j] = out[i]
            j += 1
    return out[:j]


def closed_form_ivf(removed_pos):
    """The device plan: kept entries below the new length stay; the holes below it, ascending, take the kept entries at or above
    it, descending position order."""
    L = len(removed_pos)
    nl = L - int(removed_pos.sum())
    holes = [j for j in range(nl) if removed_pos[j]]
    tail = [p for p in range(L - 1, nl - 1, -1) if not removed_pos[p]]
    assert len(holes) == len(tail)
    out = list(range(nl))
    for h, p in zip(holes, tail):
        out[h] = p
    return out


def _cases():
    rng = np.random.default_rng(11)
    yield np.zeros(0, bool)
    for L in (1, 2, 3, 31, 32, 33, 64, 100, 257, 1000):
        yield np.zeros(L, bool)                       # none removed
        yield np.ones(L, bool)                        # all removed
        t = np.zeros(L, bool); t[L - max(1, L // 3):] = True
        yield t                                       # tail only
        h = np.zeros(L, bool); h[:max(1, L // 3)] = True
        yield h                                       # head only
        for p in (0.01, 0.1, 0.5, 0.9):
            yield rng.random(L) < p


def test_ivf_closed_form_matches_faiss_loop():
    for removed_pos in _cases():
        ids = np.arange(len(removed_pos))          # ids = positions: the selector's answer per entry
        want = faiss_ivf_list_remove(ids, removed_pos)
        got = closed_form_ivf(removed_pos)
        assert got == want, removed_pos.astype(int).tolist()


def test_ivf_loop_with_arbitrary_ids():
    rng = np.random.default_rng(2)
    for _ in range(50):
        L = int(rng.integers(0, 300))
        ids = rng.permutation(10 * L + 1)[:L]
        sel = set(rng.choice(10 * L + 1, size=int(rng.integers(0, 2 * L + 1)), replace=True).tolist())
        removed_id = np.zeros(10 * L + 1, bool)
        removed_id[list(sel)] = True
        want = [ids[p] for p in faiss_ivf_list_remove(ids, removed_id)]
        got = [ids[p] for p in closed_form_ivf(removed_id[ids])]
        assert got == want


def test_flat_compaction_is_stable():
    for removed_pos in _cases():
        n = len(removed_pos)
        assert faiss_flat_remove(n, removed_pos) == [i for i in range(n) if not removed_pos[i]]


def test_abi_version_has_remove_ids(rsxlib):
    assert rsxlib.lib().rsx_version() >= 1002


def test_null_arguments_are_invalid_without_gpu(rsxlib):
    L = rsxlib.lib()
    sel = rsxlib.IDSelectorRange(0, 10)
    n = ctypes.c_int64(-7)
    assert L.rsx_remove_ids(None, sel._native(), ctypes.byref(n)) == -1
    assert L.rsx_remove_ids(None, None, ctypes.byref(n)) == -1
    assert L.rsx_remove_ids(None, sel._native(), None) == -1
    assert "null" in L.rsx_last_error().decode()


def test_array_becomes_id_selector_batch(rsxlib):
    from rsx import _remove_selector
    ids = np.array([5, 5, 9, -1, 1 << 40, 5], dtype=np.int64)
    s = _remove_selector(ids)
    assert isinstance(s, rsxlib.IDSelectorBatch)
    probe = np.arange(-3, 20)
    assert np.array_equal(s.is_member(probe), np.isin(probe, ids))
    s32 = _remove_selector(np.array([3, 3, 4], dtype=np.int32))     # any integer dtype, duplicates allowed
    assert s32.ids.dtype == np.int64 and s32.is_member([3, 4, 5]).tolist() == [True, True, False]
    assert _remove_selector([]).ids.size == 0
    r = rsxlib.IDSelectorRange(1, 2)
    assert _remove_selector(r) is r
    with pytest.raises(ValueError):
        _remove_selector(np.zeros((2, 3), np.int64))
    with pytest.raises(TypeError):
        _remove_selector(np.array([1.5, 2.0]))
