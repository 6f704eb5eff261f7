"""CPU: merge_from / copy_subset_to without a device — the ABI, the constants, FAISS's running split of SUBSET_TYPE_ELEMENT_RANGE
(merge_ref.element_ranges, the literal loop) and the refusals that need no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import merge_ref
from conftest import PKG, REPO


def test_abi_has_merge_and_subset(rsxlib):
    L = rsxlib.lib()
    assert L.rsx_version() >= 1010
    header = open(os.path.join(REPO, "include", "rsx.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "csrc", "librsx.so")], text=True)
    for sym in ("rsx_merge_from", "rsx_copy_subset_to"):
        assert re.search(rf"\b{sym}\s*\(", header)
        assert sym in rsxlib.ABI_SYMBOLS
        assert re.search(rf" T {sym}\b", out)
        assert getattr(L, sym) is not None
    for faiss_call in ("IndexIVF::merge_from", "IndexFlatCodes::merge_from", "copy_subset_to"):
        assert faiss_call in header


def test_null_handles_are_invalid_without_gpu(rsxlib):
    L = rsxlib.lib()
    assert L.rsx_merge_from(None, None, 0) == -1
    assert "null" in L.rsx_last_error().decode()
    assert L.rsx_copy_subset_to(None, None, 0, 0, 0) == -1


def test_subset_type_constants(rsxlib):
    IL = rsxlib.InvertedLists
    assert (IL.SUBSET_TYPE_ID_RANGE, IL.SUBSET_TYPE_ID_MOD, IL.SUBSET_TYPE_ELEMENT_RANGE, IL.SUBSET_TYPE_INVLIST_FRACTION,
            IL.SUBSET_TYPE_INVLIST) == (0, 1, 2, 3, 4)
    assert (merge_ref.SUBSET_TYPE_ID_RANGE, merge_ref.SUBSET_TYPE_ID_MOD, merge_ref.SUBSET_TYPE_ELEMENT_RANGE) == (0, 1, 2)
    header = open(os.path.join(REPO, "include", "rsx.h")).read()
    for name, v in (("ID_RANGE", 0), ("ID_MOD", 1), ("ELEMENT_RANGE", 2), ("INVLIST_FRACTION", 3), ("INVLIST", 4)):
        assert re.search(rf"RSX_SUBSET_TYPE_{name} = {v}\b", header)


def test_element_ranges_partition_every_list():
    """FAISS's running split gives list l the positions [i(a1), i(a2)) with i(c) = floor(B c / nt) - floor(A c / nt), A and B = the
    entries before and up to the list (B - A = n).  For cuts c < c' this is a range, and consecutive ranges tile the list, when i is
    monotone in c: i(c') - i(c) > n (c' - c) / nt - 2, so it is whenever every non-empty list's share n (c' - c) / nt of a piece
    is at least two entries.  The sizes below keep to that (asserted, not skipped); the case below this one pins what the literal
    loop does beneath it."""
    rng = np.random.default_rng(5)
    ncases = 0
    for trial in range(80):
        nlist = int(rng.integers(1, 12))
        sizes = rng.integers(24, 300, nlist)
        sizes[rng.random(nlist) < 0.3] = 0                 # empty lists
        if trial % 9 == 0:
            sizes[:] = 0
            sizes[int(rng.integers(0, nlist))] = int(rng.integers(24, 300))      # all but one list empty
        nt = int(sizes.sum())
        if nt == 0:
            continue
        for pieces in (1, 2, 3, 7, 8):                     # ntotal is not divisible by most of them
            cuts = [nt * p // pieces for p in range(pieces + 1)]
            dmin = min(cuts[p + 1] - cuts[p] for p in range(pieces))
            assert all(int(n) * dmin >= 2 * nt for n in sizes if n), "the test's own sizes left the domain of the property"
            ncases += 1
            per_piece = [merge_ref.element_ranges(sizes, cuts[p], cuts[p + 1]) for p in range(pieces)]
            for l in range(nlist):
                at = 0
                for p in range(pieces):                    # consecutive ranges tile [0, n) of the list in order
                    i1, i2 = per_piece[p][l]
                    assert i1 == at and i2 >= i1
                    at = i2
                assert at == sizes[l]
            totals = [sum(i2 - i1 for i1, i2 in pp) for pp in per_piece]
            assert totals == [cuts[p + 1] - cuts[p] for p in range(pieces)] and sum(totals) == nt
            # after every list boundary a piece holds its share of the entries seen so far to within one
            for p in range(pieces):
                seen = got = 0
                for l in range(nlist):
                    seen += int(sizes[l])
                    got += per_piece[p][l][1] - per_piece[p][l][0]
                    assert abs(got - seen * (cuts[p + 1] - cuts[p]) / nt) <= 1.0
    assert ncases >= 300


def test_element_range_below_two_entries_per_list_is_the_literal_loop():
    """A list whose share of a range is below two entries can get i1 > i2 from the running split: FAISS's `for (i = i1; i < i2; i++)`
    then copies nothing from it, and its neighbours' ranges overlap by that entry.  The reference keeps the literal loop."""
    assert merge_ref.element_ranges([13, 3, 13], 4, 9) == [(1, 4), (1, 0), (2, 5)]
    lists = [(np.arange(n)[:, None], np.arange(n, dtype=np.int64)) for n in (13, 3, 13)]
    assert [len(p) for p in merge_ref.subset_positions(lists, 2, 4, 9)] == [3, 0, 3]


def test_subset_rules_on_small_lists():
    ids = np.array([7, -3, 12, 5, 9, 0, 30], dtype=np.int64)
    lists = [(np.arange(7)[:, None], ids), (np.zeros((0, 1), np.int64), np.zeros(0, np.int64))]
    assert merge_ref.subset_positions(lists, 0, 5, 12)[0].tolist() == [0, 3, 4]
    assert merge_ref.subset_positions(lists, 1, 3, 0)[0].tolist() == [1, 2, 4, 5, 6]      # C++: -3 % 3 == 0
    assert merge_ref.subset_positions(lists, 1, 3, 1)[0].tolist() == [0]
    assert merge_ref.subset_positions(lists, 2, 2, 5)[0].tolist() == [2, 3, 4]
    m = merge_ref.merged_lists(lists, lists, add_id=100)
    assert m[0][1].tolist() == ids.tolist() + (ids + 100).tolist() and len(m[1][1]) == 0


def test_refine_flat_refuses_merge_without_a_device(rsxlib):
    ix = rsxlib.IndexRefineFlat.__new__(rsxlib.IndexRefineFlat)
    with pytest.raises(RuntimeError, match="IndexRefineFlat"):
        ix.merge_from(ix)
