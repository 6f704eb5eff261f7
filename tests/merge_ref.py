"""The rules of merge_from / copy_subset_to (FAISS 1.8.0: IndexIVF::merge_from, InvertedLists::copy_subset_to) stated in numpy.
A list is a pair (payload [n, ...], ids int64 [n])."""
import numpy as np

SUBSET_TYPE_ID_RANGE, SUBSET_TYPE_ID_MOD, SUBSET_TYPE_ELEMENT_RANGE = 0, 1, 2


def merged_lists(dst, src, add_id=0):
    """per list: dst's entries, then src's in src's own order with ids + add_id"""
    out = []
    for (pd, idd), (ps, ids_) in zip(dst, src):
        if len(ids_) == 0:
            out.append((pd, idd))
        elif len(idd) == 0:
            out.append((ps, ids_ + add_id))
        else:
            out.append((np.concatenate([pd, ps.astype(pd.dtype)]), np.concatenate([idd, ids_ + add_id])))
    return out


def c_mod(ids, a1):
    """C++ remainder (sign of the dividend), as FAISS's `id % a1` computes it"""
    ids = np.asarray(ids, dtype=np.int64)
    return np.sign(ids) * (np.abs(ids) % a1)


def element_ranges(sizes, a1, a2):
    """type 2, the literal running loop of InvertedLists::copy_subset_to -> [(i1, i2)] per list"""
    nt = int(sum(int(s) for s in sizes))
    accu_n = accu_a1 = accu_a2 = 0
    out = []
    for n in sizes:
        next_n = accu_n + int(n)
        na1 = next_n * a1 // nt
        na2 = next_n * a2 // nt
        out.append((na1 - accu_a1, na2 - accu_a2))
        accu_n, accu_a1, accu_a2 = next_n, na1, na2
    return out


def subset_positions(lists, subset_type, a1, a2):
    """positions of the selected entries of every list, ascending (list order is kept)"""
    if subset_type == SUBSET_TYPE_ELEMENT_RANGE:
        return [np.arange(i1, i2, dtype=np.int64) for i1, i2 in element_ranges([len(ids) for _, ids in lists], a1, a2)]
    out = []
    for _, ids in lists:
        if subset_type == SUBSET_TYPE_ID_RANGE:
            m = (ids >= a1) & (ids < a2)
        elif subset_type == SUBSET_TYPE_ID_MOD:
            m = c_mod(ids, a1) == a2
        else:
            raise ValueError(f"subset type {subset_type}")
        out.append(np.nonzero(m)[0].astype(np.int64))
    return out


def subset_lists(lists, subset_type, a1, a2):
    return [(p[pos], ids[pos]) for (p, ids), pos in zip(lists, subset_positions(lists, subset_type, a1, a2))]
