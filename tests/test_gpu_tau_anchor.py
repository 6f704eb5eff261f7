"""GPU: the exact anchor of the four-query threshold pre-pass (k_pq_prepass4, engine parameter pq_tau_anchor).

The pre-pass re-scores the k best rows of its sample canonically and raises the threshold from a_k - 2 eps to s_k - eps.  Every case here
is compared with the CPU oracle (orc.ivfpq_search) with ids and fp32 scores bit-equal, for every query, and no query may take the exact
re-run (fallback_queries == 0).  At an equal sample the anchored threshold is never below the parent's, so the scan never lets more keys
through (cand_keys under profile 2).

Shapes: nlist 8 over ~36 000 vectors = lists of ~4500 rows, 64 queries x nprobe 4 = 32 probing queries per list: the smallest index
on which the sliced layout takes k_pq_scan_sl8 (ntotal >= 4096 nlist) and a list is longer than the largest sample (3520 rows)."""
import numpy as np
import pytest

from util import assert_same_results

pytestmark = pytest.mark.gpu

NLIST, NPROBE, K, NQ = 8, 4, 10, 64
_CASES = {}


def _centroids(d, seed):
    rng = np.random.RandomState(seed)
    cen = rng.randn(NLIST, d).astype(np.float32)
    return (3.0 * cen / np.linalg.norm(cen, axis=1, keepdims=True)).astype(np.float32)


def _data(cen, per_list, seed, sigma=0.3):
    """per_list rows around each centroid, dealt round-robin: a list holds its ids in ascending order, and with equal lists a row's
    position in its list is id // NLIST."""
    rng = np.random.RandomState(seed)
    per = [per_list] * NLIST if np.isscalar(per_list) else list(per_list)
    lab = np.array([l for r in range(max(per)) for l in range(NLIST) if r < per[l]])
    x = (cen[lab] + sigma * rng.randn(len(lab), cen.shape[1])).astype(np.float16)
    return x, lab


def _queries(cen, x, nq, seed, labels=None):
    rng = np.random.RandomState(seed)
    rows = rng.randint(0, len(x), nq) if labels is None else labels
    return (x[rows].astype(np.float32) + 0.05 * rng.randn(nq, x.shape[1])).astype(np.float32)


def _build(gpu, orc, d, M, layout, x, cen, tag):
    """Index + oracle lists, once per case (the reference stays as it is)."""
    if tag not in _CASES:
        x32 = x.astype(np.float32)
        a, _ = orc.assign_ip(cen, x32)
        res = orc.residuals(cen, x32, a)
        cb = orc.pq_train(res[:4000], M, 3, 1234)
        lm = orc.ListMajor(a, np.arange(len(x)), orc.pq_encode(cb, res), NLIST)
        ix = gpu.IndexIVFPQ(None, d, NLIST, M, 8, gpu.METRIC_INNER_PRODUCT)
        ix.set_param("pq_layout", layout)
        ix.set_centroids(cen); ix.set_codebooks(cb); ix.add(x)
        assert ix._get("pq_layout") == layout
        ix.nprobe = NPROBE
        _CASES[tag] = (ix, cb, lm, a)
    return _CASES[tag]


def _search(ix, q, k, anchor, pre_rows=None):
    """One profiled batch: (D, I, keys that passed the scan's filter, exact re-runs, queries per table gather of the scan: 8 = k_pq_scan_sl8
    on the sliced layout and the eight-query k_pq_scan_rot at M = 64)."""
    ix.set_param("pq_tau_anchor", anchor)
    if pre_rows is not None:
        ix.set_param("pq_pre_rows", pre_rows)
    ix.set_param("profile", 2)
    D, I = ix.search(q, k)
    out = (D, I, ix.get_timing("cand_keys"), ix.get_timing("fallback_queries"), ix.get_timing("scan_group_queries"))
    # the route: the four-query pre-pass, anchored or not as asked, on the sample asked for
    assert ix.get_timing("pq_prepass4_batches") == 1 and ix.get_timing("pq_anchored_batches") == (1 if anchor else 0)
    assert pre_rows is None or ix.get_timing("pq_pre_rows_used") == pre_rows
    ix.set_param("profile", 0)
    ix.set_param("pq_tau_anchor", 1)
    return out


def _check(ix, orc, cen, cb, lm, q, k, label, gq):
    Dr, Ir = orc.ivfpq_search(cen, cb, lm, q, NPROBE, k)
    samples = (1024, 2048) if len(q) <= 64 else (2048, 3520)       # up to 64 queries the pre-pass samples 2048 rows at most
    for rows in samples:            # equal samples: the anchored threshold is the parent's or higher
        got = {}
        for anchor in (1, 0):
            D, I, cand, fb, g = _search(ix, q, k, anchor, rows)
            print(f"{label} sample {rows} pq_tau_anchor={anchor}: cand_keys {cand:.0f} fallback {fb:.0f} scan_group_queries {g:.0f}")
            assert g == gq, f"{label}: the scan gathers for {g} queries, expected {gq}"
            assert fb == 0, f"{label} sample {rows} anchor {anchor}: {fb} exact re-runs"
            assert_same_results(D, I, Dr, Ir, f"{label} sample {rows} pq_tau_anchor={anchor}")
            got[anchor] = cand
        assert got[1] <= got[0], f"{label} sample {rows}: anchored {got[1]} keys > parent rule {got[0]}"
    return Dr, Ir


@pytest.mark.parametrize("d,M,layout,gq", [(192, 96, 2, 8), (128, 64, 1, 8)], ids=["sliced-M96", "rotated-M64"])
def test_anchor_matches_oracle_and_never_loosens(gpu, orc, d, M, layout, gq):
    cen = _centroids(d, 3)
    x, _ = _data(cen, 4500, 5)
    ix, cb, lm, a = _build(gpu, orc, d, M, layout, x, cen, ("plain", d, M, layout))
    assert np.bincount(a, minlength=NLIST).min() >= 4096
    _check(ix, orc, cen, cb, lm, _queries(cen, x, NQ, 7), K, f"d{d} M{M} layout {layout}", gq)
    _check(ix, orc, cen, cb, lm, _queries(cen, x, NQ + 3, 9), K, f"d{d} M{M} layout {layout}, 67 queries", gq)    # the 3520-row sample, a ragged last workgroup
    # the defaults (the sample the anchored pre-pass chooses itself), k = 25 (the largest k of this pre-pass) and a ragged batch
    for k, nq in ((K, NQ), (25, NQ), (K, NQ + 3)):
        qq = _queries(cen, x, nq, 11 + k)
        ix2 = gpu.IndexIVFPQ(None, d, NLIST, M, 8, gpu.METRIC_INNER_PRODUCT)      # a handle whose pq_pre_rows was never set
        ix2.set_param("pq_layout", layout); ix2.set_centroids(cen); ix2.set_codebooks(cb); ix2.add(x); ix2.nprobe = NPROBE
        Dr, Ir = orc.ivfpq_search(cen, cb, lm, qq, NPROBE, k)
        for anchor in (1, 0):
            D, I, cand, fb, g = _search(ix2, qq, k, anchor)
            print(f"defaults k={k} nq={nq} pq_tau_anchor={anchor}: cand_keys {cand:.0f}")
            assert fb == 0 and g == gq
            assert_same_results(D, I, Dr, Ir, f"defaults k={k} nq={nq} pq_tau_anchor={anchor}")


@pytest.mark.parametrize("d,M,layout,gq", [(192, 96, 2, 8), (128, 64, 1, 8)], ids=["sliced-M96", "rotated-M64"])
def test_ties_at_the_kth_score(gpu, orc, d, M, layout, gq):
    """40 exact duplicates of a high-scoring vector inside the sample of list 0 (more than the 32 anchor rows, 4 k) and 12 more behind the
    sample: the k-th score is tied 52 times, the anchor is that score itself, and the drop rule's strict < must keep every duplicate."""
    cen = _centroids(d, 3)
    x, _ = _data(cen, 4500, 5)
    x = x.copy()
    dup = (1.6 * cen[0]).astype(np.float16)
    inside = 8 * (5 + 50 * np.arange(40))            # list positions 5, 55, ..., 1955 < 2048
    behind = 8 * (3600 + 70 * np.arange(12))         # positions 3600 ... 4370 > 3520
    x[inside] = dup; x[behind] = dup
    ix, cb, lm, a = _build(gpu, orc, d, M, layout, x, cen, ("ties", d, M, layout))
    assert (a[inside] == 0).all() and (a[behind] == 0).all() and (a[::8] == 0).all()
    rng = np.random.RandomState(13)
    q = np.concatenate([(cen[0] + 0.05 * rng.randn(40, d)).astype(np.float32), _queries(cen, x, NQ - 40, 17)])
    Dr, Ir = _check(ix, orc, cen, cb, lm, q, K, f"ties d{d} M{M}", gq)
    assert (Dr[:40] == Dr[:40, :1]).all() and np.isin(Ir[:40], np.concatenate([inside, behind])).all(), "the duplicates should own the top k of the first 40 queries"


@pytest.mark.parametrize("d,M,layout,gq", [(192, 96, 2, 8), (128, 64, 1, 8)], ids=["sliced-M96", "rotated-M64"])
def test_degenerate_samples(gpu, orc, d, M, layout, gq):
    """A closest list of 6 < k rows (no threshold from a sample without k rows: the parent rule takes over), closest lists shorter than the
    sample (40, 30 and 20 rows; 40 > the 32 anchor rows), a batch of 67 = 16 x 4 + 3 queries, and a query whose tables are constant (the
    zero query: scale falls back to 1, every score is +0, all 40 rows of its closest list tie).  The centroids of the four short lists lie
    60 degrees apart and far from the others, so a query near one of them probes exactly these four lists, 96 rows in all — as does the zero
    query (equal coarse scores, lowest index first): without a threshold every probed row is a candidate, and 96 fit the candidate row."""
    rng = np.random.RandomState(23)
    cen = _centroids(d, 3)
    qr = np.linalg.qr(rng.randn(d, 5))[0].T.astype(np.float32)          # orthonormal b, e0..e3
    cen[:4] = 3.0 * np.sqrt(0.5) * (qr[0] + qr[1:5])
    per = [40, 6, 30, 20, 8200, 8200, 8200, 8200]          # 32 896 >= 4096 nlist rows: k_pq_scan_sl8 on the sliced layout
    x, lab = _data(cen, per, 19)
    ix, cb, lm, a = _build(gpu, orc, d, M, layout, x, cen, ("degenerate", d, M, layout))
    assert list(np.bincount(a, minlength=NLIST)) == per
    nq = NQ + 3
    q = _queries(cen, x, nq, 29)
    for l, (q0, q1) in enumerate(((0, 8), (8, 16), (16, 20), (20, 24))):       # queries whose closest list is list 0, 1, 2, 3
        q[q0:q1] = (cen[l] + 0.05 * rng.randn(q1 - q0, d)).astype(np.float32)
    q[24] = 0.0
    pid, _ = orc.coarse_probe(cen, q[:25], NPROBE)
    assert (np.sort(pid, axis=1) == np.arange(4)).all(), pid
    assert [int(p[0]) for p in pid[[0, 8, 16, 20]]] == [0, 1, 2, 3]
    _check(ix, orc, cen, cb, lm, q, K, f"degenerate d{d} M{M}", gq)
