"""CPU: the preconditions the route tests of IndexIVFScalarQuantizer (tests/test_gpu_sq_routes.py) lean on, asserted from the oracle
alone: the crowds defeat the certificate and nothing else does, the adversarial queries of set F overflow their candidate rows and no
other query does, the large-k cases of set D stay clear of the bound, and the rows of G and H are walked in the slices the tests name."""
import numpy as np
import pytest

import sq_ref

F32 = np.float32
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered")      # inf - inf between padded results
COMBOS = [(m, r) for m in (0, 1) for r in (False, True)]


def _tol(Dk, k):
    return np.abs(Dk[:, :k][np.isfinite(Dk[:, :k])]).max() * 2.0 ** -23      # the GPU tests' tolerance: from the k results


def _risky(name, metric, by_residual, k, Dp, q32):
    """queries whose gap between the exact k-th and the exact (K' + 1)-th score is under twice the bound the kernel uses (test_sq_host.py),
    at the state row's depth K'"""
    c = sq_ref.inputs(name)
    t, codes, xhat = sq_ref.quantised(name, by_residual)
    kp = sq_ref.kprime(k)
    eps = sq_ref.cert_eps(c.d, metric, by_residual, t, c.cen, codes, xhat, q32)
    if metric == 1:
        q2 = (q32.astype(np.float64) ** 2).sum(1)
        eps = 2 * eps + 3e-7 * (2 * np.abs(Dp[:, kp].astype(np.float64)) + 2 * q2)
    gap = np.abs(Dp[:, kp].astype(np.float64) - Dp[:, k - 1])
    return np.isfinite(Dp[:, kp]) & (gap < 2 * eps), gap


def test_kprime_is_the_state_rows_depth():
    assert [sq_ref.kprime(k) for k in (1, 10, 100, 1000, 3000, 4096)] == [16, 32, 128, 2048, 4096, 8192]


# ------------------------------------------------------------------------------------------ E, G, H: the crowds
@pytest.mark.parametrize("metric,by_residual", COMBOS)
@pytest.mark.parametrize("name,nprobe", [("E", 4), ("E", 1000), ("G", 4), ("H", 4)])
def test_the_crowd_defeats_the_certificate_and_nothing_else_does(name, nprobe, metric, by_residual):
    """Crowd queries: the exact scores of rank k and rank K' + 1 are equal (both inside the crowd), so no bound can clear them.  The other
    queries: near-ties at most 2 %, queries within 2 eps of the bound at most 5 %.  No run of equal scores shares a near-tie with an
    unequal neighbour: the id rule's mask never reaches into the crowd."""
    c = sq_ref.inputs(name)
    assert c.copies > sq_ref.kprime(max(c.ks)) and c.is_crowd_q.sum() in (4, 6)
    _, codes, _ = sq_ref.quantised(name, by_residual)
    crowd_rows = np.nonzero(np.isin(c.ids, c.crowd_ids))[0]
    assert len(crowd_rows) == c.copies + 1 and (codes[crowd_rows] == codes[c.r0]).all() and (c.assign[crowd_rows] == c.assign[c.r0]).all()
    assert (np.diff(c.ids[len(c.ids) - c.copies:]) == -1).all(), "the crowd's ids descend in insertion order"
    for k in c.ks:
        kp = sq_ref.kprime(k)
        Dk, Ik = sq_ref.expected(name, metric, by_residual, k + 1, None, nprobe)
        tol = _tol(Dk, k)
        share = sq_ref.near_tied(Dk, tol)[~c.is_crowd_q].mean()
        masked, _ = sq_ref.id_rule(Dk, tol)
        Dp, _ = sq_ref.expected(name, metric, by_residual, kp + 1, None, nprobe)
        risky, gap = _risky(name, metric, by_residual, k, Dp, c.q32)
        print(f"set {name} nprobe {nprobe} metric {metric} by_residual {by_residual} k {k}: near-tied share of the other queries {share:.5f}, "
              f"masked positions {masked.mean():.5f}, other queries within 2 eps {risky[~c.is_crowd_q].mean():.5f}, "
              f"largest crowd gap {gap[c.is_crowd_q].max():.1e}")
        assert share <= 0.02 and masked.mean() <= 0.02
        assert risky[~c.is_crowd_q].mean() <= 0.05
        assert (gap[c.is_crowd_q] == 0).all(), "rank k and rank K' + 1 of a crowd query lie inside the crowd"
        assert np.isin(Ik[c.is_crowd_q][:, k - 1], c.crowd_ids).all()
        assert not masked[c.is_crowd_q].any()
        # the oracle orders the crowd by ascending id: the original row first, then the copies from the LAST one added
        first = Ik[c.is_crowd_q][:, :k]
        inside = np.isin(first, c.crowd_ids)
        for row, m in zip(first, inside):
            assert (np.diff(row[m]) > 0).all()


def test_crowd_sets_keep_their_base():
    b, e = sq_ref.inputs("B"), sq_ref.inputs("E")
    assert np.array_equal(e.x32[:b.n], b.x32) and np.array_equal(e.q32[~e.is_crowd_q], b.q32) and e.cen is b.cen
    assert e.n == b.n + 300 and e.nq == b.nq + 6
    for name, d, nq in (("G", 1100, 70), ("H", 301, 200)):
        c = sq_ref.inputs(name)
        assert (c.d, c.n, c.nq, c.nlist, c.nprobe) == (d, 6040, nq + 4, 8, 4)
        print(f"set {name}: list sizes {c.sizes.min()} .. {c.sizes.max()}")


# ------------------------------------------------------------------------------------------ F: overflowing candidate rows
def _scores(metric, q, xhat):
    q, x = q.astype(np.float64), xhat.astype(np.float64)
    s = q @ x.T
    return s if metric == 0 else -((q ** 2).sum(1)[:, None] - 2 * s + (x ** 2).sum(1)[None, :])


@pytest.mark.parametrize("metric,by_residual", COMBOS)
def test_adversarial_queries_overflow_their_candidate_rows_and_no_other_query_does(orc, metric, by_residual):
    """The threshold of a query at k = 10 is the 32nd best score of the first 512 rows of its closest list.  An adversarial query's lets
    more than the row's 16384 keys through (by a margin of 1000); any other query's at most half a row.  Exact scores stand in for
    the scan's: the margins are thousands of rows against a bound of about 1e-6 relative."""
    c = sq_ref.inputs("F")
    assert np.array_equal(c.assign, c.labels), "the construction keeps every row in its list"
    assert c.sizes.tolist() == [24000, 4000, 4000, 4000] and c.nprobe == c.nlist
    tmax = (int(((c.sizes + 15) // 16 * 16).sum()) + 255) // 256 * 256
    cap = min(max(tmax, 1024), 16384)
    assert tmax > 16384 and cap == 16384, "a candidate row holds 16384 keys"
    assert sq_ref.kprime(10) == 32 and 4 * 32 <= 512, "one 512-row chunk of one list is the threshold sample"
    _, _, xhat = sq_ref.quantised("F", by_residual)
    first = [np.nonzero(c.assign == l)[0][:512] for l in range(c.nlist)]
    for key, adv in c.adv.items():
        q = c.qsets[key]
        pid, _ = orc.coarse_probe(c.cen, q, 1)
        S = _scores(metric, q, xhat)
        tau = np.array([np.sort(S[i, first[pid[i, 0]]])[-32] for i in range(len(q))])
        passing = (S > tau[:, None]).sum(1)
        is_adv = np.zeros(len(q), bool); is_adv[list(adv)] = True
        assert (pid[is_adv, 0] == 0).all() and (pid[~is_adv, 0] != 0).all()
        print(f"set F batch {key} metric {metric} by_residual {by_residual}: keys past the threshold: adversarial {passing[is_adv].tolist()}, "
              f"others at most {passing[~is_adv].max()}")
        assert (passing[is_adv] >= cap + 1000).all()
        assert (passing[~is_adv] <= cap // 2).all()
        assert len(adv) <= max(2, len(q) // 128) if key == "a" else max(2, len(q) // 128) < len(adv) <= 8


@pytest.mark.parametrize("metric,by_residual", COMBOS)
def test_set_f_near_ties_and_certificate_gaps(metric, by_residual):
    for key in ("a", "b"):
        Dk, _ = sq_ref.expected("F", metric, by_residual, 11, None, None, key)
        share = sq_ref.near_tied(Dk, _tol(Dk, 10)).mean()
        Dp, _ = sq_ref.expected("F", metric, by_residual, 33, None, None, key)
        risky, _ = _risky("F", metric, by_residual, 10, Dp, sq_ref.inputs("F").qsets[key])
        print(f"set F batch {key} metric {metric} by_residual {by_residual}: near-tied share {share:.5f}, queries within 2 eps {risky.mean():.5f}")
        assert share <= 0.02 and risky.mean() <= 0.05


def test_probing_every_list_of_f_equals_the_flat_oracle(orc):
    c = sq_ref.inputs("F")
    _, _, xhat = sq_ref.quantised("F", True)
    D, I = sq_ref.expected("F", 1, True, 11, None, None, "a")
    Dr, Ir = orc.flat_search(c.qsets["a"], xhat, 11, 1)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)


# ------------------------------------------------------------------------------------------ D at large k
@pytest.mark.parametrize("metric,by_residual", COMBOS)
@pytest.mark.parametrize("nprobe", [8, 16])
def test_large_k_on_set_d(nprobe, metric, by_residual):
    """k = 3000 (K' = 4096) and k = 4096 (K' = 8192) over the first 40 queries of set D (and all 200 at nprobe 16, k 4096): no query within
    2 eps of the bound at either certificate depth, near-ties (thousands of dense scores per query) at most 5 %; nprobe 8 pads many results, nprobe 16
    fills the state row."""
    c = sq_ref.inputs("D")
    t, codes, xhat = sq_ref.quantised("D", by_residual)
    for k, nq in ((3000, 40), (4096, 40)) + (((4096, 200),) if nprobe == 16 else ()):
        Dk, _ = sq_ref.expected("D", metric, by_residual, k + 1, nq, nprobe)
        share = sq_ref.near_tied(Dk, _tol(Dk, k)).mean()
        rows = np.isfinite(Dk).sum(1)                     # probed rows per query, capped at k + 1
        full = (rows > k).mean()
        eps = sq_ref.cert_eps(c.d, metric, by_residual, t, c.cen, codes, xhat, c.q32[:nq])
        risky = np.zeros(nq, bool)
        for depth in (k + max(8, k // 16), sq_ref.kprime(k)):       # the first re-score depth and the state row's
            Dp, _ = sq_ref.expected("D", metric, by_residual, depth + 1, nq, nprobe)
            e = eps
            if metric == 1:
                q2 = (c.q32[:nq].astype(np.float64) ** 2).sum(1)
                e = 2 * eps + 3e-7 * (2 * np.abs(Dp[:, depth].astype(np.float64)) + 2 * q2)
            gap = np.abs(Dp[:, depth].astype(np.float64) - Dp[:, k - 1])
            risky |= np.isfinite(Dp[:, depth]) & (gap < 2 * e)
        print(f"set D nprobe {nprobe} metric {metric} by_residual {by_residual} k {k} nq {nq}: near-tied share {share:.5f}, "
              f"queries within 2 eps {risky.mean():.5f}, probed rows {rows.min()} .. {'> k' if rows.max() > k else rows.max()}, full rows {full:.3f}")
        assert share <= 0.05
        assert risky.mean() == 0
        if nprobe == 8:
            assert (rows <= k).any(), "some results are padded"
        else:
            assert full >= 0.9 and (k != 3000 or full == 1)


# ------------------------------------------------------------------------------------------ shapes
def test_rows_of_g_and_h_are_sliced_as_the_tests_say():
    """k_sq_list_scan keeps min(ld, 1024) dimensions of 16 queries or min(ld, 256) of 64 in LDS and walks a row slice by slice, SQ_U = 4 K
    steps of 64 dimensions at a time."""
    assert sq_ref.scan_shape(1100, 1) == (1152, [16, 2]) and sq_ref.scan_shape(1100, 4) == (1152, [4, 4, 4, 4, 2])
    assert sq_ref.scan_shape(301, 1) == (320, [5]) and sq_ref.scan_shape(301, 4) == (320, [4, 1])
    assert 301 % 4 == 1 and 1100 % 64 != 0
    for d in (64, 100, 768):       # the sets A - D: one slice in the 16-query form, whole slices in the other, and only ns = 2 off a multiple of 4
        ld, s16 = sq_ref.scan_shape(d, 1)
        _, s64 = sq_ref.scan_shape(d, 4)
        assert len(s16) == 1 and len(set(s64)) == 1 and all(n % 4 == 0 or n in (1, 2) for n in s16 + s64)
