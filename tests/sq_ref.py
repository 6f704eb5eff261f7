"""numpy restatement of the QT_8bit scalar quantiser: train / encode / decode / reconstruct, the input sets the
scalar-quantiser tests share, and the certificate bound of the scan.  numpy's fp32 elementwise operations are the canon: every
operation below is fp32 and rounded once."""
import functools

import numpy as np

import util

F32 = np.float32


def train(y):
    """y float32 [n, d] (the vectors, or their residuals) -> trained float32 [2 d]: vmin then vdiff = fp32(max - vmin), over ALL rows."""
    y = np.asarray(y, dtype=F32)
    vmin = y.min(axis=0)
    return np.concatenate([vmin, y.max(axis=0) - vmin]).astype(F32)


def encode(trained, y):
    y = np.asarray(y, dtype=F32)
    d = y.shape[1]
    vmin, vdiff = trained[:d], trained[d:]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(vdiff != 0, (y - vmin) / vdiff, F32(0)).astype(F32)
    t = np.where(t > 0, t, F32(0))
    t = np.where(t < 1, t, F32(1)).astype(F32)
    return (F32(255.0) * t).astype(F32).astype(np.int32).astype(np.uint8)      # truncation


def decode(trained, codes):
    d = codes.shape[1]
    vmin, vdiff = trained[:d], trained[d:]
    t = ((codes.astype(F32) + F32(0.5)) / F32(255.0)).astype(F32)
    return (vmin + (vdiff * t).astype(F32)).astype(F32)


def reconstruct(trained, codes, centroids=None, assign=None):
    """The stored vector: the decoded code, plus (by_residual) the centroid of the vector's list, rounded once."""
    r = decode(trained, codes)
    return r if centroids is None else (np.asarray(centroids, F32)[assign] + r).astype(F32)


def cert_eps(d, metric, by_residual, trained, centroids, codes, xhat, q):
    """The bound |scan score - exact score| <= eps per query that the library's certificate uses (api_search.hip: finalize_args and
    k_finalize's certify_rows), in fp64: q float32 [nq, d] -> eps [nq]."""
    u24 = 2.0 ** -24
    V = np.sqrt((trained[d:].astype(np.float64) ** 2).sum()) * 1.000001
    W = np.sqrt((trained[:d].astype(np.float64) ** 2).sum()) * 1.000001
    X = np.sqrt((xhat.astype(np.float64) ** 2).sum(1).max()) * 1.0000002
    C = np.sqrt((np.asarray(centroids, np.float64) ** 2).sum(1).max()) * 1.000001
    B = np.sqrt(((codes.astype(np.int64) - 128) ** 2).sum(1).max())
    rB = float(np.abs(trained[d:]).max()) / 255.0 * B * 1.00001
    rel_b = ((2 * d + 2) * u24 + 2.0 ** -21 + np.sqrt(d) * 2.0 ** -27 + 2 * u24) * 1.01
    cq = rel_b * rB + 10 * u24 * 1.01 * (V + W)
    if by_residual:
        cq += u24 * 1.01 * ((d + 4) * C + 2 * X)
    cabs = np.sqrt(d) * u24 + ((d + 4) * u24 * X if metric == 1 else 0.0)
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(1)) * 1.0000002
    return cabs * (qn + X) + cq * qn


# ------------------------------------------------------------------------------------------ the shared input sets
class Case:
    pass


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(A) the golden IVF-Flat case at d 768 (short lists, one of 8 rows); (B) d 64, lists around the 512-row work item, 70 queries;
    (C) d 100 (rows padded to 128 bytes), nprobe = nlist; (D) d 768, lists of more than one 1024-row work item, 200 queries.
    (E) - (H): the sets of the route tests, route_inputs below."""
    from oracle import oracle as orc
    orc.build()
    if name in ROUTE_SETS:
        return route_inputs(name)
    c = Case()
    c.name = name
    if name == "A":
        g = util.load_golden("ivfflat_d768")
        x, q = util.regen(orc, g)
        c.d, c.n, c.nlist, c.nprobe, c.nq, c.ks = g["d"], g["n"], g["nlist"], g["nprobe"], g["nq"], (10,)
        c.x, c.q, c.cen = x, q, np.ascontiguousarray(g["centroids"], dtype=F32)
    else:
        d, n, nlist, nprobe, nq, ks, ncent = {"B": (64, 6000, 16, 4, 70, (1, 10, 100), 16), "C": (100, 3000, 8, 8, 7, (100,), 8),
                                              "D": (768, 20000, 32, 8, 200, (10, 1000), 32)}[name]
        x = orc.synth_vectors(d, ncent, util.SEED_C, util.SEED_X, 0.5, 0, n)
        q = orc.synth_queries(d, ncent, util.SEED_C, util.SEED_X, 0.5, n, util.SEED_Q, 0.1, 0, nq)
        if name != "D":      # fp32 inputs that fp16 cannot represent
            rng = np.random.RandomState(5)
            x = (x.astype(F32) * (1 + 1e-4 * rng.randn(n, d))).astype(F32)
            q = (q.astype(F32) * (1 + 1e-4 * rng.randn(nq, d))).astype(F32)
        c.d, c.n, c.nlist, c.nprobe, c.nq, c.ks = d, n, nlist, nprobe, nq, ks
        c.x, c.q = x, q
        c.cen = orc.kmeans(0, x.astype(F32)[orc.kmeans_sample(n, nlist, 256, 1234)], nlist, 4, 1234)
    c.x32, c.q32 = c.x.astype(F32), c.q.astype(F32)
    c.assign, _ = orc.assign_ip(c.cen, c.x32)
    c.sizes = np.bincount(c.assign, minlength=c.nlist)
    return c


@functools.lru_cache(maxsize=None)
def quantised(name, by_residual):
    """trained parameters (over all of x, or of its residuals), codes and stored vectors of an input set"""
    from oracle import oracle as orc
    c = inputs(name)
    y = orc.residuals(c.cen, c.x32, c.assign) if by_residual else c.x32
    t = train(y)
    codes = encode(t, y)
    xhat = reconstruct(t, codes, c.cen if by_residual else None, c.assign)
    return t, codes, xhat


@functools.lru_cache(maxsize=None)
def expected(name, metric, by_residual, k, nq=None, nprobe=None, qset=None):
    """The oracle's IVF-Flat search of the stored vectors: the expected result of a search, computed once per (set, metric, setting, k).
    nprobe: another count than the set's; qset: one of the set's other query batches (c.qsets)."""
    from oracle import oracle as orc
    c = inputs(name)
    _, _, xhat = quantised(name, by_residual)
    lm = orc.ListMajor(c.assign, getattr(c, "ids", np.arange(c.n)), xhat, c.nlist)
    q = c.q32 if qset is None else c.qsets[qset]
    q = q if nq is None else q[:nq]
    return orc.ivfflat_search(metric, c.cen, lm, q, min(c.nprobe if nprobe is None else nprobe, c.nlist), k)


def near_tied(Dref, tol):
    """positions of an oracle result [nq, k + 1] whose score lies within 2 tol of a neighbour's -> bool [nq, k]"""
    D = Dref.astype(np.float64)
    gap = np.abs(np.diff(D, axis=1)) <= 2 * tol          # [nq, k]: between rank i and i + 1
    gap = np.where(np.isfinite(D[:, 1:]) & np.isfinite(D[:, :-1]), gap, False)
    tied = gap.copy()
    tied[:, 1:] |= gap[:, :-1]
    return tied


# ------------------------------------------------------------------------------------------ the input sets of the route tests
# (tests/test_gpu_sq_routes.py; preconditions: tests/test_sq_routes_host.py)
ROUTE_SETS = ("E", "F", "G", "H")
# the row whose copies form the crowd of a set: its own best match under both metrics, and far enough down every other query's ranking
# that the crowd stays out of the certificate's way there (test_sq_routes_host.py asserts both)
CROWD_ROW = {"E": 83, "G": 25, "H": 60}


def kprime(k):
    """the state row's depth K' (api_search.hip: kp_for): k + max(8, k / 16), rounded up to a power of two, at least 16"""
    want = k + max(8, k // 16)
    return max(16, 1 << (want - 1).bit_length())


def _add_crowd(c, x, q, r0, copies, at):
    """`copies` further copies of row r0 behind x, with DESCENDING ids (column order and id order disagree inside the crowd), and
    len(at) queries x[r0] (1 + 1e-3 noise) at the positions `at` of the batch"""
    n0, d = x.shape
    c.r0, c.copies = r0, copies
    c.x = np.concatenate([x, np.repeat(x[r0:r0 + 1], copies, axis=0)]).astype(F32)
    c.ids = np.concatenate([np.arange(n0), n0 + copies - 1 - np.arange(copies)]).astype(np.int64)
    c.crowd_ids = np.concatenate([[r0], n0 + np.arange(copies)]).astype(np.int64)
    rng = np.random.RandomState(11)
    cq = (x[r0].astype(F32) * (1 + 1e-3 * rng.randn(len(at), d))).astype(F32)
    c.nq = len(q) + len(at)
    c.is_crowd_q = np.zeros(c.nq, bool)
    c.is_crowd_q[list(at)] = True
    c.q = np.empty((c.nq, d), F32)
    c.q[c.is_crowd_q], c.q[~c.is_crowd_q] = cq, q
    c.qsets = {"crowd": (x[r0].astype(F32) * (1 + 1e-3 * rng.randn(40, d))).astype(F32)}      # a batch of crowd queries only
    c.n = n0 + copies


def _orthogonal_unit(rng, cen):
    u = rng.randn(cen.shape[1]).astype(F32)
    for _ in range(4):                               # u orthogonal to every centroid: +-u does not move a row to another list
        for v in cen:
            u -= (u @ v) / (v @ v) * v
    return (u / np.linalg.norm(u)).astype(F32)


def route_inputs(name):
    """(E) set B and a crowd: 300 copies of one stored row, six queries at it — the certificate cannot clear them at K' 32 or 128.
    (F) d 64, four lists, nprobe 4: list 0 holds 24 000 rows whose first 1024 lie 8 u below the centroid and whose others 4 .. 8 u above it;
    a query at centroid + 5 .. 7 u takes a useless threshold from the sample of that list's first 512 rows and overflows its candidate
    row; 130 ordinary queries near rows of the lists 1 - 3, and the batches "a" (two adversarial queries) and "b" (five) in c.qsets.
    (G) d 1100 (rows of 1152 bytes), (H) d 301 (rows of 320 bytes, d % 4 = 1): 6000 rows in 8 lists, nprobe 4, a crowd of 40 copies and
    four queries at it."""
    from oracle import oracle as orc
    c = Case()
    c.name = name
    if name == "E":
        b = inputs("B")
        c.d, c.nlist, c.nprobe, c.ks, c.cen = b.d, b.nlist, b.nprobe, (10, 100), b.cen
        _add_crowd(c, b.x32, b.q32, CROWD_ROW[name], 300, (3, 17, 31, 40, 58, 75))
    elif name in ("G", "H"):
        d, n, nlist, nprobe, nq, at = {"G": (1100, 6000, 8, 4, 70, (2, 33, 50, 73)), "H": (301, 6000, 8, 4, 200, (7, 64, 130, 203))}[name]
        x = orc.synth_vectors(d, nlist, util.SEED_C, util.SEED_X, 0.5, 0, n)
        q = orc.synth_queries(d, nlist, util.SEED_C, util.SEED_X, 0.5, n, util.SEED_Q, 0.1, 0, nq)
        rng = np.random.RandomState(5)                  # fp32 inputs that fp16 cannot represent, as in (B)
        x = (x.astype(F32) * (1 + 1e-4 * rng.randn(n, d))).astype(F32)
        q = (q.astype(F32) * (1 + 1e-4 * rng.randn(nq, d))).astype(F32)
        c.d, c.nlist, c.nprobe, c.ks = d, nlist, nprobe, (1, 10)
        c.cen = orc.kmeans(0, x[orc.kmeans_sample(n, nlist, 256, 1234)], nlist, 4, 1234)
        _add_crowd(c, x, q, CROWD_ROW[name], 40, at)
    else:
        rng = np.random.RandomState(17)
        d, nlist, n0, per, nq = 64, 4, 24000, 4000, 130
        c.cen = (3.0 * rng.randn(nlist, d)).astype(F32)
        c.u = u = _orthogonal_unit(rng, c.cen)
        c.labels = np.concatenate([np.zeros(n0, np.int64), np.repeat(np.arange(1, nlist), per)])
        c.n = len(c.labels)
        x = c.cen[c.labels] + 0.3 * rng.randn(c.n, d).astype(F32)
        c.bad = 1024
        x[:c.bad] -= 8.0 * u[None, :]                                                             # list 0, first rows: far below for a query along +u
        x[c.bad:n0] += (4.0 + 4.0 * rng.rand(n0 - c.bad, 1).astype(F32)) * u[None, :]            # list 0, the rest: far above
        c.x = x.astype(F32)
        src = n0 + rng.randint(0, (nlist - 1) * per, nq)                                          # ordinary queries: near rows of lists 1 .. 3
        c.q = (c.x[src] + 0.05 * rng.randn(nq, d)).astype(F32)
        c.d, c.nlist, c.nprobe, c.nq, c.ks = d, nlist, nlist, nq, (10,)
        c.adv = {"a": {5: 6.0, 77: 5.0}, "b": {5: 6.0, 30: 5.5, 77: 5.0, 100: 6.5, 129: 7.0}}
        c.qsets = {}
        for key, at in c.adv.items():
            qs = c.q.copy()
            for pos, s in at.items():
                qs[pos] = c.cen[0] + F32(s) * u
            c.qsets[key] = qs.astype(F32)
    c.x32, c.q32 = c.x.astype(F32), c.q.astype(F32)
    c.assign, _ = orc.assign_ip(c.cen, c.x32)
    c.sizes = np.bincount(c.assign, minlength=c.nlist)
    return c


def scan_shape(d, qtiles):
    """how k_sq_list_scan walks a row of d dimensions in its 16-query (qtiles 1) or 64-query (4) form: (row bytes ld, [K steps of 64
    dimensions per slice])"""
    ld = (d + 63) // 64 * 64
    kc = min(ld, 256 if qtiles >= 4 else 1024)
    return ld, [min(kc, ld - k0) // 64 for k0 in range(0, ld, kc)]


def id_rule(Dk1, tol):
    """The id rule over an oracle result [nq, k + 1] -> (masked bool [nq, k], clusters): a position is masked where its score lies within
    2 tol of a neighbour's WITHOUT being equal to it; every other position's id must be the oracle's — runs of exactly equal scores
    included, which both sides order by ascending id.  clusters: (query, lo, hi) of every maximal run of positions [lo, hi) joined by
    gaps <= 2 tol that holds a masked position and does not reach rank k + 1: there the ids must be a permutation of the oracle's."""
    D = Dk1.astype(np.float64)
    fin = np.isfinite(D[:, 1:]) & np.isfinite(D[:, :-1])
    with np.errstate(invalid="ignore"):
        diff = np.abs(np.diff(D, axis=1))
    near = np.where(fin, diff <= 2 * tol, False)               # [nq, k]: between rank i and i + 1
    loose = near & np.where(fin, diff != 0, False)             # ... near, and not equal
    masked = loose.copy()
    masked[:, 1:] |= loose[:, :-1]
    clusters = []
    k = near.shape[1]
    for qi in np.nonzero(masked.any(axis=1))[0]:
        i = 0
        while i < k:
            j = i
            while j < k and near[qi, j]:
                j += 1
            # positions i .. j are joined (j = k: the run reaches rank k + 1)
            if j > i and j < k and masked[qi, i:j + 1].any():
                clusters.append((int(qi), i, j + 1))
            i = j + 1
    return masked, clusters


def check_result(D, I, Dk1, Ik1, k, metric, what, cap=0.02, capped=None):
    """test_gpu_sq.py's check_result under the id rule above: scores within tol = max |Dref| 2^-23, the padding, near-tied positions of the
    `capped` queries (default: all) at most `cap`, ids equal at every position that is not masked, permutations inside the masked runs"""
    Dref, Iref = Dk1[:, :k], Ik1[:, :k]
    tol = np.abs(Dref[np.isfinite(Dref)]).max() * 2.0 ** -23
    assert np.array_equal(np.isfinite(D), np.isfinite(Dref)), what
    pad = -np.inf if metric == 0 else np.inf
    assert (D[~np.isfinite(Dref)] == pad).all() and (I[~np.isfinite(Dref)] == -1).all(), what
    with np.errstate(invalid="ignore"):               # inf - inf between padded results
        err = np.abs(np.where(np.isfinite(Dref), D.astype(np.float64) - Dref, 0.0))
        tied = near_tied(Dk1, tol)
    print(f"{what}: max score error {err.max():.3e} (tol {tol:.3e})")
    assert err.max() <= tol, what
    masked, clusters = id_rule(Dk1, tol)
    sel = tied if capped is None else tied[capped]
    share = sel.mean() if sel.size else 0.0
    print(f"{what}: near-tied share {share:.5f}, masked {masked.mean():.5f}")
    assert share <= cap and masked.mean() <= cap, what
    bad = (I != Iref) & ~masked
    assert not bad.any(), f"{what}: ids differ at {np.argwhere(bad)[:4].tolist()}: got {I[bad][:4].tolist()} want {Iref[bad][:4].tolist()}"
    for qi, lo, hi in clusters:
        assert sorted(I[qi, lo:hi].tolist()) == sorted(Iref[qi, lo:hi].tolist()), f"{what}: query {qi} ranks {lo} .. {hi - 1} are no permutation"
