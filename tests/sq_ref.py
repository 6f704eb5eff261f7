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
    (C) d 100 (rows padded to 128 bytes), nprobe = nlist; (D) d 768, lists of more than one 1024-row work item, 200 queries."""
    from oracle import oracle as orc
    orc.build()
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
def expected(name, metric, by_residual, k, nq=None):
    """The oracle's IVF-Flat search of the stored vectors: the expected result of a search, computed once per (set, metric, setting, k)."""
    from oracle import oracle as orc
    c = inputs(name)
    _, _, xhat = quantised(name, by_residual)
    lm = orc.ListMajor(c.assign, np.arange(c.n), xhat, c.nlist)
    q = c.q32 if nq is None else c.q32[:nq]
    return orc.ivfflat_search(metric, c.cen, lm, q, min(c.nprobe, c.nlist), k)


def near_tied(Dref, tol):
    """positions of an oracle result [nq, k + 1] whose score lies within 2 tol of a neighbour's -> bool [nq, k]"""
    D = Dref.astype(np.float64)
    gap = np.abs(np.diff(D, axis=1)) <= 2 * tol          # [nq, k]: between rank i and i + 1
    gap = np.where(np.isfinite(D[:, 1:]) & np.isfinite(D[:, :-1]), gap, False)
    tied = gap.copy()
    tied[:, 1:] |= gap[:, :-1]
    return tied
