"""Expected vectors of the reconstruct tests, from the oracle alone: orc.assign_ip / orc.residuals give lists and
residuals, orc.pq_encode the codes, sq_ref.encode / sq_ref.reconstruct the scalar-quantised vectors, a numpy table lookup plus one fp32
add the PQ decode.  The trained parameters are NOT trained: any centroids, codebooks and ranges define a stored vector, so they are drawn
from the data (cheap, deterministic) and go into the GPU index through set_centroids / set_codebooks / set_sq_trained.  Nothing expected
is read back from the code under test."""
import functools

import numpy as np

import sq_ref
import util

F32 = np.float32
N, NLIST = 6000, 8      # lists of about 750 rows: they cross the 16-, 32-, 64- and 512-row layout boundaries and end mid-block


class Case:
    pass


def _orc():
    from oracle import oracle as orc
    orc.build()
    return orc


@functools.lru_cache(maxsize=None)
def vectors(d, fp16=True, n=N):
    """x [n, d]: fp16 mixture data, or (fp16 False) float32 values that fp16 cannot represent (the rows are then stored as fp32)."""
    orc = _orc()
    x = orc.synth_vectors(d, NLIST, util.SEED_C, util.SEED_X, 0.5, 0, n)
    if not fp16:
        x = (x.astype(F32) * (1 + 1e-4 * np.random.RandomState(5).randn(n, d))).astype(F32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def coarse(d, fp16=True, n=N):
    """-> (centroids float32 [NLIST, d], assign int32 [n]): two k-means iterations of the oracle, the oracle's argmax-IP assignment"""
    orc = _orc()
    x32 = vectors(d, fp16, n).astype(F32)
    cen = orc.kmeans(0, x32[:2048], NLIST, 2, 1234)
    assign, _ = orc.assign_ip(cen, x32)
    return cen, assign


def pq_decode(cb, codes):
    """ProductQuantizer::decode: the codebook entries side by side, float32 [n, M dsub]"""
    return np.concatenate([cb[m][codes[:, m]] for m in range(cb.shape[0])], axis=1).astype(F32)


@functools.lru_cache(maxsize=None)
def pq_case(d, M, flat=False):
    """IVF-PQ (flat False): xhat = fl32(centroid + decoded residual code); IndexPQ (flat True): the decoded code of x itself, nothing added.
    Codebooks: 256 distinct sub-vectors of the encoded vectors per sub-quantiser; one entry component is -0.0 (it must come back as -0
    from an IndexPQ, where nothing is added to it)."""
    orc = _orc()
    c = Case()
    c.d, c.M, c.n, c.nlist = d, M, N, (1 if flat else NLIST)
    c.x = vectors(d)
    x32 = c.x.astype(F32)
    if flat:
        c.cen, c.assign, y = None, np.zeros(N, dtype=np.int32), x32
    else:
        c.cen, c.assign = coarse(d)
        y = orc.residuals(c.cen, x32, c.assign)
    dsub = d // M
    rng = np.random.RandomState(1000 * M + d)
    cb = np.stack([y[rng.choice(N, 256, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)]).astype(F32)
    cb[0, 3, 0] = F32(-0.0)
    cb[M - 1, 200, dsub - 1] = F32(-0.0)
    c.cb = np.ascontiguousarray(cb)
    c.codes = orc.pq_encode(c.cb, y)
    dec = pq_decode(c.cb, c.codes)
    c.xhat = dec if flat else (c.cen[c.assign] + dec).astype(F32)      # one fp32 add per component
    return c


@functools.lru_cache(maxsize=None)
def sq_case(d, by_residual):
    """IVF-SQ: sq_ref's train / encode / reconstruct over float32 inputs that fp16 cannot represent"""
    orc = _orc()
    c = Case()
    c.d, c.n, c.nlist, c.by_residual = d, N, NLIST, by_residual
    c.x = vectors(d, False)
    c.cen, c.assign = coarse(d, False)
    y = orc.residuals(c.cen, c.x, c.assign) if by_residual else c.x
    c.trained = sq_ref.train(y)
    c.codes = sq_ref.encode(c.trained, y)
    c.xhat = sq_ref.reconstruct(c.trained, c.codes, c.cen if by_residual else None, c.assign)
    return c


def storage_order(assign, nlist):
    """positions of the vectors in (list number, in-list offset) order, for an index filled by ONE add of everything"""
    return np.argsort(np.asarray(assign), kind="stable")


def bits(a):
    """the uint32 view all comparisons are made on (bit equality: -0 != +0, all-ones words compare equal)"""
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)
