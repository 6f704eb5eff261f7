"""Reference of range_search: the oracle's complete, canonically ordered search result cut at the radius, the input sets the
range tests share, and the numpy restatement of the scan threshold (k_range.hip: k_range_tau)."""
import functools

import numpy as np

import sq_ref
import util

F32 = np.float32

# the Flat case: d = 100 (rows padded to 128 values), n crosses one 65 536-row chunk and is no multiple of a tile, nq = two 256-query tiles
# with a tail.  Radii by metric: (few or no results, a few thousand per query, tens of thousands per query)
FLAT = dict(d=100, n=70001, nq=300, ncent=16)
FLAT_RADII = {0: (125.0, 97.0, 8.0), 1: (0.99, 54.0, 226.0)}
# the IVF-Flat case
IVF = dict(d=64, n=60000, nq=203, nlist=40, ncent=16)
IVF_RADII = {0: (75.0, 50.0), 1: (20.0, 40.0)}       # (about ten results per query, thousands per query)
IVF768_RADII = {0: 740.0, 1: 380.0}
# many lists: nlist = 12 800 is the smallest at which the coarse selection (16 keys kept, segments of 4096 scores) has four segments and
# takes its two-phase form; the centroids are further rows of the vectors' mixture, so most lists stay empty
WIDE = dict(d=32, n=60000, nq=70, nlist=12800, ncent=16, nprobe=6)
# fp32 storage (test_gpu_range.py: fp32_case): no oracle score lies within 8 ulp of these (tests/test_range_host.py checks it)
FP32_RADII = {0: 97.0, 1: 54.0}


def cut(D, I, radius, metric):
    """An oracle result [nq, k] (canonical order: best first, ties by id; padded with I = -1) cut at the radius -> (lims, D, I):
    inner product keeps score > radius, L2 squared distance < radius, strictly, in fp32."""
    r = F32(radius)
    keep = ((D > r) if metric == 0 else (D < r)) & (I >= 0)
    cnt = keep.sum(1)
    assert (keep == (np.arange(D.shape[1])[None, :] < cnt[:, None])).all(), "the members of a canonically ordered row are a prefix"
    lims = np.zeros(len(D) + 1, dtype=np.int64)
    np.cumsum(cnt, out=lims[1:])
    return lims, D[keep].astype(F32), I[keep].astype(np.int64)


def _orc():
    from oracle import oracle as orc
    orc.build()
    return orc


@functools.lru_cache(maxsize=None)
def flat_inputs():
    orc = _orc()
    c = FLAT
    x = orc.synth_vectors(c["d"], c["ncent"], util.SEED_C, util.SEED_X, 0.5, 0, c["n"])
    q = orc.synth_queries(c["d"], c["ncent"], util.SEED_C, util.SEED_X, 0.5, c["n"], util.SEED_Q, 0.1, 0, c["nq"])
    return x, q


@functools.lru_cache(maxsize=None)
def flat_full(metric):
    """every score of every query in canonical order (ids as int32 to halve the cache)"""
    x, q = flat_inputs()
    D, I = _orc().flat_search(q.astype(F32), x.astype(F32), len(x), metric)
    return D, I.astype(np.int32)


def flat_expected(metric, radius, nq=None):
    D, I = flat_full(metric)
    return cut(D[:nq], I[:nq].astype(np.int64), radius, metric)


def flat_expected_of(q, x, metric, radius, ids=None):
    """the same for any (small) input"""
    D, I = _orc().flat_search(np.asarray(q, F32), np.asarray(x, F32), len(x), metric, ids)
    return cut(D, I, radius, metric)


def fp32_case(metric):
    """rows and queries fp16 cannot represent (the Flat index keeps fp32 rows) -> (x, q, radius)"""
    x, q = flat_inputs()
    rng = np.random.RandomState(5)
    x = (x[:6000].astype(F32) * (1 + 1e-4 * rng.randn(6000, x.shape[1]))).astype(F32)
    q = (q[:40].astype(F32) * (1 + 1e-4 * rng.randn(40, q.shape[1]))).astype(F32)
    return x, q, FP32_RADII[metric]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def ivf_inputs():
    orc = _orc()
    c = Case()
    c.__dict__.update(IVF)
    c.x = orc.synth_vectors(c.d, c.ncent, util.SEED_C, util.SEED_X, 0.5, 0, c.n)
    c.q = orc.synth_queries(c.d, c.ncent, util.SEED_C, util.SEED_X, 0.5, c.n, util.SEED_Q, 0.1, 0, c.nq)
    c.x32, c.q32 = c.x.astype(F32), c.q.astype(F32)
    c.cen = orc.kmeans(0, c.x32[orc.kmeans_sample(c.n, c.nlist, 256, 1234)], c.nlist, 4, 1234)
    c.assign, _ = orc.assign_ip(c.cen, c.x32)
    c.sizes = np.bincount(c.assign, minlength=c.nlist)
    return c


@functools.lru_cache(maxsize=None)
def wide_inputs():
    orc = _orc()
    c = Case()
    c.__dict__.update(WIDE)
    c.x = orc.synth_vectors(c.d, c.ncent, util.SEED_C, util.SEED_X, 0.5, 0, c.n)
    c.q = orc.synth_queries(c.d, c.ncent, util.SEED_C, util.SEED_X, 0.5, c.n, util.SEED_Q, 0.1, 0, c.nq)
    c.x32, c.q32 = c.x.astype(F32), c.q.astype(F32)
    c.cen = orc.synth_vectors(c.d, c.ncent, util.SEED_C, util.SEED_X, 0.5, c.n, c.nlist).astype(F32)
    c.assign, _ = orc.assign_ip(c.cen, c.x32)
    c.sizes = np.bincount(c.assign, minlength=c.nlist)
    return c


@functools.lru_cache(maxsize=None)
def ivf_full(name, metric, nprobe, explicit_ids=False):
    """name "ivf": the case above; "wide": the many-lists case; "D": sq_ref's d = 768 set (n 20 000, nlist 32, 200 queries)"""
    c = ivf_inputs() if name == "ivf" else wide_inputs() if name == "wide" else sq_ref.inputs("D")
    orc = _orc()
    ids = 7 * np.arange(c.n, dtype=np.int64) + 1000003 if explicit_ids else np.arange(c.n, dtype=np.int64)
    lm = orc.ListMajor(c.assign, ids, c.x32, c.nlist)
    k = int(np.sort(c.sizes)[::-1][:nprobe].sum())
    return orc.ivfflat_search(metric, c.cen, lm, c.q32, nprobe, k)


def ivf_expected(name, metric, nprobe, radius, explicit_ids=False):
    D, I = ivf_full(name, metric, nprobe, explicit_ids)
    return cut(D, I, radius, metric)


# ------------------------------------------------------------------------------------------ the threshold, restated
def scan_bound(d, metric, max_norm2, storage_f16):
    """(rel, rel_qlossy, xmax, abs) of the fp16 scans' error bound (api_stages.hip: scan_cert_bound), fp32 as the library forms them"""
    u24, u11 = F32(5.9604645e-8), F32(4.8828125e-4)
    xmax = F32(np.sqrt(F32(max_norm2))) * F32(1.0000002)
    rel = (F32(d) + F32(2)) * u24 * F32(1.01) + (F32(0) if storage_f16 else u11 * F32(1.002))
    rel_q = u11 * F32(1.002) + u11 * u11
    ab = F32(np.sqrt(F32(d))) * u24 + ((F32(d) + F32(4)) * u24 * xmax if metric == 1 else F32(0))
    return F32(rel), F32(rel_q), F32(xmax), F32(ab)


def threshold(q32, radius, metric, max_norm2, storage_f16=True, q_lossy=False):
    """-> (t float32 [nq], eps float32 [nq]): the scan admits ranking scores >= t (k_range_tau); ranking score = <q, x> (inner product) or
    <q, x> - |x|^2 / 2 (L2).  A query with a non-finite component gets t = +inf."""
    q32 = np.asarray(q32, F32)
    d = q32.shape[1]
    rel, rel_q, xmax, ab = scan_bound(d, metric, max_norm2, storage_f16)
    q2 = (q32.astype(np.float64) ** 2).sum(1)
    with np.errstate(invalid="ignore"):
        qn = (np.sqrt(q2).astype(F32) * F32(1.0000002)).astype(F32)
        r = F32(rel + (rel_q if q_lossy else F32(0)))
        eps = (r * qn * xmax + ab * (qn + xmax)).astype(F32)
        rad, qx = float(F32(radius)), qn.astype(np.float64) * float(xmax)
        t = rad - 2.0 ** -23 * qx if metric == 0 else 0.5 * (q2 - rad - 2.0 ** -22 * abs(rad))
        t = t - eps.astype(np.float64)
        t = t - 2.0 ** -40 * (np.abs(t) + q2 + abs(rad) + qx + eps.astype(np.float64))
        tf = t.astype(F32)
        tf = np.where(tf.astype(np.float64) > t, np.nextafter(tf, F32(-np.inf)), tf).astype(F32)
    tf = np.where(np.isfinite(q2), tf, F32(np.inf)).astype(F32)
    return tf, eps


def ranking_scores(q32_row, x32_rows, metric):
    """exact (fp64) ranking scores of stored rows against one query"""
    q, x = q32_row.astype(np.float64), x32_rows.astype(np.float64)
    s = x @ q
    return s if metric == 0 else s - 0.5 * (x * x).sum(1)


def ulp_distance(a, b):
    """|a - b| in units in the last place of fp32 arrays of equal sign"""
    ia, ib = np.asarray(a, F32).view(np.int32).astype(np.int64), np.asarray(b, F32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
