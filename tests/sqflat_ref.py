"""numpy restatement of what IndexScalarQuantizer's int8 scan adds to the QT_8bit scalar quantiser of tests/sq_ref.py: the
bit budget, the query planes (k_sq_gemm.hip: k_sqflat_planes), the scan's score and the certificate bound (api_sqflat.hip:
sqf_finalize_args), and the expected results the flat tests share.  Every fp32 operation is numpy's, rounded once."""
import functools

import numpy as np

import sq_ref

F32 = np.float32
SETS = ("B", "C", "D", "G", "H")


def wmax(d):
    """largest |w_j| of a scaled query (rsx_sqflat.h: sqflat_wmax): the planes hold 127 * 128 + 63, and (wmax + 64) * 128 * d < 2^31"""
    return min(16319, (2 ** 31 - 1) // (128 * d) - 64)


def kprime(k):
    """the state row's depth K' of this kind (api_sqflat.hip: sqf_plan): sq_ref.kprime, doubled below 1024 where it is under 2 k + 16"""
    kp = sq_ref.kprime(k)
    return 2 * kp if kp < 2 * k + 16 and kp < 1024 else kp


def planes(trained, q32):
    """q float32 [nq, d] -> (h int8 [nq, d], l int8 [nq, d], inv float32 [nq] = fl(1 / s), qc float32 [nq]): w = 128 h + l"""
    q32 = np.asarray(q32, F32)
    d = q32.shape[1]
    vmin, vdiff = trained[:d], trained[d:]
    W = wmax(d)
    qp = ((q32 * vdiff).astype(F32) / F32(255.0)).astype(F32)
    qc = (q32.astype(np.float64) * vmin.astype(np.float64) + 128.5 * qp.astype(np.float64)).sum(1).astype(F32)
    mx = np.abs(qp).max(1)
    ok = (mx > 0) & np.isfinite(mx)
    with np.errstate(divide="ignore", over="ignore"):
        s = np.where(ok, np.minimum((F32(W) / np.where(ok, mx, F32(1))).astype(F32), F32(2.0 ** 100)), F32(1)).astype(F32)
    inv = (F32(1.0) / s).astype(F32)
    w = np.clip(np.rint((qp * s[:, None]).astype(F32)).astype(np.int64), -W, W)
    h = (w + 64) >> 7
    l = w - (h << 7)
    assert np.abs(h).max() <= 127 and l.min() >= -64 and l.max() <= 63
    return h.astype(np.int8), l.astype(np.int8), inv, qc


def int_sums(h, l, codes):
    """(128 A_h, A) int64 [nq, n], A = sum_j w_j (code_j - 128): the products run through float64 BLAS, where every partial sum is an
    integer below 2^53"""
    b = (codes.astype(np.float64) - 128.0).T
    Ah = (h.astype(np.float64) @ b).astype(np.int64)
    Al = (l.astype(np.float64) @ b).astype(np.int64)
    return 128 * Ah, 128 * Ah + Al


def scan_scores(A, inv, qc, bias=None):
    """the kernel's fp32 score of every (query, row): fl(fl(fl(A) inv) + qc) (+ bias)"""
    sc = ((A.astype(F32) * inv[:, None]).astype(F32) + qc[:, None]).astype(F32)
    return sc if bias is None else (sc + bias[None, :]).astype(F32)


def rho_of(trained, q32):
    """the batch's largest max_j |q'_j| / |q| (k_sqflat_planes' running maximum), rounded up as the kernel does"""
    d = q32.shape[1]
    qp = ((np.asarray(q32, F32) * trained[d:]).astype(F32) / F32(255.0)).astype(F32)
    mx = np.abs(qp).max(1).astype(np.float64)
    qn = np.sqrt((q32.astype(np.float64) ** 2).sum(1))
    ok = (mx > 0) & np.isfinite(mx) & (qn > 0)
    return float(((mx[ok] / qn[ok]).astype(F32) * F32(1.000001)).max()) if ok.any() else 0.0


def cert_eps(d, metric, trained, codes, xhat, q):
    """|scan score - exact score| <= eps per query of the batch q (api_sqflat.hip: sqf_finalize_args, k_finalize's certify_rows), in fp64
    -> eps [nq]"""
    u24 = 2.0 ** -24
    W = wmax(d)
    V = np.sqrt((trained[d:].astype(np.float64) ** 2).sum()) * 1.000001
    Wn = np.sqrt((trained[:d].astype(np.float64) ** 2).sum()) * 1.000001
    X = np.sqrt((xhat.astype(np.float64) ** 2).sum(1).max()) * 1.0000002
    Bn = np.sqrt(((codes.astype(np.int64) - 128) ** 2).sum(1).max()) * 1.00001
    r = float(np.abs(trained[d:]).max()) / 255.0 * 1.00001
    rho = min(rho_of(trained, q), r)
    hw = np.sqrt(d) / (2.0 * W)
    rel_b = (u24 + 4 * u24 * (1 + hw) + 2 * u24) * 1.01
    cq = hw * 1.000001 * 1.01 * rho * Bn + rel_b * r * Bn + 10 * u24 * 1.01 * (V + Wn)
    cabs = np.sqrt(d) * u24 + ((d + 4) * u24 * X if metric == 1 else 0.0)
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(1)) * 1.0000002
    return cabs * (qn + X) + cq * qn


@functools.lru_cache(maxsize=None)
def quantised(name):
    """(trained, codes, xhat) of an input set as a flat scalar quantiser holds it: trained over the vectors themselves, no centroids"""
    c = sq_ref.inputs(name)
    t = sq_ref.train(c.x32)
    codes = sq_ref.encode(t, c.x32)
    return t, codes, sq_ref.reconstruct(t, codes)


@functools.lru_cache(maxsize=None)
def expected(name, metric, k):
    """the oracle's Flat search of the decoded vectors (ids = positions)"""
    from oracle import oracle as orc
    c = sq_ref.inputs(name)
    _, _, xhat = quantised(name)
    return orc.flat_search(c.q32, xhat, k, metric)


def ks_all(name):
    """k in {1, 10, 100, 1000} where the set has that many rows (the host-side certificate precondition)"""
    return tuple(k for k in (1, 10, 100, 1000) if k <= sq_ref.inputs(name).n)


def l2_eps(eps, Dp_kp, q32):
    """a distance moves by twice the ranking score's bound, plus the conversion's roundings (k_finalize: certify_rows)"""
    q2 = (q32.astype(np.float64) ** 2).sum(1)
    return 2 * eps + 3e-7 * (2 * np.abs(Dp_kp.astype(np.float64)) + 2 * q2)


@functools.lru_cache(maxsize=None)
def uncertifiable(name, metric, k):
    """bool [nq]: queries whose exact k-th score lies within 2 eps of their exact (K' + 1)-th at K' = sq_ref.kprime(k) — no bound of this
    size can clear them there (the kind's own K', kprime above, is that or twice that: the cut lies deeper, the gap is no smaller)"""
    c = sq_ref.inputs(name)
    t, codes, xhat = quantised(name)
    kp = sq_ref.kprime(k)
    if kp + 1 > c.n:
        return np.zeros(len(c.q32), bool)
    Dp, _ = expected(name, metric, kp + 1)
    eps = cert_eps(c.d, metric, t, codes, xhat, c.q32)
    if metric == 1:
        eps = l2_eps(eps, Dp[:, kp], c.q32)
    gap = np.abs(Dp[:, kp].astype(np.float64) - Dp[:, k - 1])
    return np.isfinite(Dp[:, kp]) & (gap < 2 * eps)
