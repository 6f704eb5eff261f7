"""CPU: the anchored threshold of the IVF-PQ pre-pass (k_pq_prepass4) restated in numpy — the proof as an executable check.

Tables are quantised the way k_pq_lut8 does it (one scale per query, one offset per sub-quantiser, eps = 1.0001 x the sum of the per-m
maximum errors + the fp32 slack term), vectors are random code sets, every operation is rounded to fp32 where the kernels round:

  a(v)  = dis0 + fma(scale, A(v), bias)                  the scan's approximate score, A = the integer sum of the 8-bit entries
  s(v)  = dis0 + (((0 + T[0][c0]) + T[1][c1]) + ...)     the canonical score
  tau   = down(a_k - 2.0002 eps)                         the parent rule: a_k = the k-th best a(.) of the sample
  tau'  = down(s_k - 1.0001 eps)                         s_k = the k-th best s(.) of the sample rows with A >= A_k, at most 32 in position order

Asserted for a few hundred seeds: a vector whose canonical score reaches the k-th best canonical score of ALL vectors passes the scan's
test a(v) > tau' (nothing that belongs to the result is dropped), and tau' >= tau (nothing the parent dropped comes back)."""
import numpy as np
import pytest

F = np.float32
ANCH = 32


def fma(a, b, c):
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def down(t):
    return F(t - F(F(np.abs(t) * F(4.8e-7)) + F(1e-30)))


def quantise(T):
    """k_pq_lut8: T [M, 256] fp32 -> u8 table, scale, bias, eps."""
    M = T.shape[0]
    mn, mx = T.min(axis=1), T.max(axis=1)
    maxrange = F((mx - mn).max())
    scale = F(maxrange / F(255.0)) if maxrange > 0 else F(1.0)
    inv = F(F(1.0) / scale)
    u = np.clip(np.rint((T - mn[:, None]) * inv), 0.0, 255.0).astype(F)
    err = np.abs(T - (mn[:, None] + scale * u).astype(F)).astype(F).max(axis=1)
    e_quant, bias, absmax = F(0), F(0), F(0)
    for m in range(M):
        e_quant = F(e_quant + err[m]); bias = F(bias + mn[m]); absmax = F(absmax + max(abs(mn[m]), abs(mx[m])))
    return u.astype(np.int64), scale, bias, e_quant, absmax


def thresholds(T, dis0, codes, sample, k):
    M, n = T.shape[0], len(codes)
    u, scale, bias, e_quant, absmax = quantise(T)
    slack = F(F(3 * M + 12) * F(5.9604645e-8) * F(1.05))
    B = F(absmax + abs(dis0) + abs(bias) + F(scale * F(255.0) * F(M)) + F(1.0))
    eps = F(F(e_quant * F(1.0001)) + F(slack * B))
    A = u[np.arange(M)[None, :], codes].sum(axis=1)                       # exact integers
    a = np.array([F(dis0 + fma(scale, F(Av), bias)) for Av in A], dtype=F)
    s = np.zeros(n, F)
    for m in range(M):                                                    # sequential fp32 sum in m order
        s = (s + T[m, codes[:, m]]).astype(F)
    s = (F(dis0) + s).astype(F)
    A_k = np.sort(A[:sample])[-k]
    a_k = F(dis0 + fma(scale, F(A_k), bias))
    tau = down(fma(F(-2.0002), eps, a_k))
    anchors = np.nonzero(A[:sample] >= A_k)[0][:ANCH]                     # position order, capped
    assert len(anchors) >= k
    s_k = np.sort(s[anchors])[-k]
    tau2 = down(fma(F(-1.0001), eps, s_k))
    return a, s, tau, tau2


@pytest.mark.parametrize("seed", range(300))
def test_anchored_threshold_keeps_the_result_and_never_loosens(seed):
    rng = np.random.default_rng(seed)
    M = int(rng.choice([4, 8, 16, 32, 64, 96]))
    n, k = 600, int(rng.choice([1, 3, 10, 25]))
    sample = int(rng.choice([k, 40, 128, 600]))
    spread = 10.0 ** rng.uniform(-3, 3)
    T = (spread * rng.standard_normal((M, 256)) * rng.uniform(0.05, 1.0, size=(M, 1)) + rng.standard_normal((M, 1)) * spread).astype(F)
    if seed % 7 == 0:
        T[rng.integers(0, M)] = F(rng.standard_normal())                  # a constant sub-table
    if seed % 50 == 0:
        T[:] = F(0.25)                                                    # every entry equal: scale falls back to 1
    dis0 = F(spread * rng.standard_normal() * 4)
    codes = rng.integers(0, 256, size=(n, M))
    if seed % 3 == 0:                                                     # exact duplicates: ties at the k-th score, inside and behind the sample
        codes[rng.integers(0, n, size=60)] = codes[0]
    if seed % 5 == 0:                                                     # a skewed code set: a few codes per sub-quantiser, many near-ties
        codes = codes % 3
    a, s, tau, tau2 = thresholds(T, dis0, codes, sample, k)
    assert np.isfinite(tau2) and tau2 >= tau, (tau, tau2)
    s_true_k = np.sort(s)[-k]
    need = s >= s_true_k
    assert (a[need] > tau2).all(), f"dropped {np.count_nonzero(a[need] <= tau2)} of the result's vectors (M {M} k {k} sample {sample})"
    assert (a[need] > tau).all()
