"""CPU model of the L2 IndexPQ staged scan's final candidate band (no GPU): are the inputs of tests/test_gpu_pq_l2.py fair?

The staged scan keeps, per query, every row whose 8-bit approximate score reaches a_k - 2 eps (a_k: the k-th best approximate score,
eps: the query's certified quantisation error).  A query whose candidate row overflows is re-run exactly, and the GPU test caps those
re-runs at 5 % of a batch — so the band of its inputs must sit far inside a candidate row BY THE REFERENCE ALONE, or the cap would
test the data and not the table builder.  This restates k_pq_lut8f's affine quantisation in numpy (per-m minimum as offset, one scale
per query from the largest range, eps = e_quant * 1.0001 + pq_round_slack(M) * B) on the oracle's codebooks and codes, with the table
T'[m][c] = -|q_m - cb[m][c]|^2 of an L2 IndexPQ, and counts the band.  Shape: the GPU test's staged index (d 64, M 16, n 300 000)."""
import numpy as np

SEED = 1234


def cand_row_cap(k, M):
    """api_search.hip cand_row_cap: keys a query's candidate row holds."""
    cap = 131072 if k > 512 else 65536 if k > 64 else 16384
    if 0 < M <= 32:
        cap = min(cap * 4, 262144)
    return cap


def quantise(T, M):
    """k_pq_lut8f, phases B and C and the parameters: T [M, 256] fp32 -> u8 table, scale, bias, eps."""
    f = np.float32
    mn, mx = T.min(axis=1), T.max(axis=1)
    maxrange = (mx - mn).max()
    scale = f(maxrange / f(255.0)) if maxrange > 0 else f(1.0)
    inv = f(1.0) / scale
    u = np.clip(np.rint((T - mn[:, None]) * inv), 0, 255).astype(f)
    err = np.abs(T - (mn[:, None] + scale * u)).max(axis=1)
    e_quant, bias = f(err.sum(dtype=np.float64)), f(mn.sum(dtype=np.float64))
    absmax_sum = np.maximum(np.abs(mn), np.abs(mx)).sum(dtype=np.float64)
    B = absmax_sum + abs(bias) + float(scale) * 255.0 * M + 1.0            # probe_dis0 = +0 for an IndexPQ
    slack = (3 * M + 12) * 5.9604645e-8 * 1.05
    eps = float(e_quant) * 1.0001 + slack * B
    return u.astype(np.int32), float(scale), float(bias), eps, float(e_quant)


def band_sizes(cb, codes, q32, ks, l2):
    M, _, dsub = cb.shape
    out = {k: [] for k in ks}
    for qv in q32:
        qs = qv.reshape(M, 1, dsub)
        T = (-((qs - cb) ** 2).sum(-1) if l2 else (qs * cb).sum(-1)).astype(np.float32)
        u, scale, bias, eps, _ = quantise(T, M)
        A = np.zeros(len(codes), np.int32)
        for m in range(M):
            A += u[m][codes[:, m]]
        a = bias + scale * A.astype(np.float64)
        for k in ks:
            a_k = np.partition(a, len(a) - k)[len(a) - k]
            out[k].append(int((a >= a_k - 2.0 * eps).sum()))
    return out


def test_l2_band_is_far_inside_a_candidate_row(orc):
    d, M, n, nq = 64, 16, 300_000, 64
    x = orc.synth_vectors(d, 256, 1234, 10000, 0.5, 0, n)
    q = orc.synth_queries(d, 256, 1234, 10000, 0.5, n, 999, 0.1, 0, nq)
    xt = orc.synth_vectors(d, 64, 1234, 10000, 0.5, 0, 4096).astype(np.float32)       # the GPU tests' training set (codebooks_for)
    cb = orc.pq_train(xt[orc.kmeans_sample(len(xt), 256, 256, SEED)], M, 25, SEED)
    codes = orc.pq_encode(cb, x.astype(np.float32))
    q32 = q.astype(np.float32)
    ks = (10, 1000)
    for name, l2 in (("IP", False), ("L2", True)):
        bands = band_sizes(cb, codes, q32, ks, l2)
        for k in ks:
            b = np.array(bands[k])
            print(f"{name} d={d} M={M} n={n} k={k}: band keys mean {b.mean():.0f} max {b.max()} (row capacity {cand_row_cap(k, M)})")
            assert b.min() >= k
            if l2:
                assert b.max() < cand_row_cap(k, M) // 4, f"k={k}: the largest L2 band {b.max()} is not under a quarter of the candidate row"
