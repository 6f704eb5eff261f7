// k_sq.h — the QT_8bit scalar quantiser's arithmetic as device functions, and the decode row loader of the exact
// re-score: what rescore_rows (k_rescore.h) does for stored fp16 / fp32 rows, for rows of code bytes.  Shared by k_sq.hip (encode,
// norms, exact scores) and k_finalize (k_select.hip).
#pragma once
#include "k_rescore.h"

namespace rsx {

// fp32, every operation rounded once: the numpy restatement's bits.  hipcc contracts a * b + c into one fma by default — also across the
// __fmul_rn / __fadd_rn intrinsics, which are plain operators compiled in the header's own (contracting) context — so these functions use
// the operators themselves with contraction switched off (the instructions keep that through inlining).
__device__ __forceinline__ uint32_t sq_encode(float y, float vmin, float vdiff) {
#pragma clang fp contract(off)
    float t = vdiff != 0.0f ? ((y - vmin) / vdiff) : 0.0f;
    t = t > 0.0f ? t : 0.0f;
    t = t < 1.0f ? t : 1.0f;
    return (uint32_t)(int)(255.0f * t);
}
__device__ __forceinline__ float sq_decode(uint32_t code, float vmin, float vdiff) {
#pragma clang fp contract(off)
    const float t = ((float)code + 0.5f) / 255.0f;
    return vmin + vdiff * t;
}
// the stored vector's dimension t: the decoded value, plus the list's centroid (by_residual; cen = that centroid's row or null)
__device__ __forceinline__ float sq_xhat(uint32_t code, const float* trained, const float* cen, int d, int t) {
#pragma clang fp contract(off)
    const float r = sq_decode(code, trained[t], trained[d + t]);
    return cen ? (cen[t] + r) : r;
}
// the list that owns storage row `row`: the largest l with list_base[l] <= row (lists without capacity share their successor's base)
__device__ __forceinline__ int sq_list_of_row(const SqRows& s, int64_t row) {
    int lo = 0, hi = s.nlist;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s.list_base[mid] <= row) lo = mid; else hi = mid; }
    return lo;
}
// one lane's share (4 consecutive dimensions from t4, a 4-byte word of the row) of the fp64 sum of a decoded row against the query
__device__ __forceinline__ double sq_dot4(uint32_t w, const float* trained, const float* cen, const float* qv, int d, int t4, int metric) {
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int t = t4 + e;
        if (t < d) {
            const double xd = (double)sq_xhat((w >> (8 * e)) & 255u, trained, cen, d, t), qd = (double)qv[t];
            if (metric == 0) acc += qd * xd; else { const double df = qd - xd; acc += df * df; }
        }
    }
    return acc;
}

// rescore_rows for code rows: candidates c of [c_lo, c_hi) with a storage row srow[c] >= 0 get sord[c] = the order word of the canonical
// score of the query against the DECODED row (fp64 accumulation of exact products, rounded once; L2: 0 - squared distance).  One wave
// per candidate, four in flight, a 4-byte word of the row per lane and load.  Ends with a workgroup barrier.
__device__ __forceinline__ void rescore_rows_sq(const SqRows& s, int ld, int d, int metric, const float* qv, const int64_t* srow, uint32_t* sord,
                                                int c_lo, int c_hi, int lane, int wv, int nwv) {
    for (int c0 = c_lo + 4 * wv; c0 < c_hi; c0 += 4 * nwv) {
        int64_t rows[4]; double acc[4]; const float* cen[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {   // wave-uniform (LDS values)
            const int64_t r = c0 + u < c_hi ? srow[c0 + u] : -1;
            rows[u] = r >= 0 ? r : -1; acc[u] = 0.0;
            cen[u] = (r >= 0 && s.centroids) ? s.centroids + (int64_t)sq_list_of_row(s, r) * d : nullptr;
        }
        for (int t4 = 4 * lane; t4 < d; t4 += 256) {
            uint32_t w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) w[u] = rows[u] >= 0 ? *reinterpret_cast<const uint32_t*>(s.codes + rows[u] * ld + t4) : 0u;
#pragma unroll
            for (int u = 0; u < 4; u++) if (rows[u] >= 0) acc[u] += sq_dot4(w[u], s.trained, cen[u], qv, d, t4, metric);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (rows[u] < 0) continue;
            const double sacc = wave_sum_f64(acc[u]);
            if (lane == 0) {
                const float sc = (float)sacc;
                sord[c0 + u] = f2ord((metric == 0 ? sc : 0.0f - sc) + 0.0f);
            }
        }
    }
    __syncthreads();
}

}  // namespace rsx
