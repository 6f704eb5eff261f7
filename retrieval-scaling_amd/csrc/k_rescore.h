// k_rescore.h — the exact re-score of stored rows and the (score desc, id asc) sort of a candidate set in LDS, shared by k_finalize
// (k_select.hip: candidates of a Flat / IVF-Flat scan) and k_refine (k_refine.hip: candidates named by label, rsx_refine), and k_refine's
// launch interface (api_refine.hip); the pieces of the canonical IVF-PQ score (code bytes of a 16-sub-quantiser run in m order, one table
// entry by the table builder's chain) that k_finalize and the threshold pre-pass's anchor rows (k_pq_rot.hip: k_pq_prepass4) both use.
#pragma once
#include "rsx_internal.h"

namespace rsx {

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The 16-byte piece of a 16-sub-quantiser run (pq_piece_ptrs, rsx_internal.h) rotated left by i = row & 15 bytes: the codes in m order.
__device__ inline void rot16_bytes(uint32_t (&w)[4], int i) {     // byte t of the result = byte (t - i) & 15 of the input
    const int wi = i >> 2, bi = i & 3;
    if (wi & 1) { const uint32_t t = w[3]; w[3] = w[2]; w[2] = w[1]; w[1] = w[0]; w[0] = t; }
    if (wi & 2) { uint32_t t = w[0]; w[0] = w[2]; w[2] = t; t = w[1]; w[1] = w[3]; w[3] = t; }
    if (bi) {
        const int l = 8 * bi, r = 32 - l;
        const uint32_t r0 = (w[0] << l) | (w[3] >> r), r1 = (w[1] << l) | (w[0] >> r), r2 = (w[2] << l) | (w[1] >> r), r3 = (w[3] << l) | (w[2] >> r);
        w[0] = r0; w[1] = r1; w[2] = r2; w[3] = r3;
    }
}
// Inner-product table entry of one (sub-quantiser, code): <qs, cw> by the table builder's fmaf chain from +0 (k_pq_lut / k_pq_lut8f), hence
// the same bits; the canonical IVF-PQ score is dis0 + the sum of a vector's M entries added in m order.
__device__ __forceinline__ float pq_ip_entry(const float* qs, const float* cw, int dsub) {
    float t = 0.0f;
    if (dsub == 8) {
        const float4 x = ((const float4*)cw)[0], y = ((const float4*)cw)[1];
        t = __fmaf_rn(qs[0], x.x, t); t = __fmaf_rn(qs[1], x.y, t); t = __fmaf_rn(qs[2], x.z, t); t = __fmaf_rn(qs[3], x.w, t);
        t = __fmaf_rn(qs[4], y.x, t); t = __fmaf_rn(qs[5], y.y, t); t = __fmaf_rn(qs[6], y.z, t); t = __fmaf_rn(qs[7], y.w, t);
    } else {
        for (int tt = 0; tt < dsub; tt++) t = __fmaf_rn(qs[tt], cw[tt], t);
    }
    return t;
}

// Candidates c of [c_lo, c_hi) whose storage row srow[c] lies in [0, nrows) get sord[c] = the order word of their exact score against the
// query qv: fp64 accumulation of exact products, rounded once to fp32 (the oracle's canonical Flat arithmetic); inner product: the score,
// L2: 0 - squared distance.  Any other srow[c] is never dereferenced and its sord[c] stays as it is.
// One wave per candidate, lanes over the dimensions; FOUR candidates per wave in flight (round 4: at the reference's n_docs =
// 1000 a query re-scores 2048 rows of 1.5 KB that sit anywhere in HBM — one row at a time per wave was 3.2 ms per 1024 queries).
// Ends with a workgroup barrier: every thread of the workgroup calls it.
__device__ __forceinline__ void rescore_rows(const void* X, int x_f16, int ld, int d, int metric, const float* qv, int ldq, int64_t nrows,
                                             const int64_t* srow, uint32_t* sord, int c_lo, int c_hi, int lane, int wv, int nwv) {
    for (int c0 = c_lo + 4 * wv; c0 < c_hi; c0 += 4 * nwv) {
        int64_t rows[4]; double acc[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {   // wave-uniform (LDS values)
            const int64_t r = c0 + u < c_hi ? srow[c0 + u] : -1;
            rows[u] = (uint64_t)r < (uint64_t)nrows ? r : -1; acc[u] = 0.0;
        }
        if (x_f16 && (ldq & 7) == 0 && ldq >= ld) {
            // fp16 rows: 16 bytes (8 values) per lane and load — a 1536-byte row is 1.5 wave loads instead of 12 two-byte ones (the
            // rows' zero padding up to ld contributes exact zeros; fp64 sums of products of fp16-valued numbers do not depend on the order)
            for (int c8 = lane; c8 < (ld >> 3); c8 += 64) {
                const float4 qa = *reinterpret_cast<const float4*>(qv + 8 * c8), qb = *reinterpret_cast<const float4*>(qv + 8 * c8 + 4);
                const float qf[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
                uint4 xr[4];
#pragma unroll
                for (int u = 0; u < 4; u++) xr[u] = rows[u] >= 0 ? *reinterpret_cast<const uint4*>((const __half*)X + rows[u] * ld + 8 * c8) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t wds[4] = {xr[u].x, xr[u].y, xr[u].z, xr[u].w};
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const __half hx = __ushort_as_half((unsigned short)((wds[e >> 1] >> (16 * (e & 1))) & 0xffffu));
                        const double qd = (double)qf[e], xd = (double)__half2float(hx);
                        if (metric == 0) acc[u] += qd * xd; else { const double df = qd - xd; acc[u] += df * df; }
                    }
                }
            }
        } else
        for (int t = lane; t < d; t += 64) {
            const double qd = (double)qv[t];
            double xd[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                xd[u] = 0.0;
                if (rows[u] >= 0) xd[u] = x_f16 ? (double)__half2float(((const __half*)X)[rows[u] * ld + t]) : (double)((const float*)X)[rows[u] * ld + t];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) { if (metric == 0) acc[u] += qd * xd[u]; else { const double df = qd - xd[u]; acc[u] += df * df; } }
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

// Orders the KP candidates (sord[c], sid[c]) in LDS by (ord desc, id asc); invalid entries (ord 0, id INT64_MAX) sink to the end.
// rank_sort: by counting — a candidate's position is the number of candidates that beat it (every thread walks the same LDS words —
// broadcasts — and there are two barriers instead of the 28 of a 128-key bitonic network); any KP, and sord2[KP] / sid2[KP] hold the second
// copy.  Otherwise a bitonic network: KP a power of two, sord2 / sid2 unused.  Every thread of the workgroup calls it.
__device__ __forceinline__ void sort_candidates(uint32_t* sord, int64_t* sid, int KP, int rank_sort, uint32_t* sord2, int64_t* sid2, int tid, int nt) {
    if (rank_sort) {
        for (int c = tid; c < KP; c += nt) {
            const uint32_t oi = sord[c];
            const int64_t ii = sid[c];
            int rank = 0;
            for (int j = 0; j < KP; j++) {
                const uint32_t oj = sord[j];
                const int64_t ij = sid[j];
                rank += ((oj > oi) || (oj == oi && (ij < ii || (ij == ii && j < c)))) ? 1 : 0;
            }
            sord2[rank] = oi; sid2[rank] = ii;
        }
        __syncthreads();
        for (int c = tid; c < KP; c += nt) { sord[c] = sord2[c]; sid[c] = sid2[c]; }
        __syncthreads();
    } else
    for (int size = 2; size <= KP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (KP >> 1); t += nt) {
                int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                int j = i + stride;
                bool desc = ((i & size) == 0);
                uint32_t oi = sord[i], oj = sord[j];
                int64_t ii = sid[i], ij = sid[j];
                bool i_worse = (oi < oj) || (oi == oj && ii > ij);
                if (i_worse == desc) {
                    sord[i] = oj; sord[j] = oi; sid[i] = ij; sid[j] = ii;
                }
            }
            __syncthreads();
        }
    }
}

// rsx_refine (k_refine.hip): the kc candidate LABELS of every query re-scored exactly against a Flat row store (k_finalize's re-score
// arithmetic, k_rescore.h), ordered by (score desc / distance asc, label asc), the best k emitted; labels outside [0, ntotal) are
// skipped (never dereferenced), a label >= ntotal additionally sets *flag.  kc <= 4096, 1 <= k <= kc.
#define REFINE_RANK_MAX 512        // up to here the candidates are ordered by counting (as k_finalize's FIN_RANK_MAX in k_select.hip), past it by the bitonic network
struct RefineArgs {
    int metric; int64_t nq; int kc; int k;
    const int64_t* labels;                  // [nq, kc], device memory
    const float* Q32; int ldq; int d;       // fp32 queries, rows of ldq >= ld values, zero padded
    const void* X; int x_f16; int ld; int64_t ntotal;
    float* D; int64_t* I;                   // [nq, k]
    int* flag;                              // host-visible word
    int KP; int rank_sort;                  // set by launch_refine: sort slots (kc, or its power of two for the network) and the sort's form
};
void launch_refine(const RefineArgs& a, hipStream_t st);

}  // namespace rsx
