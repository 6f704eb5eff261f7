// rsx_sqflat.h — the int8 matrix-core scan of IndexScalarQuantizer (RSX_KIND_SQ, rsx_index::flat_sq): what k_sq_gemm.hip
// (kernels, launchers) and api_sqflat.hip (the staged driver) share.
#pragma once
#include "rsx_internal.h"

namespace rsx {

// The query planes.  q'_j = fl(fl(q_j vdiff_j) / 255) as k_sq_query_factors defines it; w_j = rint(fl(q'_j s)) with one scale
// s = fl(wmax / max_j |q'_j|) per query, |w_j| <= wmax; w_j = 128 h_j + l_j with l_j in [-64, 63] and h_j in [-127, 127], both int8.
// The scan's sum over a row is A = sum_j w_j (code_j - 128) = 128 A_h + A_l, exact in i32.  wmax is the bit budget of the i32 sum:
//   |w_j| <= 127 * 128 + 63 = 16319 (the planes), and (wmax + 64) * 128 * d < 2^31 (|128 A_h| <= sum_j (|w_j| + 64) 128, |A| <= wmax 128 d)
// so d <= 1023 has the full 14 bits and longer rows fewer (d = 1100: 15188, d = 2048: 8127).  tests/sqflat_ref.py restates both.
inline int sqflat_wmax(int d) {
    const int64_t by_sum = (((int64_t)1 << 31) - 1) / ((int64_t)128 * d) - 64;
    return (int)(by_sum < 16319 ? by_sum : 16319);
}

// planes [nq_pad / 128][2][128][ldp] int8 (query tile, plane h then l, query of the tile, dimension; rows >= nq and dimensions >= d zero;
// ldp = ld rounded up to 128: a K step of the scan is 128 bytes), qs [nq_pad, 2] = {fl(1 / s), qc}, qc = k_sq_query_factors' constant;
// *rho_bits (zeroed by the caller): the float bits of max over the batch of 1.000001 max_j |q'_j| / |q| — 1 / s <= (1 + 2^-23) rho |q| / wmax for
// every query of the batch, the scale of the certificate's half-unit term (a few times smaller than the worst case max_j vdiff_j / 255)
void launch_sqflat_planes(const float* Q32, int ldq, int64_t nq, int64_t nq_pad, int d, int ldp, const float* trained, int wmax, int8_t* planes,
                          float* qs, unsigned int* rho_bits, hipStream_t st);

// k_sq_gemm over the code rows [v0, v0 + nv) of `codes` (rows of ld bytes): score of (query q, row r) = fl(fl(fl(A) qs[2 q]) + qs[2 q + 1]) (+ bias[r]).
//   scores: temp[q * tstride + (r - v0)] for q < nq_pad
void launch_sqflat_gemm(const int8_t* planes, const float* qs, int nq_pad, int ldp, const uint8_t* codes, int64_t v0, int64_t nv, int ld,
                        const float* bias, float* temp, int64_t tstride, hipStream_t st);
//   filter: the keys make_key(score, r) that beat tau[q * tau_stride] go to cand[q][0 .. cap), counted in cand_cnt[q * CCS]
void launch_sqflat_gemm_filter(const int8_t* planes, const float* qs, int nq_pad, int nq, int ldp, const uint8_t* codes, int64_t v0, int64_t nv,
                               int ld, const float* bias, const uint64_t* tau, int64_t tau_stride, uint64_t* cand, unsigned long long* cand_cnt,
                               int cand_cap, hipStream_t st);

}  // namespace rsx
