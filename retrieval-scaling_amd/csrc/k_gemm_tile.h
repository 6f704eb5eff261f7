// k_gemm_tile.h — the operand loader the exact f32-input MFMA contractions share (k_gemm.hip: k_gemm_exact; k_vt.hip: k_vt_apply).
#pragma once
#include "rsx_internal.h"

namespace rsx {

typedef float floatx16 __attribute__((ext_vector_type(16)));

// 16 consecutive elements t0 .. t0 + 15 of row `row` of X (fp16 widened exactly, or fp32) -> out; elements at or past d read as +0.
// vec_ok: the row starts are 16-byte aligned, so a run that lies inside the row is fetched with 16-byte loads.
template <bool XF16>
__device__ inline void load16_f32(const void* X, int64_t row, int ldx, int t0, int d, bool vec_ok, float* out) {
    if (XF16) {
        const __half* p = (const __half*)X + row * ldx + t0;
        if (vec_ok && t0 + 16 <= d) {
            uint4 u0 = *reinterpret_cast<const uint4*>(p);
            uint4 u1 = *reinterpret_cast<const uint4*>(p + 8);
            const __half* h0 = reinterpret_cast<const __half*>(&u0);
            const __half* h1 = reinterpret_cast<const __half*>(&u1);
#pragma unroll
            for (int e = 0; e < 8; e++) { out[e] = __half2float(h0[e]); out[8 + e] = __half2float(h1[e]); }
        } else {
#pragma unroll
            for (int e = 0; e < 16; e++) out[e] = (t0 + e < d) ? __half2float(p[e]) : 0.0f;
        }
    } else {
        const float* p = (const float*)X + row * ldx + t0;
        if (vec_ok && t0 + 16 <= d) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float4 f = *reinterpret_cast<const float4*>(p + 4 * e);
                out[4 * e] = f.x; out[4 * e + 1] = f.y; out[4 * e + 2] = f.z; out[4 * e + 3] = f.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; e++) out[e] = (t0 + e < d) ? p[e] : 0.0f;
        }
    }
}

static inline int aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace rsx
