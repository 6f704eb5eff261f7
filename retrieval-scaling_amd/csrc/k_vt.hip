// k_vt.hip — the dense contraction of the vector transforms (faiss.LinearTransform::apply / transform_transpose).
//
//  k_vt_apply : Y[n, nc] = X'[n, d] · Cᵀ (+ badd), row-major fp32 out, on the f32-input MFMA (v_mfma_f32_32x32x2_f32) exactly as
//               k_gemm_exact runs it (k_gemm.hip: 128 x 128 tile, four waves of 64 x 64, K steps of 32 through padded LDS, the next
//               step's operands fetched while the current one is multiplied).  On gfx950 that instruction is bit for bit a k-ordered
//               fp32 fmaf chain, so
//                   y_j = fp32( s_j + badd_j ),   s_j = fmaf(x'[t], C[j][t], s) for t = 0 .. d - 1 from +0,
//               the sum with the bias rounded once (__fadd_rn: no contraction), no bias = no add.
//               X' = X widened exactly (fp16) or as it is (fp32); with SUB, x'[t] = fp32(x[t] - bsub[t]) while the operand is loaded
//               (__fsub_rn).  Forward transform: C = A [d_out, d_in], badd = b.  Reverse transform of an orthonormal A: C = Aᵀ
//               [d_in, d_out] (the transposed device copy), bsub = b — the chain then runs over j = 0 .. d_out - 1.
//               What differs from k_gemm_exact is the operand hook (SUB) and the epilogue (bias, rows of nc floats, no score-row stride
//               and no arg-max); the tile loop is restated here so that k_gemm_exact's code stays what its callers were measured with.
#include "rsx_internal.h"
#include "k_gemm_tile.h"

namespace rsx {

template <bool XF16, bool SUB>
__device__ inline void vt_load16(const void* X, int64_t row, int ldx, int t0, int d, bool vec_ok, const float* bsub, float* out) {
    load16_f32<XF16>(X, row, ldx, t0, d, vec_ok, out);
    if (SUB) {
#pragma unroll
        for (int e = 0; e < 16; e++)
            if (t0 + e < d) out[e] = __fsub_rn(out[e], bsub[t0 + e]);      // (the K padding past d stays +0)
    }
}

template <bool XF16, bool SUB>
__global__ __launch_bounds__(256) void k_vt_apply(const void* X, int64_t n, int ldx, int x_vec_ok, const float* bsub, const float* C,
                                                  int nc, int d, int c_vec_ok, const float* badd, float* Y) {
    __shared__ float As[128][33];
    __shared__ float Bs[128][33];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1;
    const int64_t row0 = (int64_t)blockIdx.y * 128;
    const int col0 = blockIdx.x * 128;

    floatx16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;

    // staging: thread (sr, sh) owns 16 of the 32 K values of tile row sr of both operands; rows past the end re-read the last one
    const int sr = tid >> 1, sh = tid & 1;
    int64_t xr = row0 + sr; if (xr > n - 1) xr = n - 1;
    int cr = col0 + sr; if (cr > nc - 1) cr = nc - 1;

    float xa[16], cb[16];
    vt_load16<XF16, SUB>(X, xr, ldx, 16 * sh, d, x_vec_ok, bsub, xa);
    load16_f32<false>(C, cr, d, 16 * sh, d, c_vec_ok, cb);

    for (int k0 = 0; k0 < d; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; e++) { As[sr][16 * sh + e] = xa[e]; Bs[sr][16 * sh + e] = cb[e]; }
        __syncthreads();
        if (k0 + 32 < d) {
            vt_load16<XF16, SUB>(X, xr, ldx, k0 + 32 + 16 * sh, d, x_vec_ok, bsub, xa);
            load16_f32<false>(C, cr, d, k0 + 32 + 16 * sh, d, c_vec_ok, cb);
        }
        const int li = lane & 31, lk = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            const int kc = 2 * kk + lk;
            float a0 = As[wr * 64 + li][kc], a1 = As[wr * 64 + 32 + li][kc];
            float b0 = Bs[wc * 64 + li][kc], b1 = Bs[wc * 64 + 32 + li][kc];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }

    // C/D layout of the 32x32 MFMA: reg r of lane l holds (row i = (r&3) + 8*(r>>2) + 4*(l>>5), col j = l&31): a wave stores runs of 32 floats
    const int lj = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int tj = 0; tj < 2; tj++) {
        const int col = col0 + wc * 64 + tj * 32 + lj;
        if (col >= nc) continue;
        const float bj = badd ? badd[col] : 0.0f;
#pragma unroll
        for (int ti = 0; ti < 2; ti++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int64_t row = row0 + wr * 64 + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (row < n) Y[row * nc + col] = badd ? __fadd_rn(acc[ti][tj][r], bj) : acc[ti][tj][r];
            }
    }
}

void launch_vt_apply(const void* X, int x_f16, int64_t n, int d, const float* bsub, const float* C, int nc, const float* badd, float* Y,
                     hipStream_t st) {
    if (n <= 0 || nc <= 0 || d <= 0) return;
    const int64_t rows_per_launch = 65535ll * 128;      // grid.y is limited to 65535 row tiles per launch
    const int xv = aligned16(X) && (d % 8 == 0);
    const int cv = aligned16(C) && (d % 4 == 0);
    const size_t esz = x_f16 ? 2 : 4;
    for (int64_t r0 = 0; r0 < n; r0 += rows_per_launch) {
        const int64_t nr = n - r0 < rows_per_launch ? n - r0 : rows_per_launch;
        dim3 grid((unsigned)((nc + 127) / 128), (unsigned)((nr + 127) / 128));
        const void* Xp = (const char*)X + (size_t)r0 * d * esz;
        float* Yp = Y + r0 * nc;
        if (bsub) {
            if (x_f16) hipLaunchKernelGGL((k_vt_apply<true, true>), grid, dim3(256), 0, st, Xp, nr, d, xv, bsub, C, nc, d, cv, badd, Yp);
            else hipLaunchKernelGGL((k_vt_apply<false, true>), grid, dim3(256), 0, st, Xp, nr, d, xv, bsub, C, nc, d, cv, badd, Yp);
        } else {
            if (x_f16) hipLaunchKernelGGL((k_vt_apply<true, false>), grid, dim3(256), 0, st, Xp, nr, d, xv, bsub, C, nc, d, cv, badd, Yp);
            else hipLaunchKernelGGL((k_vt_apply<false, false>), grid, dim3(256), 0, st, Xp, nr, d, xv, bsub, C, nc, d, cv, badd, Yp);
        }
    }
}

// At[t][j] = A[j][t]: the reverse transform's operand, made once when the matrix is set
__global__ void k_vt_transpose(const float* A, int rows, int cols, float* At) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * cols) return;
    const int t = (int)(i / rows), j = (int)(i - (int64_t)t * rows);
    At[i] = A[(int64_t)j * cols + t];
}
void launch_vt_transpose(const float* A, int rows, int cols, float* At, hipStream_t st) {
    const int64_t tot = (int64_t)rows * cols;
    if (tot <= 0) return;
    hipLaunchKernelGGL(k_vt_transpose, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, A, rows, cols, At);
}

}  // namespace rsx
