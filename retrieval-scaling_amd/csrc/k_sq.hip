// k_sq.hip — IVF scalar quantiser (QT_8bit, KIND_IVFSQ): training reduction, encoder, per-batch query factors, the
// list-major MFMA scan over rows of code bytes and the exact scores of the re-run.  The arithmetic of a code is in k_sq.h.
#include "k_sq.h"

#include <algorithm>

// every fp32 operation of this file is rounded on its own (the encoder's and the query factors' arithmetic is specified that way; the
// fp64 sums are of exact products either way)
#pragma clang fp contract(off)

namespace rsx {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------
// training: per-dimension min / max over all rows (order words: unsigned min / max = float min / max)
// ---------------------------------------------------------------------------------------
__global__ void k_sq_minmax_init(uint32_t* mnmx, int d) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < d) { mnmx[t] = 0xFFFFFFFFu; mnmx[d + t] = 0u; }
}
#define SQ_MM_ROWS 256
__global__ __launch_bounds__(256) void k_sq_minmax(const float* x, int64_t n, int d, const float* centroids, const int32_t* assign, uint32_t* mnmx) {
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= d) return;
    const int64_t r0 = (int64_t)blockIdx.x * SQ_MM_ROWS;
    const int64_t r1 = r0 + SQ_MM_ROWS < n ? r0 + SQ_MM_ROWS : n;
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
    for (int64_t r = r0; r < r1; r++) {
        float y = x[r * d + t];
        if (centroids) y = (y - centroids[(int64_t)assign[r] * d + t]);
        const uint32_t o = f2ord(y);
        mn = o < mn ? o : mn; mx = o > mx ? o : mx;
    }
    if (r1 > r0) { atomicMin(&mnmx[t], mn); atomicMax(&mnmx[d + t], mx); }
}
void launch_sq_minmax(const float* x, int64_t n, int d, const float* centroids, const int32_t* assign, uint32_t* mnmx, hipStream_t st) {
    hipLaunchKernelGGL(k_sq_minmax_init, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, mnmx, d);
    if (n <= 0) return;
    hipLaunchKernelGGL(k_sq_minmax, dim3((unsigned)((n + SQ_MM_ROWS - 1) / SQ_MM_ROWS), (unsigned)((d + 255) / 256)), dim3(256), 0, st, x, n, d,
                       centroids, assign, mnmx);
}

// ---------------------------------------------------------------------------------------
// encoder: one wave per row, lanes over the dimensions.  The norm term is that of the row the re-score will decode: the fp64 sum of
// the decoded values' squares (lane t accumulates dimensions t, t + 64, ...; wave_sum_f64), rounded once — k_sq_norms repeats it
// term for term for imported codes.
// ---------------------------------------------------------------------------------------
// bsum: the lane's share of sum_j (code_j - 128)^2 — the scan multiplies the CENTRED codes, and the largest such norm over the stored rows
// is a term of its certificate (maxnorm_bits[1]; [0] = the largest |x^|^2 as float bits)
__device__ __forceinline__ void sq_store_norm(double acc, unsigned int bsum, int lane, float* norm_out, unsigned int* maxnorm_bits) {
    acc = wave_sum_f64(acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bsum += __shfl_xor(bsum, off);
    if (lane == 0) {
        const float n2 = (float)acc;
        if (norm_out) *norm_out = n2;
        if (maxnorm_bits) { atomicMax(maxnorm_bits, __float_as_uint(n2)); atomicMax(maxnorm_bits + 1, bsum); }     // n2 >= 0: the bit patterns order like the values
    }
}
template <bool XF16>
__global__ __launch_bounds__(256) void k_sq_encode(const void* x, int64_t n, int d, int ld, const float* trained, const float* centroids,
                                                   const int32_t* assign, const int64_t* dest_row, uint8_t* codes, float* norms,
                                                   unsigned int* maxnorm_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t row = dest_row[i];
    if (row < 0) return;                      // a vector another list shard owns
    const float* cen = centroids ? centroids + (int64_t)assign[i] * d : nullptr;
    uint8_t* out = codes + row * ld;
    double acc = 0.0; unsigned int bsum = 0;
    for (int t = lane; t < ld; t += 64) {
        uint32_t code = 0;
        if (t < d) {
            float y = XF16 ? __half2float(reinterpret_cast<const __half*>(x)[i * d + t]) : reinterpret_cast<const float*>(x)[i * d + t];
            if (cen) y = (y - cen[t]);
            code = sq_encode(y, trained[t], trained[d + t]);
            const double xh = (double)sq_xhat(code, trained, cen, d, t);
            acc += xh * xh;
            const int b = (int)code - 128; bsum += (unsigned int)(b * b);
        }
        out[t] = (uint8_t)code;
    }
    sq_store_norm(acc, bsum, lane, norms ? norms + row : nullptr, maxnorm_bits);
}
void launch_sq_encode(const void* x, int x_f16, int64_t n, int d, int ld, const float* trained, const float* centroids, const int32_t* assign,
                      const int64_t* dest_row, uint8_t* codes, float* norms, unsigned int* maxnorm_bits, hipStream_t st) {
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 3) / 4));
    if (x_f16) hipLaunchKernelGGL(k_sq_encode<true>, grid, dim3(256), 0, st, x, n, d, ld, trained, centroids, assign, dest_row, codes, norms, maxnorm_bits);
    else hipLaunchKernelGGL(k_sq_encode<false>, grid, dim3(256), 0, st, x, n, d, ld, trained, centroids, assign, dest_row, codes, norms, maxnorm_bits);
}
__global__ __launch_bounds__(256) void k_sq_norms(const uint8_t* codes, int64_t row0, int64_t n, int d, int ld, const float* trained,
                                                  const float* centroid, float* norms, unsigned int* maxnorm_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint8_t* in = codes + (row0 + i) * ld;
    double acc = 0.0; unsigned int bsum = 0;
    for (int t = lane; t < d; t += 64) {
        const double xh = (double)sq_xhat(in[t], trained, centroid, d, t);
        acc += xh * xh;
        const int b = (int)in[t] - 128; bsum += (unsigned int)(b * b);
    }
    sq_store_norm(acc, bsum, lane, norms ? norms + row0 + i : nullptr, maxnorm_bits);
}
void launch_sq_norms(const uint8_t* codes, int64_t row0, int64_t n, int d, int ld, const float* trained, const float* centroid, float* norms,
                     unsigned int* maxnorm_bits, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_sq_norms, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, codes, row0, n, d, ld, trained, centroid, norms, maxnorm_bits);
}

// ---------------------------------------------------------------------------------------
// per-batch query factors.  <q, x^> = sum_j q_j vmin_j + sum_j q'_j (code_j + 0.5), q'_j = q_j vdiff_j / 255.  The scan multiplies the
// CENTRED codes b_j = code_j - 128 (exact in fp16; a third of the magnitude the raw bytes would put through the fp32 accumulator, and
// with it of the certificate's rounding term) with q' on the fp16 matrix cores, so q' is what gets rounded: it is scaled by a power of two s so that its
// largest element lies in [2^13, 2^14) (typical q' of 1e-5 would be fp16 subnormals), then split into hi = fp16(q' s) and
// lo = fp16(q' s - hi): |q' s - hi - lo| <= 2^-22 |q' s| unless lo falls below the fp16 normal range (error <= 2^-14 then, whatever the
// denormal mode) — the error terms finalize_args (api_search.hip) accounts for.  qc[q] = {1 / s, sum_j q_j vmin_j + 128.5 sum_j q'_j}.
// The exponent of s is clamped to +-100 (s and 1 / s stay normal floats): for a degenerate query whose largest |q'_j| lies below about
// 2^-86 the scaled factors no longer reach [2^13, 2^14) and the bound's sub-normal term is not covered — such a query's factors are
// below 1e-25 of any stored value's scale; it is NOT flagged for the exact re-run.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sq_query_factors(const float* Q32, int ldq, int d, int ld, const float* trained, __half* qhi, __half* qlo,
                                                          float* qc) {
    __shared__ double s_sum[4];
    __shared__ float s_max[4];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* qv = Q32 + q * ldq;
    double sum = 0.0; float mx = 0.0f;
    for (int t = tid; t < d; t += 256) {
        const float qp = ((qv[t] * trained[d + t]) / 255.0f);
        sum += (double)qv[t] * (double)trained[t] + 128.5 * (double)qp;
        mx = fmaxf(mx, fabsf(qp));
    }
    sum = wave_sum_f64(sum);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) { s_sum[wv] = sum; s_max[wv] = mx; }
    __syncthreads();
    sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    mx = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    float sc = 1.0f;
    if (mx > 0.0f && mx < __builtin_inff()) {
        int ex; (void)frexpf(mx, &ex);                  // mx = m 2^ex, m in [0.5, 1)
        int e = 14 - ex; e = e > 100 ? 100 : e; e = e < -100 ? -100 : e;
        sc = ldexpf(1.0f, e);
    }
    if (tid == 0) { qc[2 * q] = 1.0f / sc; qc[2 * q + 1] = (float)sum; }
    for (int t = tid; t < ld; t += 256) {
        __half hi = __float2half_rn(0.0f), lo = hi;
        if (t < d) {
            const float v = (((qv[t] * trained[d + t]) / 255.0f) * sc);
            hi = __float2half_rn(v);
            lo = __float2half_rn((v - __half2float(hi)));
        }
        qhi[q * ld + t] = hi; qlo[q * ld + t] = lo;
    }
}
void launch_sq_query_factors(const float* Q32, int ldq, int64_t nq, int64_t nq_pad, int d, int ld, const float* trained, __half* qhi, __half* qlo,
                             float* qc, hipStream_t st) {
    (void)nq_pad;
    if (nq <= 0) return;
    hipLaunchKernelGGL(k_sq_query_factors, dim3((unsigned)nq), dim3(256), 0, st, Q32, ldq, d, ld, trained, qhi, qlo, qc);
}

// ---------------------------------------------------------------------------------------
// k_sq_list_scan: the list-major MFMA scan over rows of code bytes.  Work items, grouping, score rows and the filtered epilogue are
// k_list_scan2's (k_gemm.hip); what differs is the operand path:
//   * a lane fetches 16 code bytes of its row per K step of 64 dimensions (a wave: 16 rows x 64 contiguous bytes; two steps = whole
//     128-byte lines), SQ_U steps ahead of the MFMAs in registers, across the 16-row blocks of its chunk;
//   * bytes become fp16 in registers: v_perm_b32 pairs each byte with 0x64 (fp16 1024 + code, exact), a packed subtract of 1152 leaves
//     the centred code b = code - 128 (exact) — the 1024 is NOT folded into the constant: it would put 1024 sum |q'| through the fp32
//     accumulator and with it many times the rounding error into the certificate;
//   * the K order inside a step is permuted (MFMA 0 takes bytes 0-7 of every lane's 16, MFMA 1 bytes 8-15); the query fragments are
//     read from LDS in the same order;
//   * per K step and 16-query tile FOUR MFMAs: hi and lo halves of q' against both byte groups;
//   * the group's query halves for a slice of `kc` dimensions sit in LDS ((kc + 8) fp16 per row: conflict-free 16-byte reads); rows
//     longer than kc are scanned slice after slice with the accumulators kept — 64 KiB hold 16 queries x 1024 dimensions or 64 x 256, so
//     two workgroups share a CU in both forms.
// QT = 16-query tiles per group (1: four waves, 512 rows per work item; 4: eight waves, 1024 rows).
// ---------------------------------------------------------------------------------------
#define SQ_NB 8             // 16-row blocks per wave per work item
#define SQ_U 4              // K steps a wave keeps in flight

__device__ __forceinline__ void sq_widen16(const uint4& c, half8& x0, half8& x1) {
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
    const half2v off = {(_Float16)1152.0f, (_Float16)1152.0f};      // 1024 (the perm's exponent byte) + 128 (centring)
    union { uint32_t u; half2v h; } p[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        p[2 * i].u = __builtin_amdgcn_perm(0x64646464u, w[i], 0x04010400u);         // {1024 + byte 0, 1024 + byte 1}
        p[2 * i + 1].u = __builtin_amdgcn_perm(0x64646464u, w[i], 0x04030402u);     // {1024 + byte 2, 1024 + byte 3}
    }
#pragma unroll
    for (int i = 0; i < 8; i++) p[i].h = p[i].h - off;
    x0 = half8{p[0].h[0], p[0].h[1], p[1].h[0], p[1].h[1], p[2].h[0], p[2].h[1], p[3].h[0], p[3].h[1]};
    x1 = half8{p[4].h[0], p[4].h[1], p[5].h[0], p[5].h[1], p[6].h[0], p[6].h[1], p[7].h[0], p[7].h[1]};
}

template <bool FILTER, int QT, int NW>
__global__ __launch_bounds__(64 * NW) void k_sq_list_scan(ListScanArgs a, int kc) {
    constexpr int NQG = 16 * QT;
    constexpr int NT = 64 * NW;
    constexpr int BR = 16 * NW;                  // rows between a wave's consecutive blocks
    extern __shared__ __attribute__((aligned(16))) unsigned char sq_smem[];
    const int qstride = (kc + 8) * 2;            // bytes
    unsigned char* Qh = sq_smem;
    unsigned char* Ql = sq_smem + NQG * qstride;
    int64_t* segoff = reinterpret_cast<int64_t*>(sq_smem + 2 * NQG * qstride);      // [NQG] score-row offset | (FILTER) column in the query's row
    int64_t* sq = segoff + NQG;                                                     // [NQG] query
    uint64_t* stau = reinterpret_cast<uint64_t*>(sq + NQG);                         // [NQG] threshold key (FILTER)
    float* sinv = reinterpret_cast<float*>(stau + NQG);                             // [NQG] 1 / scale
    float* scst = sinv + NQG;                                                       // [NQG] constant (+ <q, c_l>)
    int32_t* sqn = reinterpret_cast<int32_t*>(scst + NQG);                          // [NQG] query number or -1
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int g = blockIdx.x;
    int chunk = blockIdx.y;
    int l, gi;
    if (a.item_off) {
        if (!pq_decode_item(a.item_off, a.group_off, *a.total_items, a.nlist, l, gi, chunk)) return;
        g = a.group_off[l] + gi;
    } else {
        if (g >= *a.total_groups) return;
        int lo = 0, hi = a.nlist;  // largest l with group_off[l] <= g
        while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (a.group_off[mid] <= g) lo = mid; else hi = mid; }
        l = lo;
        gi = g - a.group_off[l];
    }
    const int cnt = a.pair_off[l + 1] - a.pair_off[l];
    int np = cnt - NQG * gi; if (np > NQG) np = NQG;
    const int pair0 = a.pair_off[l] + NQG * gi;
    const int64_t base = a.list_base[l], len = a.list_len[l];
    const int64_t len_pad = (len + 15) & ~15ll;
    const int64_t c0 = (int64_t)chunk * (BR * SQ_NB);
    if (c0 >= len_pad) return;                   // (workgroup-uniform)
    int64_t c1 = c0 + BR * SQ_NB; if (c1 > len_pad) c1 = len_pad;

    if (tid < NQG) {
        int64_t q = -1, off = 0; uint64_t t = ~0ull; float inv = 0.0f, cst = 0.0f;      // padding slot: nothing passes
        if (tid < np) {
            const int pidx = a.pairs_sorted[pair0 + tid];
            q = pidx / a.nprobe; const int j = pidx - (int)q * a.nprobe;
            off = q * a.tstride + ((!FILTER && a.pre_stride) ? (int64_t)j * a.pre_stride : a.seg_start[q * (a.nprobe + 1) + j]);
            inv = a.sq_qc[2 * q]; cst = a.sq_qc[2 * q + 1];
            if (a.sq_dis0) cst = (cst + a.sq_dis0[q * a.nprobe + j]);
            if (FILTER) { t = a.tau_key[q * a.tau_stride]; off -= q * a.tstride; }
        }
        sqn[tid] = (int32_t)q; segoff[tid] = off; sq[tid] = q < 0 ? 0 : q; stau[tid] = t; sinv[tid] = inv; scst[tid] = cst;
    }

    // this wave's blocks: rows c0 + 16 w + BR i, i < nb (nb = 0: the wave only helps staging the queries)
    const int64_t r0 = c0 + 16 * w;
    const int nb = r0 < c1 ? (int)((c1 - r0 + BR - 1) / BR) : 0;
    const int lr = lane & 15, kg = lane >> 4;
    const uint8_t* xrow = a.sq_codes + (base + r0 + lr) * a.ld + 16 * kg;       // + i * BR * ld + 64 * step
    const int64_t blk_bytes = (int64_t)BR * a.ld;
    floatx4 acc[QT][SQ_NB];
#pragma unroll
    for (int t = 0; t < QT; t++)
#pragma unroll
        for (int i = 0; i < SQ_NB; i++) acc[t][i] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int k0 = 0; k0 < a.ld; k0 += kc) {
        const int kw = a.ld - k0 < kc ? a.ld - k0 : kc;      // dimensions of this slice (a multiple of 64)
        __syncthreads();                                      // sqn is there / everybody is done with the previous slice
        {
            const int ppr = kw >> 3;                          // 16-byte pieces per query row and half
            const int npc = 2 * NQG * ppr;
            for (int pc = tid; pc < npc; pc += NT) {
                const int hl = pc >= NQG * ppr, r = pc - hl * NQG * ppr;
                const int i = r / ppr, t = r - i * ppr;
                const int q = sqn[i];
                uint4 v = make_uint4(0, 0, 0, 0);
                if (q >= 0) v = *reinterpret_cast<const uint4*>((hl ? a.sq_qlo : a.sq_qhi) + (int64_t)q * a.ld + k0 + t * 8);
                *reinterpret_cast<uint4*>((hl ? Ql : Qh) + i * qstride + t * 16) = v;
            }
        }
        __syncthreads();
        const int ns = kw >> 6;                               // K steps of the slice
        const uint8_t* xs = xrow + k0;
        auto load_batch = [&](uint4 (&c)[SQ_U], int i, int s0) {
#pragma unroll
            for (int u = 0; u < SQ_U; u++)
                c[u] = (s0 + u < ns) ? *reinterpret_cast<const uint4*>(xs + i * blk_bytes + (s0 + u) * 64) : make_uint4(0, 0, 0, 0);
        };
        uint4 cur[SQ_U];
        if (nb > 0) load_batch(cur, 0, 0);
#pragma unroll
        for (int i = 0; i < SQ_NB; i++) {
            if (i < nb) {
                for (int s0 = 0; s0 < ns; s0 += SQ_U) {
                    uint4 nxt[SQ_U];
                    if (s0 + SQ_U < ns) load_batch(nxt, i, s0 + SQ_U);
                    else if (i + 1 < nb) load_batch(nxt, i + 1, 0);
                    else {
#pragma unroll
                        for (int u = 0; u < SQ_U; u++) nxt[u] = make_uint4(0, 0, 0, 0);
                    }
#pragma unroll
                    for (int u = 0; u < SQ_U; u++) {
                        if (s0 + u < ns) {
                            half8 x0, x1;
                            sq_widen16(cur[u], x0, x1);
                            const int qoff = lr * qstride + ((s0 + u) * 64 + 16 * kg) * 2;
#pragma unroll
                            for (int t = 0; t < QT; t++) {
                                const unsigned char* ph = Qh + t * 16 * qstride + qoff;
                                const unsigned char* pl = Ql + t * 16 * qstride + qoff;
                                const half8 h0 = *reinterpret_cast<const half8*>(ph), h1 = *reinterpret_cast<const half8*>(ph + 16);
                                const half8 l0 = *reinterpret_cast<const half8*>(pl), l1 = *reinterpret_cast<const half8*>(pl + 16);
                                acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h0, x0, acc[t][i], 0, 0, 0);
                                acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h1, x1, acc[t][i], 0, 0, 0);
                                acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(l0, x0, acc[t][i], 0, 0, 0);
                                acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(l1, x1, acc[t][i], 0, 0, 0);
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < SQ_U; u++) cur[u] = nxt[u];
                }
            }
        }
    }
    // C/D layout of the 16x16 MFMA: reg r of lane l holds (row i = 4 (l >> 4) + r, col j = l & 15): i = query, j = row of the block
#pragma unroll
    for (int i = 0; i < SQ_NB; i++) {
        if (i < nb) {
            const int64_t rloc = r0 + BR * i + lr;
            const float bv = (a.bias && rloc < len) ? a.bias[base + rloc] : 0.0f;
#pragma unroll
            for (int t = 0; t < QT; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int qi = t * 16 + kg * 4 + r;
                const float sc = (((acc[t][i][r] * sinv[qi]) + scst[qi]) + bv);
                if (!FILTER) {
                    if (qi < np) a.temp[segoff[qi] + rloc] = (rloc < len) ? sc : -__builtin_inff();
                } else {
                    // lanes 16 kg .. 16 kg + 15 hold query qi's scores of the block's 16 rows
                    const uint64_t key = (rloc < len && qi < np) ? make_key(sc, (uint32_t)(segoff[qi] + rloc)) : 0ull;
                    const bool pass = key > stau[qi];
                    const uint64_t mask = __ballot(pass);
                    const uint64_t mine = (mask >> (16 * kg)) & 0xffffull;
                    if (mine) {   // one counter update per query per block, as in k_list_scan2
                        const int64_t q = sq[qi];
                        unsigned long long slot0 = 0;
                        const int leader = (__ffsll((unsigned long long)mine) - 1) + 16 * kg;
                        if (lane == leader) slot0 = atomicAdd(&a.cand_cnt[(int64_t)q * CCS], (unsigned long long)__popcll(mine));
                        slot0 = __shfl(slot0, leader);
                        const unsigned long long slot = slot0 + __popcll(mine & ((1ull << lr) - 1ull));
                        if (pass && slot < (unsigned long long)a.cand_cap) a.cand[q * a.cand_cap + slot] = key;
                    }
                }
            }
        }
    }
}

int sq_list_scan_chunk_rows(int qtiles) { return (qtiles >= 4 ? 8 : 4) * 16 * SQ_NB; }
static int sq_kc(int qt, int ld) { const int kmax = qt >= 4 ? 256 : 1024; return ld < kmax ? ld : kmax; }
template <bool FILTER, int QT, int NW>
static void sq_launch(const ListScanArgs& a, dim3 grid, hipStream_t st) {
    const int kc = sq_kc(QT, a.ld);
    const size_t shm = (size_t)2 * 16 * QT * (kc + 8) * 2 + (size_t)16 * QT * (8 + 8 + 8 + 4 + 4 + 4);
    lds_grant(k_sq_list_scan<FILTER, QT, NW>, shm);
    hipLaunchKernelGGL((k_sq_list_scan<FILTER, QT, NW>), grid, dim3(64 * NW), shm, st, a, kc);
}
void launch_sq_list_scan(const ListScanArgs& a, hipStream_t st) {
    if (a.max_groups <= 0 || a.max_chunks <= 0) return;
    const dim3 grid = a.item_off ? dim3((unsigned)((std::max(a.max_items, 1) + 7) & ~7), 1) : dim3((unsigned)a.max_groups, (unsigned)a.max_chunks);      // items: XCD-aware order
    if (a.qtiles >= 4) { if (a.tau_key) sq_launch<true, 4, 8>(a, grid, st); else sq_launch<false, 4, 8>(a, grid, st); }
    else { if (a.tau_key) sq_launch<true, 1, 4>(a, grid, st); else sq_launch<false, 1, 4>(a, grid, st); }
}

// ---------------------------------------------------------------------------------------
// exact scores of the re-run (k_exact_scores_f16's shape for code rows): sixteen consecutive columns per wave, four rows in flight
// ---------------------------------------------------------------------------------------
#define SQ_XS_COLS 16
__global__ __launch_bounds__(256) void k_sq_exact_scores(ExactScoreArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t q = blockIdx.y;
    const int64_t c0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * SQ_XS_COLS;
    if (c0 >= a.tstride) return;
    const int64_t* ss = a.seg_start + q * (a.nprobe + 1);
    const int64_t total = ss[a.nprobe];
    int lo = 0;
    int64_t seg_lo = 0, seg_hi = 0, seg_base = 0, seg_len = 0;
    const float* seg_cen = nullptr;
    auto load_seg = [&]() {
        seg_lo = ss[lo]; seg_hi = ss[lo + 1];
        const int32_t l = a.probe_list[q * a.nprobe + lo];
        seg_base = l >= 0 ? a.list_base[l] : 0; seg_len = l >= 0 ? a.list_len[l] : 0;
        seg_cen = (l >= 0 && a.sq.centroids) ? a.sq.centroids + (int64_t)l * a.d : nullptr;
    };
    if (c0 < total) {
        int hi = a.nprobe;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ss[mid] <= c0) lo = mid; else hi = mid; }
        load_seg();
    }
    const float* qv = a.Q32 + q * a.ldq;
    for (int u4 = 0; u4 < SQ_XS_COLS; u4 += 4) {
        int64_t rows[4]; double acc[4]; const float* cen[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t c = c0 + u4 + u;
            rows[u] = -1; acc[u] = 0.0; cen[u] = nullptr;
            if (c >= a.tstride || c >= total) continue;
            while (c >= seg_hi && lo + 1 < a.nprobe) { lo++; load_seg(); }      // (padded segments: columns past the list's rows stay -inf)
            if (c >= seg_lo && c - seg_lo < seg_len) { rows[u] = seg_base + (c - seg_lo); cen[u] = seg_cen; }
        }
        for (int t4 = 4 * lane; t4 < a.d; t4 += 256) {
            uint32_t w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) w[u] = rows[u] >= 0 ? *reinterpret_cast<const uint32_t*>(a.sq.codes + rows[u] * a.ld + t4) : 0u;
#pragma unroll
            for (int u = 0; u < 4; u++) if (rows[u] >= 0) acc[u] += sq_dot4(w[u], a.sq.trained, cen[u], qv, a.d, t4, a.metric);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t c = c0 + u4 + u;
            if (c >= a.tstride) continue;
            float out = -__builtin_inff();
            if (rows[u] >= 0) {
                const float sc = (float)wave_sum_f64(acc[u]);
                out = (a.metric == 0 ? sc : 0.0f - sc) + 0.0f;
            }
            if (lane == 0) a.temp[q * a.tstride + c] = out;
        }
    }
}
void launch_sq_exact_scores(const ExactScoreArgs& a, hipStream_t st) {
    if (a.nq <= 0 || a.tstride <= 0) return;
    hipLaunchKernelGGL(k_sq_exact_scores, dim3((unsigned)((a.tstride + 4 * SQ_XS_COLS - 1) / (4 * SQ_XS_COLS)), (unsigned)a.nq), dim3(256), 0, st, a);
}

}  // namespace rsx
