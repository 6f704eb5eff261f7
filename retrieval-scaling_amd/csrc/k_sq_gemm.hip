// k_sq_gemm.hip — the large-batch scan of IndexScalarQuantizer (RSX_KIND_SQ): an int8 GEMM of the stored code bytes against
// two int8 planes of every query on the i8 matrix cores (v_mfma_i32_32x32x32_i8), and the kernel that makes the planes (rsx_sqflat.h).
//   * code - 128 is an int8, exactly: a K step XORs the code bytes with 0x80 in registers;
//   * the query side is w_j = rint(q'_j s) = 128 h_j + l_j, two int8 planes; both accumulate in i32 without rounding, and the epilogue
//     forms A = 128 A_h + A_l in i32 (sqflat_wmax keeps every term below 2^31): the scan's only error is the rounding of the queries;
//   * the tile is k_flat_gemm2's (k_gemm.hip) in BYTES: a 128-byte row slice per K step — now 128 dimensions —, 16-byte chunks swizzled by
//     chunk ^ ((row >> 1) & 7), ds_read_b128 operands (16 int8 for 32x32x32), two 64 KiB stages filled by LDS-DMA, one barrier per K step.
//     The two planes of a query cost as many bytes per dimension as an fp16 query did, so the QUERY TILE is 128 queries (2 planes x 128
//     rows x 128 B = 32 KiB, beside 256 code rows x 128 B = 32 KiB); a workgroup of 8 waves (2 x 4) computes 128 queries x 256 rows, a
//     wave 64 x 64 for both planes: 2 x 2 x 2 accumulator tiles (128 registers, as k_flat_gemm2) and 6 ds_read_b128 per 8 MFMAs;
//   * kept from k_flat_gemm2: the persistent XCD-ranged walk of the filtered form (a code tile crosses HBM once per XCD), the per-wave
//     queue of passing keys in LDS with one atomic round trip per flush.
#include "rsx_sqflat.h"

#include <algorithm>

// (the planes' arithmetic is specified operation by operation: tests/sqflat_ref.py restates it)
#pragma clang fp contract(off)

namespace rsx {

typedef int int32x16 __attribute__((ext_vector_type(16)));
typedef int int32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------
// the planes: one workgroup per row of the padded batch
// ---------------------------------------------------------------------------------------
// rho_bits: running maximum over the batch of max_j |q'_j| / |q| (float bits, atomicMax): what the certificate's half-unit term scales with
__global__ __launch_bounds__(256) void k_sqflat_planes(const float* Q32, int ldq, int64_t nq, int d, int ldp, const float* trained, int wmax,
                                                       int8_t* planes, float* qs, unsigned int* rho_bits) {
    __shared__ double s_sum[4], s_q2[4];
    __shared__ float s_max[4];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int8_t* ph = planes + ((q >> 7) * 256 + (q & 127)) * (int64_t)ldp;
    int8_t* pl = ph + (int64_t)128 * ldp;
    if (q >= nq) {                                   // (workgroup-uniform) padding row: zero planes, nothing of it is ever read back
        for (int t = tid; t < ldp; t += 256) { ph[t] = 0; pl[t] = 0; }
        if (tid == 0) { qs[2 * q] = 0.0f; qs[2 * q + 1] = 0.0f; }
        return;
    }
    const float* qv = Q32 + q * ldq;
    double sum = 0.0, q2 = 0.0; float mx = 0.0f;
    for (int t = tid; t < d; t += 256) {
        const float qp = ((qv[t] * trained[d + t]) / 255.0f);
        sum += (double)qv[t] * (double)trained[t] + 128.5 * (double)qp;
        q2 += (double)qv[t] * (double)qv[t];
        mx = fmaxf(mx, fabsf(qp));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { sum += __shfl_xor(sum, off); q2 += __shfl_xor(q2, off); mx = fmaxf(mx, __shfl_xor(mx, off)); }
    if (lane == 0) { s_sum[wv] = sum; s_q2[wv] = q2; s_max[wv] = mx; }
    __syncthreads();
    sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    q2 = (s_q2[0] + s_q2[1]) + (s_q2[2] + s_q2[3]);
    mx = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    if (tid == 0 && mx > 0.0f && mx < __builtin_inff() && q2 > 0.0) atomicMax(rho_bits, __float_as_uint((float)((double)mx / sqrt(q2)) * 1.000001f));
    // s = wmax / max |q'|, at most 2^100 (s and 1 / s stay normal floats; a query whose largest |q'_j| lies below wmax 2^-100 keeps |w_j| <= wmax
    // but not the bound's half-unit term: DESIGN.md 10, as k_sq_query_factors)
    float sc = 1.0f;
    if (mx > 0.0f && mx < __builtin_inff()) { sc = ((float)wmax / mx); sc = sc < 0x1p100f ? sc : 0x1p100f; }
    if (tid == 0) { qs[2 * q] = (1.0f / sc); qs[2 * q + 1] = (float)sum; }
    for (int t = tid; t < ldp; t += 256) {
        int h = 0, l = 0;
        if (t < d) {
            const float v = (((qv[t] * trained[d + t]) / 255.0f) * sc);
            int w = (int)rintf(v);
            w = w > wmax ? wmax : (w < -wmax ? -wmax : w);          // (a NaN / infinite query: any int8 pair; its scores are not finite either way)
            h = (w + 64) >> 7; l = w - (h << 7);
        }
        ph[t] = (int8_t)h; pl[t] = (int8_t)l;
    }
}
void launch_sqflat_planes(const float* Q32, int ldq, int64_t nq, int64_t nq_pad, int d, int ldp, const float* trained, int wmax, int8_t* planes,
                          float* qs, unsigned int* rho_bits, hipStream_t st) {
    if (nq_pad <= 0) return;
    hipLaunchKernelGGL(k_sqflat_planes, dim3((unsigned)nq_pad), dim3(256), 0, st, Q32, ldq, nq, d, ldp, trained, wmax, planes, qs, rho_bits);
}

// ---------------------------------------------------------------------------------------
// k_sq_gemm
// ---------------------------------------------------------------------------------------
#define SQG_STAGE 65536
#define SQG_QCAP 192        // entries of a wave's queue of passing keys (filtered epilogue); flushed beyond QCAP - 128

struct SqgFilter {
    const uint64_t* tau; int64_t tau_stride;
    uint64_t* cand; unsigned long long* cand_cnt; int cand_cap;
    int nq, qt; int64_t ntiles; int walk;
};

__device__ __forceinline__ void sqg_dma16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// P: planes (launch_sqflat_planes), a query tile = 256 consecutive rows of ldp bytes (plane h of its 128 queries, then plane l);
// X: code rows of ld bytes (ld % 64 == 0, ldp = ld rounded up to 128)
template <bool FILTER>
__global__ __launch_bounds__(512) void k_sq_gemm(const int8_t* P, const float* qs, int nq_pad, int ldp, const uint8_t* X, int64_t v0, int64_t nv,
                                                 int ld, const float* bias, float* temp, int64_t tstride, SqgFilter F) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sqg_smem[];   // 2 stages x (planes 32 KiB | codes 32 KiB), per-query words
    uint64_t* s_tau = reinterpret_cast<uint64_t*>(sqg_smem + 2 * SQG_STAGE);    // [2][128] threshold keys (FILTER)
    float* s_tf = reinterpret_cast<float*>(s_tau + 256);                        // [2][128] ... as floats
    float* s_inv = s_tf + 256;                                                  // [2][128] 1 / s
    float* s_qc = s_inv + 256;                                                  // [2][128] the query's constant
    uint64_t* s_wq_key = reinterpret_cast<uint64_t*>(s_qc + 256);               // (FILTER) per-wave queue of passing keys [8][SQG_QCAP] ...
    uint16_t* s_wq_q = reinterpret_cast<uint16_t*>(s_wq_key + 8 * SQG_QCAP);    // ... and their queries inside the tile
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr0 = __builtin_amdgcn_readfirstlane(w >> 2), wc0 = __builtin_amdgcn_readfirstlane(w & 3);
    // work items = (query tile, code tile) pairs through ONE software pipeline of K steps, as k_flat_gemm2:
    //  !FILTER       : one pair per workgroup (2-D grid);
    //  FILTER, walk  : persistent workgroups; workgroup b sits on XCD b % 8, slot s = b / 8 keeps query tile s % qt and walks the code tiles
    //                  x + 8 (s / qt) + 8 (S / qt) n — the qt slots that share s / qt walk the same tiles at the same pace;
    //  FILTER, !walk : the workgroup owns ONE code tile and passes every query tile over it (small launches).
    const bool walk = FILTER && F.walk != 0;
    int qi0, nitems;
    int64_t vt0, vt_step;
    if (!FILTER) { vt0 = (int64_t)blockIdx.y * 256; vt_step = 0; qi0 = (int)blockIdx.x; nitems = 1; }
    else if (!walk) { vt0 = (int64_t)blockIdx.x * 256; vt_step = 0; qi0 = 0; nitems = F.qt; }
    else {
        const int x = blockIdx.x & 7, s = blockIdx.x >> 3, ngq = (int)(gridDim.x >> 3) / F.qt;
        qi0 = s % F.qt;
        const int64_t t0 = x + 8 * (s / F.qt), tstep = 8 * (int64_t)ngq;
        vt0 = t0 * 256; vt_step = tstep * 256;
        nitems = t0 < F.ntiles ? (int)((F.ntiles - 1 - t0) / tstep) + 1 : 0;
        if (nitems == 0) return;
    }
    auto load_query_words = [&](int qi) {       // tid < 128
        const int64_t qn = (int64_t)qi * 128 + tid;
        const int o = (qi & 1) * 128 + tid;
        s_inv[o] = qs[2 * qn]; s_qc[o] = qs[2 * qn + 1];           // qn < nq_pad: the padding rows hold zeros
        if (FILTER) {
            const uint64_t t = (qn < F.nq) ? F.tau[qn * F.tau_stride] : ~0ull;
            s_tau[o] = t;
            s_tf[o] = (qn < F.nq) ? key_score(t) : __builtin_inff();
        }
    };
    if (tid < 128) load_query_words(qi0);

    // DMA sources: wave w copies blocks [4w, 4w + 4) (8 rows each) of both operands, every stage.  A code row's last K step may hold only 64
    // bytes (ld % 128 = 64): the lanes of its upper half fetch the lower half again — the planes are zero there, any byte will do — instead
    // of reading past the row (and, behind the last row, past the allocation)
    const char* srcA[4];
    int cB[2];
    const int r8 = lane >> 3;
    {
        const int p = lane & 7;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int R = (4 * w + j) * 8 + r8;
            const int c = p ^ ((R >> 1) & 7);
            srcA[j] = reinterpret_cast<const char*>(P) + ((int64_t)qi0 * 256 + R) * ldp + c * 16;   // nq_pad % 128 == 0
            if (j < 2) cB[j] = c * 16;                                                              // c depends on j & 1 only
        }
    }
    const char* xb = reinterpret_cast<const char*>(X) + v0 * ld;
    const int KT = ldp / 128;
    const int G = nitems * KT;                   // K steps of all work items, one software pipeline
    const int64_t a_step = walk ? 0 : (int64_t)256 * ldp;        // the next item's query tile ...
    const int64_t i_vstep = vt_step;                              // ... or code tile
    const int64_t vlast = nv - 1;
    int i_kt = 0; int64_t i_aoff = 0, i_vt = vt0;    // position of the next stage to issue
    auto issue = [&](int buf, bool advance) {
        unsigned char* sa = sqg_smem + buf * SQG_STAGE + (4 * w) * 1024;
        unsigned char* sb = sa + 32768;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int64_t xrow = i_vt + ((4 * w + j) * 8 + r8);
            xrow = xrow > vlast ? vlast : xrow;
            int koff = i_kt * 128 + cB[j & 1];
            koff = koff >= ld ? koff - 64 : koff;
            sqg_dma16(srcA[j] + i_aoff + (int64_t)i_kt * 128, sa + j * 1024);
            sqg_dma16(xb + (uint64_t)(uint32_t)xrow * (uint32_t)ld + koff, sb + j * 1024);
        }
        i_kt += advance ? 1 : 0;
        const bool wrap = i_kt == KT;
        i_kt = wrap ? 0 : i_kt;
        i_aoff += wrap ? a_step : 0;
        i_vt += wrap ? i_vstep : 0;
    };

    // acc[t][tj]: t = 2 plane + query sub-tile (32 queries), tj = code sub-tile (32 rows)
    int32x16 acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0;

    const int li = lane & 31, kh = lane >> 5;
    const int sw = (li >> 1) & 7;
    int offs[4];
#pragma unroll
    for (int s = 0; s < 4; s++) offs[s] = li * 128 + (((2 * s + kh) ^ sw) << 4);

    issue(0, G > 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // operand fragments are double-buffered in registers, as in k_flat_gemm2; a lane's 16 bytes of an operand are the same K positions in
    // both operands (chunk 2 s + kh of the row slice), so the sum does not depend on how the instruction orders K inside a step
    int32x4 fa[2][4], fb[2][2];
#define SQG_LOAD_FRAGS(BUF, S, SLOT)                                                                                   \
    {                                                                                                                    \
        const unsigned char* As_ = sqg_smem + (BUF) * SQG_STAGE + wr0 * (64 * 128);                                      \
        const unsigned char* Bs_ = sqg_smem + (BUF) * SQG_STAGE + 32768 + wc0 * (64 * 128);                              \
        _Pragma("unroll") for (int t = 0; t < 4; t++)                                                                    \
            fa[SLOT][t] = *reinterpret_cast<const int32x4*>(As_ + (t >> 1) * (128 * 128) + (t & 1) * 4096 + offs[S]);    \
        _Pragma("unroll") for (int t = 0; t < 2; t++)                                                                    \
            fb[SLOT][t] = *reinterpret_cast<const int32x4*>(Bs_ + t * 4096 + offs[S]);                                   \
    }
#define SQG_MFMAS(SLOT)                                                                                                \
    {                                                                                                                    \
        const int32x4 m80_ = {(int)0x80808080u, (int)0x80808080u, (int)0x80808080u, (int)0x80808080u};                   \
        const int32x4 b0_ = fb[SLOT][0] ^ m80_, b1_ = fb[SLOT][1] ^ m80_;       /* code - 128 as int8 */                 \
        _Pragma("unroll") for (int ti = 0; ti < 4; ti++) {                                                               \
            acc[ti][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[SLOT][ti], b0_, acc[ti][0], 0, 0, 0);                  \
            acc[ti][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[SLOT][ti], b1_, acc[ti][1], 0, 0, 0);                  \
        }                                                                                                                \
    }
    SQG_LOAD_FRAGS(0, 0, 0)
    const int lj0 = lane & 31, lh0 = lane >> 5;
    int kt = 0, qi = qi0;
    int64_t vt = vt0;                            // code tile of the item being computed (the issue position runs ahead)
    for (int g = 0; g < G; g++) {
        // sub-step 0 carries the DMA of the NEXT stage (into the buffer every wave left at the last barrier); the last step re-fetches its
        // own stage into the idle buffer so the body stays branch-free
        issue((g + 1) & 1, g + 2 < G);
        SQG_LOAD_FRAGS(g & 1, 1, 1)
        SQG_MFMAS(0)
        SQG_LOAD_FRAGS(g & 1, 2, 0)
        SQG_MFMAS(1)
        SQG_LOAD_FRAGS(g & 1, 3, 1)
        SQG_MFMAS(0)
        SQG_MFMAS(1)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // my pieces of stage g+1 have landed
        __syncthreads();                                    // everyone: done with stage g, stage g+1 complete
        if (++kt < KT) {
            SQG_LOAD_FRAGS((g + 1) & 1, 0, 0)
            continue;
        }
        kt = 0;
        // ---- end of a work item: the sums of (query tile qi, code tile vt) are complete
        const int64_t q0 = (int64_t)qi * 128;
        // launder the lane coordinates (k_flat_gemm2: what is derived from them would otherwise be hoisted out of the K loop and held in registers)
        int lj = lj0, lh = lh0, wr = wr0, wc = wc0;
        asm volatile("" : "+v"(lj), "+v"(lh), "+s"(wr), "+s"(wc));
        const float* invs = s_inv + (qi & 1) * 128;
        const float* qcs = s_qc + (qi & 1) * 128;
        float bv[2]; int64_t colv[2];
#pragma unroll
        for (int tj = 0; tj < 2; tj++) {
            colv[tj] = vt + wc * 64 + tj * 32 + lj;
            bv[tj] = (bias && colv[tj] < nv) ? bias[v0 + colv[tj]] : 0.0f;
        }
        if (!FILTER) {
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int ql = wr * 64 + u * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const int64_t qrow = q0 + ql;
                    const float inv = invs[ql], qc = qcs[ql];
#pragma unroll
                    for (int tj = 0; tj < 2; tj++) {
                        const int A = (acc[u][tj][r] << 7) + acc[2 + u][tj][r];
                        if (colv[tj] < nv && qrow < nq_pad) temp[qrow * tstride + colv[tj]] = ((((float)A * inv) + qc) + bv[tj]);
                    }
                }
        } else {
            const uint64_t* taus = s_tau + (qi & 1) * 128;
            const float* tfs = s_tf + (qi & 1) * 128;
            const bool in0 = colv[0] < nv, in1 = colv[1] < nv;
            uint64_t* wq_key = s_wq_key + w * SQG_QCAP;
            uint16_t* wq_q = s_wq_q + w * SQG_QCAP;
            int qn = 0;                                   // wave-uniform
            auto flush = [&]() {
                __builtin_amdgcn_wave_barrier();
                for (int i = lane; i < qn; i += 64) {
                    const uint64_t key = wq_key[i];
                    const int64_t qg = q0 + wq_q[i];
                    const unsigned long long slot = atomicAdd(&F.cand_cnt[qg * CCS], 1ull);
                    if (slot < (unsigned long long)F.cand_cap) F.cand[qg * F.cand_cap + slot] = key;
                }
                __builtin_amdgcn_wave_barrier();
                qn = 0;
            };
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int ql = wr * 64 + u * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;   // query inside the tile
                    const float inv = invs[ql], qc = qcs[ql];
                    const int A0 = (acc[u][0][r] << 7) + acc[2 + u][0][r], A1 = (acc[u][1][r] << 7) + acc[2 + u][1][r];
                    const float s0 = ((((float)A0 * inv) + qc) + bv[0]), s1 = ((((float)A1 * inv) + qc) + bv[1]);
                    // fast reject of the row pair on the float threshold (+inf for padding queries); the decision below is on the full key
                    const float tf = tfs[ql];
                    if (!__any((in0 && s0 >= tf) || (in1 && s1 >= tf))) continue;
                    const uint64_t tau = taus[ql];
#pragma unroll
                    for (int tj = 0; tj < 2; tj++) {
                        const float sc = tj ? s1 : s0;
                        const uint64_t key = (colv[tj] < nv) ? make_key(sc, (uint32_t)(v0 + colv[tj])) : 0ull;
                        const bool pass = key > tau;
                        const uint64_t mask = __ballot(pass);
                        if (mask) {
                            const int pos = qn + (int)__popcll(mask & ((1ull << lane) - 1ull));
                            if (pass) { wq_key[pos] = key; wq_q[pos] = (uint16_t)ql; }
                            qn += (int)__popcll(mask);
                        }
                    }
                    if (qn > SQG_QCAP - 128) flush();
                }
            if (qn) flush();
        }
        // the per-query words of the next pass (read after at least one more barrier)
        if (FILTER && !walk && qi + 1 < nitems && tid < 128) load_query_words(qi + 1);
        if (FILTER && KT == 1) __syncthreads();          // no K-loop barrier would order them before the next epilogue
        qi += walk ? 0 : 1;
        vt += vt_step;
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[a][b][r] = 0;
        if (g + 1 < G) SQG_LOAD_FRAGS((g + 1) & 1, 0, 0)
    }
#undef SQG_MFMAS
#undef SQG_LOAD_FRAGS
}

static const size_t SQG_SHM = 2 * SQG_STAGE + 2 * 128 * 8 + 3 * 2 * 128 * 4;
static const size_t SQG_SHM_FILTER = SQG_SHM + 8 * SQG_QCAP * (8 + 2);

void launch_sqflat_gemm(const int8_t* planes, const float* qs, int nq_pad, int ldp, const uint8_t* codes, int64_t v0, int64_t nv, int ld,
                        const float* bias, float* temp, int64_t tstride, hipStream_t st) {
    if (nv <= 0 || nq_pad <= 0) return;
    SqgFilter F{};
    lds_grant(k_sq_gemm<false>, SQG_SHM);
    const dim3 grid((unsigned)(nq_pad / 128), (unsigned)((nv + 255) / 256));
    hipLaunchKernelGGL((k_sq_gemm<false>), grid, dim3(512), SQG_SHM, st, planes, qs, nq_pad, ldp, codes, v0, nv, ld, bias, temp, tstride, F);
}

void launch_sqflat_gemm_filter(const int8_t* planes, const float* qs, int nq_pad, int nq, int ldp, const uint8_t* codes, int64_t v0, int64_t nv,
                               int ld, const float* bias, const uint64_t* tau, int64_t tau_stride, uint64_t* cand, unsigned long long* cand_cnt,
                               int cand_cap, hipStream_t st) {
    if (nv <= 0 || nq_pad <= 0) return;
    SqgFilter F{};
    F.tau = tau; F.tau_stride = tau_stride; F.cand = cand; F.cand_cnt = cand_cnt; F.cand_cap = cand_cap;
    F.nq = nq; F.qt = nq_pad / 128; F.ntiles = (nv + 255) / 256;
    lds_grant(k_sq_gemm<true>, SQG_SHM_FILTER);
    // persistent walking workgroups once every slot has a few code tiles to walk (k_flat_gemm2's rule)
    static int ncu_of[64] = {};
    int& ncu = ncu_of[cur_device()];
    if (ncu == 0) {
        int dev = 0; hipDeviceProp_t pr;
        ncu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
    }
    const int slots = ((ncu / 8) / F.qt) * F.qt;              // per XCD, a multiple of the query tiles
    unsigned grid = (unsigned)F.ntiles;
    if (slots > 0 && nv < ((int64_t)1 << 31) && F.ntiles >= (int64_t)4 * 8 * (slots / F.qt)) { F.walk = 1; grid = 8u * (unsigned)slots; }
    hipLaunchKernelGGL((k_sq_gemm<true>), dim3(grid), dim3(512), SQG_SHM_FILTER, st, planes, qs, nq_pad, ldp, codes, v0, nv, ld, bias,
                       (float*)nullptr, (int64_t)0, F);
}

}  // namespace rsx
