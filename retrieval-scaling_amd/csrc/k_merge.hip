// k_merge.hip — rsx_merge_from / rsx_copy_subset_to: the data movement between two handles on one device.
//   k_mg_count / k_mg_fill   copy_subset_to types 0 / 1: one workgroup per list tests the stored ids (k_merge.h: mg_id_selected), counts
//                            the selected entries and, once the host has turned the counts into offsets, writes their storage rows in
//                            list order (prefix sum over the workgroup per tile of MG_WG entries: the order inside a list is kept)
//   k_mg_rows                row kinds (Flat, IVF-Flat fp16 / fp32, IVF-SQ, IndexScalarQuantizer): one workgroup per work item of
//                            <= MG_TILE rows, every lane moves 16-byte pieces (row strides are multiples of 64 bytes); the widening form
//                            reads 8 fp16 values and stores 8 fp32 values; ids (+ add_id) and L2 norm terms move beside the rows
//   k_mg_pq                  IVF-PQ codes between ANY pair of layouts and any phase of the rows inside their blocks: RUNS = true moves
//                            the 16-byte runs both layouts keep together (k_merge.h: mg_pq_run — two 8-byte loads, a byte rotation
//                            by the difference of the rows' phases, two 8-byte stores; neighbouring lanes touch neighbouring pieces),
//                            RUNS = false byte by byte through pq_code_addr (mg_pq_byte: the 4-byte granule layout on either side)
// The work items come from the host (k_merge.h: mg_push_items).  Source and destination are different allocations: no kernel reads
// what another thread of the launch writes.
#include "../../include/rsx.h"
#include "k_merge.h"

namespace rsx {

constexpr int MG_WG = 256;

// exclusive prefix sum of v over the workgroup's four waves; *total = the sum.  wsum: LDS of four ints, free again on return.
__device__ inline int mg_block_scan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < MG_WG / 64; i++) { if (i < wv) before += wsum[i]; all += wsum[i]; }
    __syncthreads();
    *total = all;
    return before + x - v;
}

__global__ __launch_bounds__(MG_WG) void k_mg_count(const int64_t* ids, const int64_t* base, const int64_t* len, int nlist, int type, int64_t a1,
                                                    int64_t a2, int64_t* cnt) {
    __shared__ int wsum[MG_WG / 64];
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const int64_t L = len[l];
        const int64_t* li = ids + base[l];
        int64_t c = 0;
        for (int64_t j0 = 0; j0 < L; j0 += MG_WG) {      // (uniform trip count: every thread reaches the barriers of the scan)
            const int64_t j = j0 + threadIdx.x;
            int t;
            (void)mg_block_scan(j < L && mg_id_selected(type, li[j], a1, a2) ? 1 : 0, wsum, &t);
            c += t;
        }
        if (threadIdx.x == 0) cnt[l] = c;
    }
}

__global__ __launch_bounds__(MG_WG) void k_mg_fill(const int64_t* ids, const int64_t* base, const int64_t* len, int nlist, int type, int64_t a1,
                                                   int64_t a2, const int64_t* off, uint32_t* sel_rows) {
    __shared__ int wsum[MG_WG / 64];
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const int64_t L = len[l], b = base[l];
        int64_t out = off[l];
        for (int64_t j0 = 0; j0 < L; j0 += MG_WG) {
            const int64_t j = j0 + threadIdx.x;
            const int s = j < L && mg_id_selected(type, ids[b + j], a1, a2) ? 1 : 0;
            int t;
            const int r = mg_block_scan(s, wsum, &t);
            if (s) sel_rows[out + r] = (uint32_t)(b + j);      // (storage rows < 2^32: ensure_capacity)
            out += t;
        }
    }
}

__global__ __launch_bounds__(MG_WG) void k_mg_rows(const MergeItem* items, const uint32_t* sel_rows, const uint8_t* sdata, uint8_t* ddata,
                                                   int64_t srb, int64_t drb, int widen, const int64_t* sids, int64_t* dids, int64_t add_id,
                                                   const float* snorms, float* dnorms) {
    const MergeItem it = items[blockIdx.x];
    const int ppr = (int)(srb >> 4);              // 16-byte pieces of a source row
    const int64_t np = (int64_t)it.n * ppr;
    for (int64_t t = threadIdx.x; t < np; t += MG_WG) {
        const int j = (int)(t / ppr), p = (int)(t - (int64_t)j * ppr);
        const uint4 v = *reinterpret_cast<const uint4*>(sdata + mg_row_off(mg_src_row(it, j, sel_rows), srb) + (int64_t)p * 16);
        if (!widen) {
            *reinterpret_cast<uint4*>(ddata + mg_row_off(it.dst + j, drb) + (int64_t)p * 16) = v;
        } else {
            const __half2* h = reinterpret_cast<const __half2*>(&v);
            const float2 f0 = __half22float2(h[0]), f1 = __half22float2(h[1]), f2 = __half22float2(h[2]), f3 = __half22float2(h[3]);
            float4* o = reinterpret_cast<float4*>(ddata + mg_row_off(it.dst + j, drb) + (int64_t)p * 32);
            o[0] = make_float4(f0.x, f0.y, f1.x, f1.y);
            o[1] = make_float4(f2.x, f2.y, f3.x, f3.y);
        }
    }
    for (int j = threadIdx.x; j < it.n; j += MG_WG) {
        const int64_t s = mg_src_row(it, j, sel_rows);
        if (sids) dids[it.dst + j] = sids[s] + add_id;
        if (snorms) dnorms[it.dst + j] = snorms[s];
    }
}

template <bool RUNS>
__global__ __launch_bounds__(MG_WG) void k_mg_pq(const MergeItem* items, const uint32_t* sel_rows, const uint8_t* scodes, uint8_t* dcodes, int M,
                                                 int Mpad, int CBs, int CBd, const int64_t* sids, int64_t* dids, int64_t add_id) {
    const MergeItem it = items[blockIdx.x];
    if (RUNS) {
        const int64_t nr = (int64_t)it.n * (Mpad >> 4);
        for (int64_t t = threadIdx.x; t < nr; t += MG_WG) mg_pq_run(it, t, sel_rows, scodes, dcodes, M, Mpad, CBs, CBd);
    } else {
        const int64_t nb = (int64_t)it.n * Mpad;
        for (int64_t t = threadIdx.x; t < nb; t += MG_WG) mg_pq_byte(it, t, sel_rows, scodes, dcodes, M, Mpad, CBs, CBd);
    }
    for (int j = threadIdx.x; j < it.n; j += MG_WG) dids[it.dst + j] = sids[mg_src_row(it, j, sel_rows)] + add_id;
}

void launch_mg_count(const int64_t* ids, const int64_t* base, const int64_t* len, int nlist, int type, int64_t a1, int64_t a2, int64_t* cnt,
                     hipStream_t st) {
    hipLaunchKernelGGL(k_mg_count, dim3((unsigned)std::min(nlist, 65536)), dim3(MG_WG), 0, st, ids, base, len, nlist, type, a1, a2, cnt);
}
void launch_mg_fill(const int64_t* ids, const int64_t* base, const int64_t* len, int nlist, int type, int64_t a1, int64_t a2, const int64_t* off,
                    uint32_t* sel_rows, hipStream_t st) {
    hipLaunchKernelGGL(k_mg_fill, dim3((unsigned)std::min(nlist, 65536)), dim3(MG_WG), 0, st, ids, base, len, nlist, type, a1, a2, off, sel_rows);
}
void launch_mg_rows(const MergeItem* items, int64_t nitems, const uint32_t* sel_rows, const uint8_t* sdata, uint8_t* ddata, int64_t srb,
                    int64_t drb, int widen, const int64_t* sids, int64_t* dids, int64_t add_id, const float* snorms, float* dnorms, hipStream_t st) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(k_mg_rows, dim3((unsigned)nitems), dim3(MG_WG), 0, st, items, sel_rows, sdata, ddata, srb, drb, widen, sids, dids, add_id,
                       snorms, dnorms);
}
void launch_mg_pq(const MergeItem* items, int64_t nitems, const uint32_t* sel_rows, const uint8_t* scodes, uint8_t* dcodes, int M, int Mpad,
                  int CBs, int CBd, const int64_t* sids, int64_t* dids, int64_t add_id, hipStream_t st) {
    if (nitems <= 0) return;
    if (mg_pq_runs_apply(CBs, CBd))
        hipLaunchKernelGGL(k_mg_pq<true>, dim3((unsigned)nitems), dim3(MG_WG), 0, st, items, sel_rows, scodes, dcodes, M, Mpad, CBs, CBd, sids, dids, add_id);
    else
        hipLaunchKernelGGL(k_mg_pq<false>, dim3((unsigned)nitems), dim3(MG_WG), 0, st, items, sel_rows, scodes, dcodes, M, Mpad, CBs, CBd, sids, dids, add_id);
}

}  // namespace rsx
