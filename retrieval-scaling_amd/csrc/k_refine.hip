// k_refine.hip — rsx_refine: exact re-ranking of candidates named by LABEL against a Flat handle's row store (FAISS:
// IndexFlat::compute_distance_subset followed by IndexRefine::search's re-order).  One launch per batch, one workgroup per query:
// the kc labels of the query go to LDS, every label in [0, ntotal) is scored against its stored row with k_finalize's arithmetic
// (k_rescore.h: one wave per candidate, four candidates per wave in flight, 16-byte loads on fp16 rows, fp64 sum rounded once), the
// (order word, label) pairs are sorted by (score desc / distance asc, label asc) and the best k leave.
#include "rsx_internal.h"
#include "k_rescore.h"

namespace rsx {

// LDS: sid [KP] int64 | sord [KP] uint32 | rank sort only, from the next 16-byte boundary: sord2 [KP + (KP & 1)] uint32 | sid2 [KP] int64.
// KP = kc (rank sort) or kc rounded up to a power of two (bitonic network: 12 bytes per slot, 48 KiB at kc = 4096).
static inline size_t refine_lds_bytes(int KP, int rank_sort) {
    const size_t base = (((size_t)KP * 12 + 15) / 16) * 16;
    return rank_sort ? base + (size_t)(KP + (KP & 1)) * 4 + (size_t)KP * 8 : base;
}

__global__ __launch_bounds__(1024) void k_refine(RefineArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t rf_buf[];
    const int KP = a.KP, kc = a.kc;
    int64_t* sid = (int64_t*)rf_buf;                 // the label IS the storage row of a Flat handle without explicit ids
    uint32_t* sord = (uint32_t*)(sid + KP);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6, nwv = nt >> 6;
    const int64_t q = blockIdx.x;

    // labels < 0 are padding of the base search and skipped; a label >= ntotal is skipped as well and marks the call (the host refuses
    // it after the closing synchronisation).  A skipped slot is a sink: order word 0, id INT64_MAX — rescore_rows dereferences rows
    // of [0, ntotal) only.
    bool out_of_range = false;
    for (int c = tid; c < KP; c += nt) {
        const int64_t label = c < kc ? a.labels[q * kc + c] : -1;
        out_of_range |= label >= a.ntotal;
        sid[c] = (label >= 0 && label < a.ntotal) ? label : INT64_MAX;
        sord[c] = 0u;
    }
    if (out_of_range) *a.flag = 1;
    __syncthreads();

    rescore_rows(a.X, a.x_f16, a.ld, a.d, a.metric, a.Q32 + q * a.ldq, a.ldq, a.ntotal, sid, sord, 0, kc, lane, wv, nwv);

    uint32_t* sord2 = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(rf_buf) + (((size_t)KP * 12 + 15) / 16) * 16);
    int64_t* sid2 = reinterpret_cast<int64_t*>(sord2 + KP + (KP & 1));
    sort_candidates(sord, sid, KP, a.rank_sort, sord2, sid2, tid, nt);

    for (int j = tid; j < a.k; j += nt) {
        const bool valid = sord[j] != 0 && sid[j] != INT64_MAX;
        float s = valid ? ord2f(sord[j]) : -__builtin_inff();
        if (a.metric != 0) s = valid ? (0.0f - s) : __builtin_inff();
        a.D[q * a.k + j] = s;
        a.I[q * a.k + j] = valid ? sid[j] : -1;
    }
}

void launch_refine(const RefineArgs& a0, hipStream_t st) {
    if (a0.nq <= 0) return;
    RefineArgs a = a0;
    a.rank_sort = a.kc <= REFINE_RANK_MAX ? 1 : 0;
    a.KP = a.rank_sort ? a.kc : 1;
    while (a.KP < a.kc) a.KP <<= 1;
    // the row gather is bound by the rows in flight (1.5 KB rows anywhere in HBM): a wave per four candidates, up to sixteen
    const int waves = std::min(16, std::max(1, (a.kc + 3) / 4));
    hipLaunchKernelGGL(k_refine, dim3((unsigned)a.nq), dim3(64 * waves), refine_lds_bytes(a.KP, a.rank_sort), st, a);
}

}  // namespace rsx
