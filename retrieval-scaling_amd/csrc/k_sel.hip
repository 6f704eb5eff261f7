// k_sel.hip — filtered search (rsx_search_sel): the slot mask of an id selector and its application to score rows.
// Neither kernel is launched by an unfiltered search.  FAISS 1.8.0 tests IDSelector::is_member(id) inside its scan loops
// (IndexFlat / InvertedListScanner); here the test runs once per (selector, index state) over the storage slots, and the
// searches read one bit per scored row.
#include "../../include/rsx.h"
#include "rsx_sel.h"

namespace rsx {

__device__ inline bool sel_member(const SelDevArgs& s, int64_t id) {
    bool m;
    if (s.kind == RSX_SEL_RANGE) m = id >= s.lo && id < s.hi;
    else if (s.kind == RSX_SEL_BITMAP) m = id >= 0 && (id >> 3) < s.nbytes && ((s.bitmap[id >> 3] >> (id & 7)) & 1);
    else {      // sorted unique ids: lower bound
        int64_t lo = 0, hi = s.nids;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (s.ids[mid] < id) lo = mid + 1; else hi = mid; }
        m = lo < s.nids && s.ids[lo] == id;
    }
    return m != (s.invert != 0);
}

// one lane per slot, one 64-slot ballot per wave: the slot ids are read coalesced and lane 0 writes the wave's two mask words
// (bit b of word w <=> slot 32 w + b holds a selected id; slot_ids null: slot = id)
__global__ __launch_bounds__(256) void k_sel_mask(SelDevArgs s, const int64_t* slot_ids, int64_t nslots, uint32_t* mask) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63));
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = wave0; base < nslots; base += step) {       // wave-uniform loop
        const int64_t slot = base + lane;
        bool m = false;
        if (slot < nslots) m = sel_member(s, slot_ids ? slot_ids[slot] : slot);
        const uint64_t bits = __ballot(m);
        if (lane == 0) { mask[base >> 5] = (uint32_t)bits; mask[(base >> 5) + 1] = (uint32_t)(bits >> 32); }
    }
}
void launch_sel_mask(const SelDevArgs& s, const int64_t* slot_ids, int64_t nslots, uint32_t* mask, hipStream_t st) {
    if (nslots <= 0) return;
    const int blocks = (int)std::min<int64_t>((nslots + 255) / 256, 65536);
    hipLaunchKernelGGL(k_sel_mask, dim3(blocks), dim3(256), 0, st, s, slot_ids, nslots, mask);
}

__device__ inline bool mask_bit(const uint32_t* mask, int64_t slot) { return (mask[slot >> 5] >> (slot & 31)) & 1u; }

// Flat: column c of a score row is slot slot0 + c.  A masked column becomes -inf, which make_key turns into "no element".
__global__ __launch_bounds__(256) void k_sel_apply_flat(float* temp, int64_t tstride, int64_t n, int64_t slot0, const uint32_t* mask) {
    float* row = temp + (int64_t)blockIdx.y * tstride;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x)
        if (!mask_bit(mask, slot0 + c)) row[c] = -__builtin_inff();
}
// IVF: one workgroup per (probe, query); segment j of query q's row holds list probe_list[q, j] from column seg_start[q, j]
// (its padding columns are -inf already)
__global__ __launch_bounds__(256) void k_sel_apply_ivf(float* temp, int64_t tstride, const uint32_t* mask, const int32_t* probe_list,
                                                       const int64_t* seg_start, int nprobe, const int64_t* list_base, const int64_t* list_len) {
    const int64_t q = blockIdx.y;
    const int j = blockIdx.x;
    const int32_t l = probe_list[q * nprobe + j];
    if (l < 0) return;
    const int64_t c0 = seg_start[q * (nprobe + 1) + j], base = list_base[l], len = list_len[l];
    float* row = temp + q * tstride + c0;
    for (int64_t i = threadIdx.x; i < len; i += blockDim.x)
        if (!mask_bit(mask, base + i)) row[i] = -__builtin_inff();
}
void launch_sel_apply(const SelApplyArgs& a, hipStream_t st) {
    if (a.nq <= 0) return;
    if (a.flat_n >= 0) {
        if (a.flat_n == 0) return;
        const int bx = (int)std::min<int64_t>((a.flat_n + 255) / 256, 1024);
        hipLaunchKernelGGL(k_sel_apply_flat, dim3(bx, (unsigned)a.nq), dim3(256), 0, st, a.temp, a.tstride, a.flat_n, a.slot0, a.mask);
        return;
    }
    if (a.nprobe <= 0) return;
    hipLaunchKernelGGL(k_sel_apply_ivf, dim3((unsigned)a.nprobe, (unsigned)a.nq), dim3(256), 0, st, a.temp, a.tstride, a.mask, a.probe_list,
                       a.seg_start, a.nprobe, a.list_base, a.list_len);
}

}  // namespace rsx
