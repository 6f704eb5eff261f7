// k_remove.hip — rsx_remove_ids (FAISS Index::remove_ids): the removal plan and the in-place compaction of the storage.
// The slot mask of the selector comes from k_sel_mask (k_sel.hip): bit s = the vector in storage slot s is removed.
//   IVF (IndexIVF::remove_ids -> DirectMap::remove_ids, NoMap branch): per list, the loop
//       j = 0; l = len; while (j < l) { if (is_member(ids[j])) { l--; entry[j] = entry[l]; } else j++; }  len = l;
//   has a closed form: the holes below the new length, ascending, take the kept entries at or above it, descending.  Sources
//   and destinations are disjoint slot sets, so one launch moves every entry; the vacated slots are cleared by the next one.
//   Flat (IndexFlatCodes::remove_ids / IndexIDMap::remove_ids): stable compaction by a prefix sum of the kept counts, staged
//   through a bounded buffer one source chunk at a time (a kept row's destination can be another kept row's source).
// Lists start on multiples of 64 slots (rsx_index::row_align), so a list's first slot is the first bit of a mask word.
#include "../../include/rsx.h"
#include "rsx_internal.h"

namespace rsx {

constexpr int RM_WG = 256;      // workgroup: four waves; one mask word (32 slots) per thread and tile

// bits of mask word w (slots 32 w .. 32 w + 31 of a list) inside [lo, hi)
__device__ inline uint32_t rm_range_bits(int64_t w, int64_t lo, int64_t hi) {
    const int64_t s = w * 32;
    if (s >= hi || s + 32 <= lo) return 0u;
    uint32_t m = 0xFFFFFFFFu;
    if (lo > s) m &= 0xFFFFFFFFu << (int)(lo - s);
    if (hi < s + 32) m &= (1u << (int)(hi - s)) - 1u;
    return m;
}

// exclusive prefix sum of v over the workgroup (wave scan by shuffles, then the four wave totals); *total = the sum.
// Every thread of the workgroup calls it; wsum is LDS of four ints, free again when the function returns.
__device__ inline int64_t rm_block_scan(int64_t v, int64_t* wsum, int64_t* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int i = 0; i < RM_WG / 64; i++) { if (i < wv) before += wsum[i]; all += wsum[i]; }
    __syncthreads();
    *total = all;
    return before + x - v;
}

__device__ inline int64_t rm_block_sum(int64_t v, int64_t* wsum) {
    int64_t t;
    (void)rm_block_scan(v, wsum, &t);
    return t;
}

// ---------------------------------------------------------------------------------------
// IVF plan
// ---------------------------------------------------------------------------------------
// per list: removed count -> new length; nmoves = the removed entries below the new length (= the kept entries at or above it)
__global__ __launch_bounds__(RM_WG) void k_rm_count(const uint32_t* mask, const int64_t* base, const int64_t* len, int nlist,
                                                    int64_t* new_len, int64_t* nmoves) {
    __shared__ int64_t wsum[RM_WG / 64];
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const int64_t L = len[l];
        const uint32_t* mw = mask + (base[l] >> 5);
        const int64_t nw = (L + 31) >> 5;
        int64_t c = 0;
        for (int64_t w = threadIdx.x; w < nw; w += RM_WG) c += __popc(mw[w] & rm_range_bits(w, 0, L));
        const int64_t nl = L - rm_block_sum(c, wsum);
        int64_t cb = 0;
        for (int64_t w = threadIdx.x; w < ((nl + 31) >> 5); w += RM_WG) cb += __popc(mw[w] & rm_range_bits(w, 0, nl));
        const int64_t below = rm_block_sum(cb, wsum);
        if (threadIdx.x == 0) { new_len[l] = nl; nmoves[l] = below; }
    }
}

// one workgroup: off[i] = v[0] + ... + v[i - 1] for i <= n (off[n] = the total)
__global__ __launch_bounds__(RM_WG) void k_rm_offsets(const int64_t* v, int64_t n, int64_t* off) {
    __shared__ int64_t wsum[RM_WG / 64];
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < n; t0 += RM_WG) {
        const int64_t i = t0 + threadIdx.x;
        int64_t tot;
        const int64_t ex = rm_block_scan(i < n ? v[i] : 0, wsum, &tot);
        if (i < n) off[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) off[n] = carry;
}

// the (source slot, destination slot) pairs of every list at move_off[l]: hole t (ascending) <- kept tail entry t (descending)
__global__ __launch_bounds__(RM_WG) void k_rm_plan(const uint32_t* mask, const int64_t* base, const int64_t* len, const int64_t* new_len,
                                                   const int64_t* nmoves, const int64_t* move_off, int nlist, uint32_t* move_src,
                                                   uint32_t* move_dst) {
    __shared__ int64_t wsum[RM_WG / 64];
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const int64_t K = nmoves[l];
        if (K == 0) continue;                         // uniform over the workgroup
        const int64_t B = base[l], L = len[l], nl = new_len[l], off = move_off[l];
        const uint32_t* mw = mask + (B >> 5);
        for (int part = 0; part < 2; part++) {        // 0: holes in [0, nl); 1: kept entries in [nl, L)
            const int64_t lo = part ? nl : 0, hi = part ? L : nl;
            int64_t carry = 0;
            for (int64_t w0 = lo >> 5; w0 < ((hi + 31) >> 5); w0 += RM_WG) {
                const int64_t w = w0 + threadIdx.x;
                uint32_t bits = 0u;
                if (w < ((hi + 31) >> 5)) bits = (part ? ~mw[w] : mw[w]) & rm_range_bits(w, lo, hi);
                int64_t tot;
                int64_t r = carry + rm_block_scan(__popc(bits), wsum, &tot);
                while (bits) {
                    const int b = __ffs(bits) - 1;
                    bits &= bits - 1u;
                    const uint32_t slot = (uint32_t)(B + w * 32 + b);
                    if (part == 0) move_dst[off + r] = slot;
                    else move_src[off + (K - 1 - r)] = slot;
                    r++;
                }
                carry += tot;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// IVF moves and the clearing of the vacated slots
// ---------------------------------------------------------------------------------------
// raw rows (IVF-Flat): one thread per 16-byte piece of a moved row; the piece-0 thread also moves the id and the norm
__global__ __launch_bounds__(RM_WG) void k_rm_move_rows(const uint32_t* move_src, const uint32_t* move_dst, const int64_t* nmoves_total,
                                                        uint8_t* data, int64_t row_bytes, int64_t* ids, float* norms) {
    const int64_t cpr = row_bytes / 16, n = *nmoves_total * cpr;
    for (int64_t i = (int64_t)blockIdx.x * RM_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * RM_WG) {
        const int64_t mv = i / cpr, c = i - mv * cpr;
        const int64_t s = move_src[mv], d = move_dst[mv];
        *reinterpret_cast<uint4*>(data + d * row_bytes + c * 16) = *reinterpret_cast<const uint4*>(data + s * row_bytes + c * 16);
        if (c == 0) {
            if (ids) ids[d] = ids[s];
            if (norms) norms[d] = norms[s];
        }
    }
}

// PQ codes: one thread per code byte, addressed through the layout (rotated and sliced layouts place a byte by its row);
// consecutive threads hold consecutive sub-quantisers of one vector, so a wave's bytes fall in a few 16-byte pieces
__global__ __launch_bounds__(RM_WG) void k_rm_move_pq(const uint32_t* move_src, const uint32_t* move_dst, const int64_t* nmoves_total,
                                                      uint8_t* codes, int Mpad, int CB, int64_t* ids) {
    const int64_t n = *nmoves_total * Mpad;
    for (int64_t i = (int64_t)blockIdx.x * RM_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * RM_WG) {
        const int64_t mv = i / Mpad;
        const int m = (int)(i - mv * Mpad);
        const int64_t s = move_src[mv], d = move_dst[mv];
        codes[pq_code_addr(d, m, Mpad, CB)] = codes[pq_code_addr(s, m, Mpad, CB)];
        if (m == 0) ids[d] = ids[s];
    }
}

// vacated slots back to what a fresh allocation holds (zero bytes, zero norms; ids -1): one workgroup per (first slot, count) run
__global__ __launch_bounds__(RM_WG) void k_rm_clear(const int64_t* runs, int64_t nruns, uint8_t* data, int64_t row_bytes, int pq, int Mpad,
                                                    int CB, int64_t* ids, float* norms) {
    for (int64_t r = blockIdx.x; r < nruns; r += gridDim.x) {
        const int64_t s0 = runs[2 * r], cnt = runs[2 * r + 1];
        const int64_t units = pq ? (int64_t)Mpad : row_bytes / 16;
        for (int64_t i = threadIdx.x; i < cnt * units; i += RM_WG) {
            const int64_t row = s0 + i / units, u = i % units;
            if (pq) data[pq_code_addr(row, (int)u, Mpad, CB)] = 0;
            else *reinterpret_cast<uint4*>(data + row * row_bytes + u * 16) = make_uint4(0u, 0u, 0u, 0u);
            if (u == 0) {
                if (ids) ids[row] = -1;
                if (norms) norms[row] = 0.0f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Flat: stable compaction
// ---------------------------------------------------------------------------------------
// kept rows before a slot: blk_off[slot >> 13] + word_pre[slot >> 5] + the kept bits below it in its word
// (a workgroup scans the 256 words of 8192 consecutive slots)
constexpr int64_t RM_FLAT_BLK = 32 * RM_WG;

__global__ __launch_bounds__(RM_WG) void k_rm_flat_scan(const uint32_t* mask, int64_t n, int32_t* word_pre, int64_t* blk_cnt) {
    __shared__ int64_t wsum[RM_WG / 64];
    const int64_t nw = (n + 31) >> 5;
    for (int64_t b = blockIdx.x; b * RM_WG < nw; b += gridDim.x) {
        const int64_t w = b * RM_WG + threadIdx.x;
        const uint32_t kept = w < nw ? ~mask[w] & rm_range_bits(w, 0, n) : 0u;
        int64_t tot;
        const int64_t ex = rm_block_scan(__popc(kept), wsum, &tot);
        if (w < nw) word_pre[w] = (int32_t)ex;
        if (threadIdx.x == 0) blk_cnt[b] = tot;
    }
}

__device__ inline int64_t rm_kept_before(const uint32_t* mask, const int32_t* word_pre, const int64_t* blk_off, int64_t slot) {
    const int64_t w = slot >> 5;
    return blk_off[slot / RM_FLAT_BLK] + word_pre[w] + __popc(~mask[w] & ((1u << (slot & 31)) - 1u));
}

// the kept rows of source slots [lo, hi) (lo, hi multiples of RM_FLAT_BLK or hi = n) compacted into out rows 0, 1, ...;
// a chunk that no earlier removal shifts and that loses no row is skipped (its rows are already in place)
__global__ __launch_bounds__(RM_WG) void k_rm_flat_gather(const uint32_t* mask, const int32_t* word_pre, const int64_t* blk_off, int64_t lo,
                                                          int64_t hi, const uint8_t* data, int64_t row_bytes, const int64_t* ids,
                                                          const float* norms, uint8_t* out, int64_t* out_ids, float* out_norms) {
    const int64_t k_lo = blk_off[lo / RM_FLAT_BLK], k_hi = blk_off[(hi + RM_FLAT_BLK - 1) / RM_FLAT_BLK];
    if (k_lo == lo && k_hi - k_lo == hi - lo) return;
    const int64_t cpr = row_bytes / 16, n = (hi - lo) * cpr;
    for (int64_t i = (int64_t)blockIdx.x * RM_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * RM_WG) {
        const int64_t s = lo + i / cpr, c = i % cpr;
        if ((mask[s >> 5] >> (s & 31)) & 1u) continue;
        const int64_t d = rm_kept_before(mask, word_pre, blk_off, s) - k_lo;
        *reinterpret_cast<uint4*>(out + d * row_bytes + c * 16) = *reinterpret_cast<const uint4*>(data + s * row_bytes + c * 16);
        if (c == 0) {
            if (ids) out_ids[d] = ids[s];
            if (norms) out_norms[d] = norms[s];
        }
    }
}

// ... and the staged rows to their destinations (rows k_lo .. k_hi - 1 of the storage)
__global__ __launch_bounds__(RM_WG) void k_rm_flat_put(const int64_t* blk_off, int64_t lo, int64_t hi, const uint8_t* stage, int64_t row_bytes,
                                                       const int64_t* stage_ids, const float* stage_norms, uint8_t* data, int64_t* ids,
                                                       float* norms) {
    const int64_t k_lo = blk_off[lo / RM_FLAT_BLK], k_hi = blk_off[(hi + RM_FLAT_BLK - 1) / RM_FLAT_BLK];
    if (k_lo == lo && k_hi - k_lo == hi - lo) return;
    const int64_t cpr = row_bytes / 16, n = (k_hi - k_lo) * cpr;
    for (int64_t i = (int64_t)blockIdx.x * RM_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * RM_WG) {
        const int64_t r = i / cpr, c = i % cpr;
        *reinterpret_cast<uint4*>(data + (k_lo + r) * row_bytes + c * 16) = *reinterpret_cast<const uint4*>(stage + r * row_bytes + c * 16);
        if (c == 0) {
            if (ids) ids[k_lo + r] = stage_ids[r];
            if (norms) norms[k_lo + r] = stage_norms[r];
        }
    }
}

// ---------------------------------------------------------------------------------------
// launchers (rsx_host.h)
// ---------------------------------------------------------------------------------------
static inline unsigned rm_grid(int64_t work, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + RM_WG - 1) / RM_WG, cap)); }

void launch_rm_ivf_plan_counts(const uint32_t* mask, const int64_t* base, const int64_t* len, int nlist, int64_t* new_len, int64_t* nmoves,
                               int64_t* move_off, hipStream_t st) {
    hipLaunchKernelGGL(k_rm_count, dim3((unsigned)std::min(nlist, 8192)), dim3(RM_WG), 0, st, mask, base, len, nlist, new_len, nmoves);
    hipLaunchKernelGGL(k_rm_offsets, dim3(1), dim3(RM_WG), 0, st, nmoves, (int64_t)nlist, move_off);
}
void launch_rm_ivf_plan_moves(const uint32_t* mask, const int64_t* base, const int64_t* len, const int64_t* new_len, const int64_t* nmoves,
                              const int64_t* move_off, int nlist, uint32_t* move_src, uint32_t* move_dst, hipStream_t st) {
    hipLaunchKernelGGL(k_rm_plan, dim3((unsigned)std::min(nlist, 8192)), dim3(RM_WG), 0, st, mask, base, len, new_len, nmoves, move_off, nlist,
                       move_src, move_dst);
}
void launch_rm_ivf_move(const uint32_t* move_src, const uint32_t* move_dst, const int64_t* nmoves_total, int64_t max_moves, uint8_t* data,
                        int64_t row_bytes, int pq, int Mpad, int CB, int64_t* ids, float* norms, hipStream_t st) {
    if (max_moves <= 0) return;
    if (pq) hipLaunchKernelGGL(k_rm_move_pq, dim3(rm_grid(max_moves * Mpad, 65536)), dim3(RM_WG), 0, st, move_src, move_dst, nmoves_total,
                               data, Mpad, CB, ids);
    else hipLaunchKernelGGL(k_rm_move_rows, dim3(rm_grid(max_moves * (row_bytes / 16), 65536)), dim3(RM_WG), 0, st, move_src, move_dst,
                            nmoves_total, data, row_bytes, ids, norms);
}
void launch_rm_clear(const int64_t* runs, int64_t nruns, uint8_t* data, int64_t row_bytes, int pq, int Mpad, int CB, int64_t* ids, float* norms,
                     hipStream_t st) {
    if (nruns <= 0) return;
    hipLaunchKernelGGL(k_rm_clear, dim3((unsigned)std::min<int64_t>(nruns, 65536)), dim3(RM_WG), 0, st, runs, nruns, data, row_bytes, pq, Mpad,
                       CB, ids, norms);
}
int64_t rm_flat_blocks(int64_t n) { return (n + RM_FLAT_BLK - 1) / RM_FLAT_BLK; }
int64_t rm_flat_unit() { return RM_FLAT_BLK; }
void launch_rm_flat_scan(const uint32_t* mask, int64_t n, int32_t* word_pre, int64_t* blk_cnt, int64_t* blk_off, hipStream_t st) {
    const int64_t nb = rm_flat_blocks(n);
    hipLaunchKernelGGL(k_rm_flat_scan, dim3((unsigned)std::min<int64_t>(std::max<int64_t>(nb, 1), 65536)), dim3(RM_WG), 0, st, mask, n, word_pre,
                       blk_cnt);
    hipLaunchKernelGGL(k_rm_offsets, dim3(1), dim3(RM_WG), 0, st, blk_cnt, nb, blk_off);
}
void launch_rm_flat_chunk(const uint32_t* mask, const int32_t* word_pre, const int64_t* blk_off, int64_t lo, int64_t hi, uint8_t* data,
                          int64_t row_bytes, int64_t* ids, float* norms, uint8_t* stage, int64_t* stage_ids, float* stage_norms, hipStream_t st) {
    const unsigned g = rm_grid((hi - lo) * (row_bytes / 16), 16384);
    hipLaunchKernelGGL(k_rm_flat_gather, dim3(g), dim3(RM_WG), 0, st, mask, word_pre, blk_off, lo, hi, data, row_bytes, ids, norms, stage,
                       stage_ids, stage_norms);
    hipLaunchKernelGGL(k_rm_flat_put, dim3(g), dim3(RM_WG), 0, st, blk_off, lo, hi, stage, row_bytes, stage_ids, stage_norms, data, ids, norms);
}

}  // namespace rsx
