// k_reconstruct.hip — rsx_reconstruct_batch: stored vectors by id, gathered and decoded on the GPU (FAISS: Index::reconstruct_batch,
// IndexIVF::reconstruct_from_offset, ProductQuantizer::decode, ScalarQuantizer::decode), and the builds of the direct map that turns an id
// into a storage row (rsx_reconstruct.h; FAISS: DirectMap).
//   k_reconstruct    one wave per key: resolve the row (bounds check / array load / hash probe), decode it into d consecutive floats of
//                    the output — coalesced stores, 16-byte accesses where the row format allows them.  A key that is not stored
//                    dereferences nothing: its output row is all-ones words and (unless it is a negative key in fill mode) the call's
//                    page-locked miss word is raised and the lowest missing position recorded.
//   k_dm_array_build / k_dm_hash_build    one thread per storage row of the list directory's valid rows.
#include "rsx_internal.h"
#include "k_sq.h"
#include "rsx_reconstruct.h"

namespace rsx {

// the storage row of a key, -1 when no stored vector has that id (keys < 0 are never looked up)
__device__ __forceinline__ int64_t rc_resolve(const ReconArgs& a, int64_t key) {
    if (key < 0) return -1;
    unsigned long long r;
    if (a.mode == RC_DIRECT) return key < a.ntotal ? key : -1;
    if (a.mode == RC_ARRAY) r = key < a.map_n ? a.map[key] : DM_NO_ROW;
    else r = dm_hash_find(a.map, (uint64_t)a.map_n - 1, key);
    return r == DM_NO_ROW ? -1 : (int64_t)r;
}

// vec: the 16-byte form of the row format applies (launch_reconstruct: d / dsub divisible, output 16-byte aligned)
template <int FMT>
__global__ __launch_bounds__(256) void k_reconstruct(ReconArgs a, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // wave-uniform: one key per wave
    if (i >= a.n) return;
    const int d = a.d;
    const int64_t key = a.keys[i];
    const int64_t row = rc_resolve(a, key);
    float* o = a.out + i * d;
    if (row < 0) {
        const float ones = __uint_as_float(0xFFFFFFFFu);      // FAISS search_and_reconstruct: memset(-1) for a label of -1
        for (int t = lane; t < d; t += 64) o[t] = ones;
        if (!(key < 0 && a.fill_negative) && lane == 0) {
            *a.miss_flag = 1;
            atomicMin(a.miss_first, (unsigned long long)(a.pos0 + i));
        }
        return;
    }
    if (FMT == RC_ROWS_F16) {
        const __half* x = reinterpret_cast<const __half*>(a.data) + row * a.ld;
        if (vec) {
            for (int t = 8 * lane; t < d; t += 512) {
                const uint4 w = *reinterpret_cast<const uint4*>(x + t);
                const __half2* h2 = reinterpret_cast<const __half2*>(&w);
                const float2 f0 = __half22float2(h2[0]), f1 = __half22float2(h2[1]), f2 = __half22float2(h2[2]), f3 = __half22float2(h2[3]);
                *reinterpret_cast<float4*>(o + t) = make_float4(f0.x, f0.y, f1.x, f1.y);
                *reinterpret_cast<float4*>(o + t + 4) = make_float4(f2.x, f2.y, f3.x, f3.y);
            }
        } else {
            for (int t = lane; t < d; t += 64) o[t] = __half2float(x[t]);
        }
    } else if (FMT == RC_ROWS_F32) {
        const float* x = reinterpret_cast<const float*>(a.data) + row * a.ld;
        if (vec) { for (int t = 4 * lane; t < d; t += 256) *reinterpret_cast<float4*>(o + t) = *reinterpret_cast<const float4*>(x + t); }
        else { for (int t = lane; t < d; t += 64) o[t] = x[t]; }
    } else {
        const SqRows dir{nullptr, nullptr, nullptr, a.list_base, a.nlist};
        const float* cen = a.centroids ? a.centroids + (int64_t)sq_list_of_row(dir, row) * d : nullptr;
        if (FMT == RC_PQ) {
            // x^_j = c_list[j] + cb[m][code_m][t], j = m dsub + t: one fp32 add (nothing to contract); IndexPQ (cen null) adds nothing
            const uint8_t* codes = reinterpret_cast<const uint8_t*>(a.data);
            const int dsub = a.dsub;
            if (vec) {
                for (int t4 = 4 * lane; t4 < d; t4 += 256) {
                    const int m = t4 / dsub, t = t4 - m * dsub;
                    const uint32_t code = codes[pq_code_addr(row, m, a.Mpad, a.CB)];
                    float4 v = *reinterpret_cast<const float4*>(a.codebooks + ((int64_t)m * 256 + code) * dsub + t);
                    if (cen) {
                        const float4 c = *reinterpret_cast<const float4*>(cen + t4);
                        v.x = c.x + v.x; v.y = c.y + v.y; v.z = c.z + v.z; v.w = c.w + v.w;
                    }
                    *reinterpret_cast<float4*>(o + t4) = v;
                }
            } else {
                for (int j = lane; j < d; j += 64) {
                    const int m = j / dsub, t = j - m * dsub;
                    const uint32_t code = codes[pq_code_addr(row, m, a.Mpad, a.CB)];
                    const float v = a.codebooks[((int64_t)m * 256 + code) * dsub + t];
                    o[j] = cen ? cen[j] + v : v;
                }
            }
        } else {
            // a 4-byte word of the code row per lane; k_sq.h's decode (contraction off), the centroid added and the sum rounded once
            const uint8_t* x = reinterpret_cast<const uint8_t*>(a.data) + row * a.ld;
            for (int t4 = 4 * lane; t4 < d; t4 += 256) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(x + t4);
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = t4 + e < d ? sq_xhat((w >> (8 * e)) & 255u, a.trained, cen, d, t4 + e) : 0.0f;
                if (vec) *reinterpret_cast<float4*>(o + t4) = make_float4(v[0], v[1], v[2], v[3]);
                else {
#pragma unroll
                    for (int e = 0; e < 4; e++) if (t4 + e < d) o[t4 + e] = v[e];
                }
            }
        }
    }
}

void launch_reconstruct(const ReconArgs& a, hipStream_t st) {
    if (a.n <= 0) return;
    const bool al16 = (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
    const dim3 grid((unsigned)((a.n + 3) / 4)), block(256);
    switch (a.fmt) {
        case RC_ROWS_F16: hipLaunchKernelGGL(k_reconstruct<RC_ROWS_F16>, grid, block, 0, st, a, (int)(al16 && a.d % 8 == 0)); break;
        case RC_ROWS_F32: hipLaunchKernelGGL(k_reconstruct<RC_ROWS_F32>, grid, block, 0, st, a, (int)(al16 && a.d % 4 == 0)); break;
        case RC_PQ:       hipLaunchKernelGGL(k_reconstruct<RC_PQ>, grid, block, 0, st, a, (int)(al16 && a.dsub % 4 == 0)); break;
        default:          hipLaunchKernelGGL(k_reconstruct<RC_SQ>, grid, block, 0, st, a, (int)(al16 && a.d % 4 == 0)); break;
    }
}

// ---- direct map builds ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dm_fill(unsigned long long* p, int64_t nwords, unsigned long long even, unsigned long long odd) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (int64_t)gridDim.x * 256) p[i] = (i & 1) ? odd : even;
}
// row holds a stored vector: it lies inside the length of the list that owns it
__device__ __forceinline__ bool dm_row_valid(const int64_t* list_base, const int64_t* list_len, int nlist, int64_t row) {
    const SqRows dir{nullptr, nullptr, nullptr, list_base, nlist};
    const int l = sq_list_of_row(dir, row);
    return row >= list_base[l] && row - list_base[l] < list_len[l];
}
// Array: map[id] = the lowest row of id; *flag is raised by an id outside [0, map_n) and by a slot hit twice (the build then falls back)
__global__ __launch_bounds__(256) void k_dm_array_build(const int64_t* ids, const int64_t* list_base, const int64_t* list_len, int nlist,
                                                        int64_t total_rows, unsigned long long* map, int64_t map_n, int* flag) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < total_rows; r += (int64_t)gridDim.x * 256) {
        if (!dm_row_valid(list_base, list_len, nlist, r)) continue;
        const int64_t id = ids[r];
        if (id < 0 || id >= map_n) { *flag = 1; continue; }
        if (atomicMin(&map[id], (unsigned long long)r) != DM_NO_ROW) *flag = 1;
    }
}
// Hashtable: the id word of a slot is claimed by compare-and-swap, the row word takes the minimum (dm_hash_insert_seq, with atomics).
// *flag is raised by the id INT64_MIN (the free-slot word) and by a table without a free slot (cannot happen at load <= 1/2).
__global__ __launch_bounds__(256) void k_dm_hash_build(const int64_t* ids, const int64_t* list_base, const int64_t* list_len, int nlist,
                                                       int64_t total_rows, unsigned long long* tab, uint64_t mask, int* flag) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < total_rows; r += (int64_t)gridDim.x * 256) {
        if (!dm_row_valid(list_base, list_len, nlist, r)) continue;
        const unsigned long long id = (unsigned long long)ids[r];
        if (id == DM_EMPTY) { *flag = 1; continue; }
        uint64_t s = dm_hash_slot((int64_t)id, mask);
        bool placed = false;
        for (uint64_t n = 0; n <= mask && !placed; n++, s = dm_hash_next(s, mask)) {
            const unsigned long long prev = atomicCAS(&tab[2 * s], DM_EMPTY, id);
            if (prev == DM_EMPTY || prev == id) { atomicMin(&tab[2 * s + 1], (unsigned long long)r); placed = true; }
        }
        if (!placed) *flag = 1;
    }
}

static inline unsigned dm_grid(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 65536); }
void launch_dm_fill(unsigned long long* p, int64_t nwords, unsigned long long even, unsigned long long odd, hipStream_t st) {
    if (nwords > 0) hipLaunchKernelGGL(k_dm_fill, dim3(dm_grid(nwords)), dim3(256), 0, st, p, nwords, even, odd);
}
void launch_dm_array_build(const int64_t* ids, const int64_t* list_base, const int64_t* list_len, int nlist, int64_t total_rows, unsigned long long* map,
                           int64_t map_n, int* flag, hipStream_t st) {
    if (total_rows > 0) hipLaunchKernelGGL(k_dm_array_build, dim3(dm_grid(total_rows)), dim3(256), 0, st, ids, list_base, list_len, nlist, total_rows, map, map_n, flag);
}
void launch_dm_hash_build(const int64_t* ids, const int64_t* list_base, const int64_t* list_len, int nlist, int64_t total_rows, unsigned long long* tab,
                          uint64_t mask, int* flag, hipStream_t st) {
    if (total_rows > 0) hipLaunchKernelGGL(k_dm_hash_build, dim3(dm_grid(total_rows)), dim3(256), 0, st, ids, list_base, list_len, nlist, total_rows, tab, mask, flag);
}

}  // namespace rsx
