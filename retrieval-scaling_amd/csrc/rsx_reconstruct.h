// rsx_reconstruct.h — the direct map of rsx_reconstruct_batch: stored id -> storage row.  Two forms, as in FAISS's DirectMap:
//   Array      int64 map[n]: map[id] = row, DM_NO_ROW where no vector has that id.  Used when every stored id lies in [0, n) once.
//   Hashtable  open addressing over cap (id, row) slots of 16 bytes, cap a power of two >= 2 n: slot 2 s holds the id (DM_EMPTY = free),
//              slot 2 s + 1 the row.  An id probes dm_hash_slot(id), then dm_hash_next(...) until it meets itself or a free slot; an id
//              stored more than once keeps ONE slot, whose row is the lowest of its storage rows (insertion takes the minimum).
// The hash, the probe sequence, the lookup and a sequential insertion are __host__ __device__, so that tests/host/directmap_check.hip runs
// them on the host; the build kernels (k_reconstruct.hip) insert with the same sequence through atomics.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace rsx {

enum { DM_NONE = 0, DM_ARRAY = 1, DM_HASH = 2 };                       // rsx_get "direct_map_type" (= faiss DirectMap::Type)
constexpr unsigned long long DM_EMPTY = 0x8000000000000000ull;        // free hash slot: the id INT64_MIN is never stored in the map
constexpr unsigned long long DM_NO_ROW = ~0ull;                       // array entry / hash row word before any row arrived; lookup "not found"

// splitmix64's finaliser: consecutive and strided ids spread over the table
__host__ __device__ inline uint64_t dm_hash(int64_t id) {
    uint64_t z = (uint64_t)id + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t dm_hash_slot(int64_t id, uint64_t mask) { return dm_hash(id) & mask; }
__host__ __device__ inline uint64_t dm_hash_next(uint64_t slot, uint64_t mask) { return (slot + 1) & mask; }      // linear probing
// capacity of the table for n stored vectors: the power of two >= 2 n (at least 2): load <= 1/2, so a probe always meets a free slot
__host__ __device__ inline uint64_t dm_hash_capacity(int64_t n) {
    uint64_t cap = 2;
    while (cap < 2 * (uint64_t)(n > 0 ? n : 0)) cap <<= 1;
    return cap;
}

// Lookup: the row of `id`, DM_NO_ROW when the probe reaches a free slot first.  *steps (optional) counts the slots read.
__host__ __device__ inline unsigned long long dm_hash_find(const unsigned long long* tab, uint64_t mask, int64_t id, int* steps = nullptr) {
    if ((unsigned long long)id == DM_EMPTY) return DM_NO_ROW;
    uint64_t s = dm_hash_slot(id, mask);
    for (uint64_t n = 0; n <= mask; n++, s = dm_hash_next(s, mask)) {
        const unsigned long long key = tab[2 * s];
        if (steps) ++*steps;
        if (key == (unsigned long long)id) return tab[2 * s + 1];
        if (key == DM_EMPTY) return DM_NO_ROW;
    }
    return DM_NO_ROW;
}
// Sequential insertion (one thread; the reference the atomic insertion of k_dm_hash_build follows step by step).  false: no free slot.
__host__ __device__ inline bool dm_hash_insert_seq(unsigned long long* tab, uint64_t mask, int64_t id, unsigned long long row) {
    if ((unsigned long long)id == DM_EMPTY) return false;
    uint64_t s = dm_hash_slot(id, mask);
    for (uint64_t n = 0; n <= mask; n++, s = dm_hash_next(s, mask)) {
        const unsigned long long key = tab[2 * s];
        if (key == DM_EMPTY) { tab[2 * s] = (unsigned long long)id; tab[2 * s + 1] = row; return true; }
        if (key == (unsigned long long)id) { if (row < tab[2 * s + 1]) tab[2 * s + 1] = row; return true; }
    }
    return false;
}

// ---- k_reconstruct.hip ----------------------------------------------------------------------------------------------------------------
// What the gather-and-decode kernel needs of a handle.  mode: how a key becomes a storage row.
enum { RC_DIRECT = 0, RC_ARRAY = 1, RC_HASH = 2 };                     // DIRECT: the key IS the row (Flat / IndexPQ of sequential ids)
enum { RC_ROWS_F16 = 0, RC_ROWS_F32 = 1, RC_PQ = 2, RC_SQ = 3 };
struct ReconArgs {
    int mode, fmt, d, ld;
    int64_t n;                          // keys of this launch
    const int64_t* keys; float* out;    // out: [n, d] fp32
    int fill_negative;                  // keys < 0 give rows of all-ones words instead of a miss
    int64_t ntotal;                     // RC_DIRECT: rows are [0, ntotal)
    const unsigned long long* map; int64_t map_n;    // RC_ARRAY: map_n entries; RC_HASH: map_n slots (a power of two)
    const void* data;                   // rows (fp16 / fp32: ld elements; SQ: ld bytes) or PQ code slabs
    int M, Mpad, CB, dsub;              // RC_PQ
    const float* codebooks;             // RC_PQ: [M][256][dsub]
    const float* trained;               // RC_SQ: vmin[d], vdiff[d]
    const float* centroids;             // added to the decoded residual (IVF-PQ, by_residual IVF-SQ); null: nothing is added
    const int64_t* list_base; int nlist;             // the list directory (a row's list, where a centroid is added)
    int* miss_flag;                     // page-locked host word: raised by any miss
    unsigned long long* miss_first;     // device word: the lowest position (of the whole call) whose key missed (atomicMin)
    int64_t pos0;                       // position of keys[0] in the call
};
void launch_reconstruct(const ReconArgs& a, hipStream_t st);
// the map builds over the valid rows of the list directory (ids null: the row number is the id — never needed, kept for completeness)
void launch_dm_fill(unsigned long long* p, int64_t nwords, unsigned long long even, unsigned long long odd, hipStream_t st);
void launch_dm_array_build(const int64_t* ids, const int64_t* list_base, const int64_t* list_len, int nlist, int64_t total_rows, unsigned long long* map,
                           int64_t map_n, int* flag, hipStream_t st);
void launch_dm_hash_build(const int64_t* ids, const int64_t* list_base, const int64_t* list_len, int nlist, int64_t total_rows, unsigned long long* tab,
                          uint64_t mask, int* flag, hipStream_t st);

}  // namespace rsx
