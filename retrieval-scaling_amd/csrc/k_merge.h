// k_merge.h — rsx_merge_from / rsx_copy_subset_to: the plan records, the subset predicates and the row / byte mapping of the
// copy kernels (k_merge.hip) as __host__ __device__ functions, so that a host program can run the very functions the kernels run
// (tests/host/merge_check.hip).  All row and byte offsets are 64-bit.
#pragma once
#include <vector>
#include "rsx_internal.h"

namespace rsx {

// InvertedLists::subset_type_t of FAISS 1.8.0
enum { MG_SUBSET_ID_RANGE = 0, MG_SUBSET_ID_MOD = 1, MG_SUBSET_ELEMENT_RANGE = 2, MG_SUBSET_INVLIST_FRACTION = 3, MG_SUBSET_INVLIST = 4 };

constexpr int MG_TILE = 256;      // rows of one work item = one workgroup of the copy kernels

// One work item: n <= MG_TILE rows that arrive at destination storage rows dst .. dst + n - 1 of ONE list, in order.  sel = 0: they are
// the source storage rows src .. src + n - 1; sel = 1: source row j is sel_rows[src + j] (the subset forms: the selected rows of the
// list, compacted in list order by k_mg_fill).
struct MergeItem { int64_t src, dst; int32_t n, sel; };

__host__ __device__ inline int64_t mg_src_row(const MergeItem& it, int j, const uint32_t* sel_rows) {
    return it.sel ? (int64_t)sel_rows[it.src + j] : it.src + j;
}
__host__ __device__ inline int64_t mg_row_off(int64_t row, int64_t row_bytes) { return row * row_bytes; }

// IndexIVF::copy_subset_to, types 0 and 1: the test of one stored id (C++ remainder, as FAISS computes it: a negative id never matches)
__host__ __device__ inline bool mg_id_selected(int type, int64_t id, int64_t a1, int64_t a2) {
    return type == MG_SUBSET_ID_RANGE ? (id >= a1 && id < a2) : (id % a1 == a2);
}

// Type 2: FAISS's running split.  State accu[3] = {accu_n, accu_a1, accu_a2} starts at zero and is carried over the lists IN ORDER; a list
// of n entries contributes its positions [i1, i2).
inline void mg_element_range(int64_t n, int64_t nt, int64_t a1, int64_t a2, int64_t accu[3], int64_t& i1, int64_t& i2) {
    const int64_t next_n = accu[0] + n;
    const int64_t na1 = next_n * a1 / nt, na2 = next_n * a2 / nt;
    i1 = na1 - accu[1]; i2 = na2 - accu[2];
    accu[0] = next_n; accu[1] = na1; accu[2] = na2;
}

// The work items of one list's run of `count` rows: source first row (or first index into sel_rows) `src`, destination first row `dst`
inline void mg_push_items(std::vector<MergeItem>& items, int64_t src, int64_t dst, int64_t count, int sel) {
    for (int64_t j0 = 0; j0 < count; j0 += MG_TILE)
        items.push_back(MergeItem{src + j0, dst + j0, (int32_t)(count - j0 < MG_TILE ? count - j0 : MG_TILE), sel});
}

// IVF-PQ codes, the byte-wise form: thread t of an item (t < n * Mpad) owns byte m = t % Mpad of the item's row t / Mpad.  The byte is read
// where the SOURCE layout keeps (source row, m) and written where the DESTINATION layout keeps (destination row, m); the padding bytes
// m in [M, Mpad) are written as zero.  Source and destination layouts (CB: rsx_internal.h) and the rows' phases inside their blocks,
// slabs or 512-row groups are independent.
__host__ __device__ inline void mg_pq_byte(const MergeItem& it, int64_t t, const uint32_t* sel_rows, const uint8_t* scodes, uint8_t* dcodes,
                                           int M, int Mpad, int CBs, int CBd) {
    const int j = (int)(t / Mpad), m = (int)(t - (int64_t)j * Mpad);
    const uint8_t v = m < M ? scodes[pq_code_addr(mg_src_row(it, j, sel_rows), m, Mpad, CBs)] : (uint8_t)0;
    dcodes[pq_code_addr(it.dst + j, m, Mpad, CBd)] = v;
}

// IVF-PQ codes, the 16-byte form (both layouts keep the 16 sub-quantisers 16 r .. 16 r + 15 of a row together: every layout but the
// 4-byte granule).  The granule layout stores such a run in m order; the rotated and sliced layouts store it rotated by the row's phase
// i = row & 15 (byte s of the piece holds m = 16 r + ((i + s) & 15)), as one 16-byte piece or, in the rotated layout's trailing half
// phase, as two 8-byte pieces of lane groups two apart.  In every case the 8 bytes from position 0 start where (row, 16 r + i) lies and
// the 8 bytes from position 8 where (row, 16 r + ((i + 8) & 15)) lies.
__host__ __device__ inline bool mg_pq_runs_apply(int CBs, int CBd) { return CBs != 4 && CBd != 4; }
__host__ __device__ inline int mg_pq_phase(int64_t row, int CB) { return pq_rot_family(CB) ? (int)(row & 15) : 0; }
// byte t of the result = byte (t - i) & 15 of the input (i in 0 .. 15)
__host__ __device__ inline void mg_rot16(uint32_t (&w)[4], int i) {
    const int wi = i >> 2, bi = i & 3;
    if (wi & 1) { const uint32_t t = w[3]; w[3] = w[2]; w[2] = w[1]; w[1] = w[0]; w[0] = t; }
    if (wi & 2) { uint32_t t = w[0]; w[0] = w[2]; w[2] = t; t = w[1]; w[1] = w[3]; w[3] = t; }
    if (bi) {
        const int l = 8 * bi, r = 32 - l;
        const uint32_t r0 = (w[0] << l) | (w[3] >> r), r1 = (w[1] << l) | (w[0] >> r), r2 = (w[2] << l) | (w[1] >> r), r3 = (w[3] << l) | (w[2] >> r);
        w[0] = r0; w[1] = r1; w[2] = r2; w[3] = r3;
    }
}
// Thread t of an item (t < n * Mpad / 16) owns run t / n of the item's row t % n (rows fastest: neighbouring lanes touch neighbouring
// 16-byte pieces in every layout): two 8-byte loads, one rotation by the difference of the two rows' phases, two 8-byte stores.
// A run that reaches past M (granule to granule only: the other layouts have M = Mpad) has its bytes m >= M cleared.
__host__ __device__ inline void mg_pq_run(const MergeItem& it, int64_t t, const uint32_t* sel_rows, const uint8_t* scodes, uint8_t* dcodes,
                                          int M, int Mpad, int CBs, int CBd) {
    const int r = (int)(t / it.n), j = (int)(t - (int64_t)r * it.n);
    const int64_t srow = mg_src_row(it, j, sel_rows), drow = it.dst + j;
    const int is = mg_pq_phase(srow, CBs), id = mg_pq_phase(drow, CBd);
    const uint2 a = *reinterpret_cast<const uint2*>(scodes + pq_code_addr(srow, 16 * r + is, Mpad, CBs));
    const uint2 b = *reinterpret_cast<const uint2*>(scodes + pq_code_addr(srow, 16 * r + ((is + 8) & 15), Mpad, CBs));
    uint32_t w[4] = {a.x, a.y, b.x, b.y};
    mg_rot16(w, (is - id) & 15);
    if (16 * r + 16 > M) {      // (phases 0 on both sides: the words are in m order)
        for (int k = 0; k < 4; k++) {
            const int keep = M - 16 * r - 4 * k;      // bytes of word k below M
            w[k] = keep >= 4 ? w[k] : keep <= 0 ? 0u : (w[k] & ((1u << (8 * keep)) - 1u));
        }
    }
    *reinterpret_cast<uint2*>(dcodes + pq_code_addr(drow, 16 * r + id, Mpad, CBd)) = make_uint2(w[0], w[1]);
    *reinterpret_cast<uint2*>(dcodes + pq_code_addr(drow, 16 * r + ((id + 8) & 15), Mpad, CBd)) = make_uint2(w[2], w[3]);
}

// k_merge.hip.  All asynchronous on `st`.
// selected entries per list (types 0 / 1): cnt[l]
void launch_mg_count(const int64_t* ids, const int64_t* base, const int64_t* len, int nlist, int type, int64_t a1, int64_t a2, int64_t* cnt,
                     hipStream_t st);
// ... and their storage rows in list order: sel_rows[off[l] .. off[l] + cnt[l])
void launch_mg_fill(const int64_t* ids, const int64_t* base, const int64_t* len, int nlist, int type, int64_t a1, int64_t a2, const int64_t* off,
                    uint32_t* sel_rows, hipStream_t st);
// rows of srb bytes (a multiple of 16) to rows of drb bytes: drb == srb copies, widen (drb == 2 srb) turns fp16 rows into fp32 rows.
// sids / snorms may be null (no ids / norm terms to move); stored ids are sids + add_id.
void launch_mg_rows(const MergeItem* items, int64_t nitems, const uint32_t* sel_rows, const uint8_t* sdata, uint8_t* ddata, int64_t srb,
                    int64_t drb, int widen, const int64_t* sids, int64_t* dids, int64_t add_id, const float* snorms, float* dnorms, hipStream_t st);
void launch_mg_pq(const MergeItem* items, int64_t nitems, const uint32_t* sel_rows, const uint8_t* scodes, uint8_t* dcodes, int M, int Mpad,
                  int CBs, int CBd, const int64_t* sids, int64_t* dids, int64_t add_id, hipStream_t st);

}  // namespace rsx
