// rsx_range.h — range search (faiss Index::range_search): the launch interface of k_range.hip, the library-owned result
// object behind rsx_range_result_t (include/rsx.h) and the host driver's entry (api_range.hip).
#pragma once
#include "rsx_stages.h"

namespace rsx {

// Per query: |q| and the threshold of the fixed-threshold scans, as a candidate key (k_range_tau; derivation beside the kernel).  Also
// resets the query's candidate counter.
struct RangeTauArgs {
    const float* Q32; int ldq; int d; int64_t nq;
    int metric; float radius;
    float cert_rel, cert_rel_qlossy, cert_xmax, cert_abs; const int* cert_qflag;     // the scan's error bound (scan_cert_bound), as FinalizeArgs carries it
    uint64_t* tau;                       // [nq] out
    unsigned long long* cand_cnt;        // [nq * CCS] out: zeroed
};
void launch_range_tau(const RangeTauArgs& a, hipStream_t st);

// Candidate rows of one scan: row r holds rcnt[r] keys (approximate score, index) in cand[r * cap ..); the row belongs to query
// qsel[r] of the batch (null: r).  cap is a power of two.
struct RangeRowsArgs {
    uint64_t* cand; int cap; int64_t nrows;
    const int32_t* rcnt; const int32_t* qsel;
    int kind; int metric; float radius;
    const float* Q32; int ldq; int d;
    const void* X; int x_f16; int ld;
    const int32_t* probe_list; const int64_t* seg_start; int nprobe; const int64_t* list_base;      // IVF: a key's index is a column of the query's row
    const int64_t* ids;                  // per storage row, or null (id = row)
    int32_t* nmem;                       // [batch queries] += members of the row
    int max_cnt;                         // the largest rcnt (sizes the grid)
};
// exact re-score + membership, in place: a member's key becomes (exact order word, index), every other slot below the row's power of two 0
void launch_range_rescore(const RangeRowsArgs& a, hipStream_t st);
// every row's first pow2ceil(rcnt) keys in descending order: the members first, best first (ties by index)
void launch_range_sort(const RangeRowsArgs& a, hipStream_t st);
// lims[0] = base, lims[i + 1] = base + nmem[0] + ... + nmem[i]
void launch_range_lims(const int32_t* nmem, int64_t nq, int64_t base, int64_t* lims, hipStream_t st);
// the members of rows [0, nrows) laid end to end: dst[koff[r] + j] = cand[r * cap + j], j < nmem[qsel[r]]
void launch_range_compact(const RangeRowsArgs& a, const int64_t* koff, uint64_t* dst, hipStream_t st);
// D / I of the batch: query q's nmem[q] sorted keys at kptr[q] go to position lims[q] - lims[0] of the batch's output.  With explicit ids the
// keys are replaced by the ids and launch_range_ties reorders the runs of equal scores by id.
struct RangeEmitArgs {
    uint64_t* const* kptr; const int32_t* nmem; const int64_t* lims; int64_t nq;
    int kind; int metric;
    const int32_t* probe_list; const int64_t* seg_start; int nprobe; const int64_t* list_base; const int64_t* ids;
    float* D; int64_t* I;
    int max_cnt;
};
void launch_range_emit(const RangeEmitArgs& a, hipStream_t st);
void launch_range_ties(const RangeEmitArgs& a, hipStream_t st);
// dst row i = src row sel[i]; rows of row_bytes (a multiple of 4)
void launch_range_gather_rows(const void* src, void* dst, int64_t row_bytes, const int32_t* sel, int64_t n, hipStream_t st);

}  // namespace rsx

// faiss RangeSearchResult: lims [nq + 1], then the distances and labels of all queries end to end.  Device memory (of `device`) when the
// queries were a device pointer, else host memory.
struct rsx_range_result {
    int64_t nq = 0, total = 0;
    int on_device = 0, device = 0;
    std::vector<int64_t> h_lims; std::vector<float> h_D; std::vector<int64_t> h_I;
    std::unique_ptr<DevBuf> d_lims, d_D, d_I;
};

rsx_range_result* range_impl(rsx_index* h, int64_t nq, const void* q, int dtype, float radius);
