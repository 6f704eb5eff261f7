// rsx_sel.h — filtered search (k_sel.hip): the slot mask of an id selector and -inf written over the masked columns of score rows.
// Only a filtered search (rsx_search_sel) launches these kernels.
#pragma once
#include "rsx_internal.h"

namespace rsx {
// kind: include/rsx.h rsx_selector_kind
struct SelDevArgs {
    int kind; int invert; int64_t lo, hi;
    const uint8_t* bitmap; int64_t nbytes;
    const int64_t* ids; int64_t nids;
};
// mask: 2 * ceil(nslots / 64) words (one 64-slot ballot per wave)
inline int64_t sel_mask_words(int64_t nslots) { return 2 * ((nslots + 63) / 64); }
void launch_sel_mask(const SelDevArgs& s, const int64_t* slot_ids, int64_t nslots, uint32_t* mask, hipStream_t st);
// flat_n >= 0: Flat, column c of a row = slot slot0 + c, c < flat_n; flat_n < 0: IVF segments (seg_start / probe_list) as k_exact_scores
// and the list scans lay them out
struct SelApplyArgs {
    float* temp; int64_t tstride; int64_t nq; const uint32_t* mask;
    int64_t flat_n; int64_t slot0;
    const int32_t* probe_list; const int64_t* seg_start; int nprobe; const int64_t* list_base; const int64_t* list_len;
};
void launch_sel_apply(const SelApplyArgs& a, hipStream_t st);
}  // namespace rsx
