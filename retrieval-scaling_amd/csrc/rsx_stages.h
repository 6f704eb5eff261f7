// rsx_stages.h — the stages of an internal batch that more than one driver runs (definitions: api_stages.hip): query conversion of the
// certified scans, the exact coarse stage, row selection, the pair grouping and the arguments of the list scans, the host-side bounds of
// the list directory, the error bound of the fp16-MFMA scans, the L2 ranking bias, a stream timer.  api_search.hip (search) and
// api_range.hip (range_search) are built from them; the batch plan and the routes of `search` stay in api_search.hip.
#pragma once
#include "rsx_host.h"

// (sum, max) of the nprobe largest values of ceil(len / unit) * scale over the lists (unit > 0), memoised per directory generation
std::pair<int64_t, int64_t> top_probe_sum(rsx_index* h, int nprobe, int unit, int scale);
// upper bound of the (list, tile, group) work items of a list-major scan with groups of G probing queries, without a host round trip
int64_t max_scan_items(rsx_index* h, int64_t nq, int nprobe, int G, int tile_rows);
// >= the largest centroid norm (the fast coarse quantiser's bound; certificate term of a by_residual scalar-quantiser index), once per centroid set
float cent_cmax(rsx_index* h);
// top-k of `nrows` rows of fp32 scores (row r valid length: row_n or n_max) into state [nrows, KP]
void select_rows(rsx_index* h, const float* scores, int64_t row_stride, const int64_t* row_n, int64_t row_n_stride, int64_t n_max,
                 uint32_t idx_base, int64_t nrows, int KP, int BUF, int k, uint64_t* state, bool merge_state,
                 unsigned long long* threshold_only_cnt = nullptr);
// |approx - exact| of the fp16-MFMA scans of Flat / IVF-Flat rows for ANY stored vector, which k_finalize's certificate and k_range_tau
// combine as  rel |q| xmax + abs (|q| + xmax)  (rel_qlossy joins rel when the batch held a query value that fp16 does not represent)
struct ScanBound { float rel, rel_qlossy, xmax, abs; };
ScanBound scan_cert_bound(const rsx_index* h);

// the queries of a certified scan (Flat, IVF-Flat, IVF-SQ): fp32 copy [nq, ld] in w_q32, fp16 operand [nq_pad, ld] in w_q16, w_flag reset
// (the fp16 conversion raises it for a value it cannot represent)
void convert_scan_queries(rsx_index* h, const void* dq, int dtype, int64_t nq, int64_t nq_pad);
// the exact coarse stage in its two launches' halves (search puts a stage mark between them): fp32 scores of every centroid (w_coarse);
// then the nprobe best lists of every query, w_probelist / w_dis0 / w_segstart with lists padded to pad_to rows
void coarse_exact_scores(rsx_index* h, int64_t nq);
void coarse_exact_probes(rsx_index* h, int64_t nq, int nprobe, int pad_to);
// 16-query tiles per group of the LDS-DMA list scans (1, 2, 4 = 16, 32, 64 probing queries; 8 = the 128-query form, only where
// allow_128), from "ivf_qtiles" and the probing queries per list; the caller has checked that the LDS-DMA scan applies
int list_scan_qtiles(const rsx_index* h, int64_t npairs, bool allow_128);
// L2: the ranking bias -|x|^2 / 2 of every storage row, in w_misc
const float* l2_bias_rows(rsx_index* h);

// what a list-major scan reads of a grouping: the pairs sorted by list, the per-list offsets, the (list, tile, group) work items
struct PairView { const int32_t *pairs_sorted, *pair_off, *group_off, *total_groups, *item_off, *total_items; int nlist; };
// the (query, probe) pairs of a batch grouped by list (launch_group_pairs), carved out of h->w_pairs; probes: the queries' probed lists
// [nq, np] (null: w_probelist)
struct PairArea {
    rsx_index* h; int64_t npairs; int nlist, nprobe; const int32_t* probes;
    int32_t *pairs_sorted, *cnt, *cursor, *pair_off, *group_off, *item_off, *total_groups, *total_items;
    PairArea(rsx_index* hh, int64_t nq, int np, int nl, const int32_t* pl = nullptr) : h(hh), npairs(nq * np), nlist(nl), nprobe(np), probes(pl) {
        h->w_pairs.ensure((size_t)(npairs + 5 * (size_t)(nlist + 1) + 8) * 4);
        pairs_sorted = h->w_pairs.as<int32_t>(); cnt = pairs_sorted + npairs; cursor = cnt + (nlist + 1); pair_off = cursor + (nlist + 1);
        group_off = pair_off + (nlist + 1); item_off = group_off + (nlist + 1); total_groups = item_off + (nlist + 1); total_items = total_groups + 1;
    }
    // groups of G probing queries; tile_rows > 0: also the (list, tile, group) work items (at most tile_cap tiles per list, 0 = all)
    PairGroupArgs args(int G, int tile_rows, int tile_cap) const {
        PairGroupArgs g{};
        g.probe_list = probes ? probes : h->w_probelist.as<int32_t>(); g.pair_off = pair_off; g.group_off = group_off; g.total_groups = total_groups; g.pairs_sorted = pairs_sorted;
        if (tile_rows) { g.list_len = h->d_len.as<int64_t>(); g.item_off = item_off; g.total_items = total_items; }
        g.npairs = (int)npairs; g.nlist = nlist; g.G = G; g.tile_rows = tile_rows; g.tile_cap = tile_cap;
        return g;
    }
    // ... over the probe ranks [0, jmax), in launches of its own
    void group(int G, int tile_rows, int jmax, int tile_cap, hipStream_t st) const { launch_group_pairs(args(G, tile_rows, tile_cap), cnt, cursor, nprobe, jmax, st); }
    PairView view() const { return PairView{pairs_sorted, pair_off, group_off, total_groups, item_off, total_items, nlist}; }
};
// what the list scans of IVF-Flat and IVF-SQ share: lists, grouping, probes (w_probelist / w_segstart), score rows [nq, tmax] in w_temp, the
// group bound, the L2 bias; each adds its rows and queries
ListScanArgs list_scan_args(rsx_index* h, int64_t nq, int64_t tmax, const PairArea& pr);

// profile > 0: stream time between two points
struct StreamTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr; hipStream_t st;
    StreamTimer(bool on, hipStream_t s) : st(s) { if (on) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); } }
    void start() { if (e0) (void)hipEventRecord(e0, st); }
    void stop() { if (e1) (void)hipEventRecord(e1, st); }
    double ms() { float m = 0; if (e0 && e1) (void)hipEventElapsedTime(&m, e0, e1); return m; }      // after a synchronisation of the stream
    ~StreamTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
