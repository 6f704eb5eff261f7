// api_stages.hip — the batch stages shared by the search driver (api_search.hip) and the range driver (api_range.hip): rsx_stages.h.
// Host code only.
#include "rsx_stages.h"

std::pair<int64_t, int64_t> top_probe_sum(rsx_index* h, int nprobe, int unit, int scale) {
    const auto key = std::make_tuple(nprobe, unit, scale);
    auto it = h->bound_cache.find(key);
    if (it != h->bound_cache.end() && it->second.first == h->dir_gen) return it->second.second;
    std::vector<int64_t> t((size_t)h->nlist);
    for (int l = 0; l < h->nlist; l++) t[(size_t)l] = (h->h_len[(size_t)l] + unit - 1) / unit * scale;
    const int np = std::min(nprobe, h->nlist);
    std::partial_sort(t.begin(), t.begin() + np, t.end(), std::greater<int64_t>());
    int64_t s = 0;
    for (int j = 0; j < np; j++) s += t[(size_t)j];
    const std::pair<int64_t, int64_t> r(s, np > 0 ? t[0] : 0);
    h->bound_cache[key] = std::make_pair(h->dir_gen, r);
    return r;
}
// sum_l ceil(cnt_l/G)*tiles_l <= (nq * TQ)/G + sum_l tiles_l, TQ = tiles of the nprobe longest lists
int64_t max_scan_items(rsx_index* h, int64_t nq, int nprobe, int G, int tile_rows) {
    const auto key = std::make_tuple(-1, tile_rows, 0);       // all tiles of all lists
    int64_t all;
    auto it = h->bound_cache.find(key);
    if (it != h->bound_cache.end() && it->second.first == h->dir_gen) all = it->second.second.first;
    else {
        all = 0;
        for (int l = 0; l < h->nlist; l++) all += (h->h_len[(size_t)l] + tile_rows - 1) / tile_rows;
        h->bound_cache[key] = std::make_pair(h->dir_gen, std::make_pair(all, (int64_t)0));
    }
    const int64_t tq = top_probe_sum(h, nprobe, tile_rows, 1).first;
    return (nq * tq + G - 1) / G + all + 8;
}
float cent_cmax(rsx_index* h) {
    if (h->cent_cmax_gen == h->cent_gen) return h->cent_cmax;
    double mx = 0.0;
    for (int l = 0; l < h->nlist; l++) { double n2 = 0.0; for (int t = 0; t < h->d; t++) { const double v = h->h_centroids[(size_t)l * h->d + t]; n2 += v * v; } mx = std::max(mx, n2); }
    h->cent_cmax = (float)(std::sqrt(mx) * 1.000001); h->cent_cmax_gen = h->cent_gen;
    return h->cent_cmax;
}

// |approx - exact| of the fp16-MFMA scan for ANY stored vector (Cauchy-Schwarz on the per-element errors):
//   fp32 accumulation of d exact products       (d + 2) 2^-24 |q| |x|
//   fp32 rows rounded to fp16 inside the scan   2^-11 |q| |x|        (fp16 storage is lossless)
//   fp32 queries rounded to fp16                2^-11 |q| |x|        (only when the batch held such a value: device flag)
//   L2: the ranking score adds -|x|^2/2 (fp32)  (d + 4) 2^-24 |x|^2  (folded into the absolute term)
// The one statement of the bound: k_finalize's certificate (finalize_args) and the fixed threshold of a radius search (k_range_tau, which
// must admit every member) both take their terms from here.  tests/range_ref.py::scan_bound restates the fp32 expressions bit for bit.
ScanBound scan_cert_bound(const rsx_index* h) {
    const int d = h->d;
    const float u24 = 5.9604645e-8f, u11 = 4.8828125e-4f;
    const float xmax = sqrtf(h->max_norm2) * 1.0000002f;
    ScanBound b;
    b.xmax = xmax;
    b.rel = ((float)d + 2.0f) * u24 * 1.01f + (h->storage_f16 ? 0.0f : u11 * 1.002f);
    b.rel_qlossy = u11 * 1.002f + u11 * u11;
    b.abs = sqrtf((float)d) * u24 + (h->metric == RSX_METRIC_L2 ? ((float)d + 4.0f) * u24 * xmax : 0.0f);
    return b;
}
void convert_scan_queries(rsx_index* h, const void* dq, int dtype, int64_t nq, int64_t nq_pad) {
    const int d = h->d, ld = h->ld;
    h->w_q32.ensure((size_t)nq * ld * 4); h->w_q16.ensure((size_t)nq_pad * ld * 2); h->w_flag.ensure(sizeof(int));
    launch_convert_to_f32(dq, dtype == RSX_F16, d, nq, d, h->w_q32.as<float>(), ld, h->st);
    HIPCHECK(hipMemsetAsync(h->w_flag.p, 0, sizeof(int), h->st));
    launch_convert_to_f16(dq, dtype == RSX_F16, nq, d, h->w_q16.as<__half>(), ld, nq_pad, h->w_flag.as<int>(), h->st);
}
void select_rows(rsx_index* h, const float* scores, int64_t row_stride, const int64_t* row_n, int64_t row_n_stride, int64_t n_max,
                 uint32_t idx_base, int64_t nrows, int KP, int BUF, int k, uint64_t* state, bool merge_state,
                 unsigned long long* threshold_only_cnt) {
    int64_t seg_len = round_up(std::max<int64_t>(4096, (int64_t)8 * BUF), 256);
    if (KP >= 1024 && n_max <= 131072) seg_len = round_up(n_max, 256);     // one segment: the radix selection (launch_select)
    int nseg = (int)std::max<int64_t>(1, (n_max + seg_len - 1) / seg_len);
    SelectArgs a{};
    a.in = scores; a.in_is_keys = 0; a.row_stride = row_stride;
    a.row_n = row_n; a.row_n_stride = row_n_stride; a.n_uniform = n_max;
    a.seg_len = seg_len; a.nseg = nseg; a.idx_base = idx_base;
    a.nrows = nrows; a.KP = KP; a.BUF = BUF; a.k = k;
    if (nseg == 1) {
        a.init = merge_state ? state : nullptr;
        a.out = state; a.out_row_stride = KP;
        if (threshold_only_cnt) { a.keep_last = 1; a.zero_cnt = threshold_only_cnt; }
        launch_select(a, h->st);
        return;
    }
    h->w_keys1.ensure((size_t)nrows * nseg * KP * 8);
    a.init = nullptr; a.out = h->w_keys1.as<uint64_t>(); a.out_row_stride = (int64_t)nseg * KP;
    if (nseg >= 4 && !merge_state) {
        // Phase A: segment 0 of every row (for IVF: the head of the closest list) alone; its k-th key is a
        // lower bound of the row's final k-th best, so (phase B) the other segments start from that
        // threshold and append almost nothing — no LDS sorts on the bulk of the row.
        SelectArgs a0 = a; a0.nseg = 1; a0.seg_base = 0;
        launch_select(a0, h->st);
        a.seg_base = 1;
        a.tau_ptr = h->w_keys1.as<uint64_t>() + (k - 1); a.tau_stride = (int64_t)nseg * KP;
        launch_select(a, h->st);
    } else
        launch_select(a, h->st);
    SelectArgs b{};
    b.in = h->w_keys1.p; b.in_is_keys = 1; b.row_stride = (int64_t)nseg * KP;
    b.row_n = nullptr; b.n_uniform = (int64_t)nseg * KP;
    b.seg_len = round_up((int64_t)nseg * KP, 256); b.nseg = 1; b.idx_base = 0;
    b.init = merge_state ? state : nullptr;
    b.out = state; b.out_row_stride = KP;
    b.nrows = nrows; b.KP = KP; b.BUF = BUF; b.k = k;
    if (threshold_only_cnt) { b.keep_last = 1; b.zero_cnt = threshold_only_cnt; }
    launch_select(b, h->st);
}
void coarse_exact_scores(rsx_index* h, int64_t nq) {
    const int nlp = (int)round_up(h->nlist, 4);   // row stride of the coarse scores: 16-byte aligned rows for k_select
    h->w_coarse.ensure((size_t)nq * nlp * 4);
    launch_gemm_exact_scores(h->w_q32.p, 0, nq, h->ld, h->d_centroids.as<float>(), h->nlist, h->d, h->w_coarse.as<float>(), nlp, h->st);
}
void coarse_exact_probes(rsx_index* h, int64_t nq, int nprobe, int pad_to) {
    const int nlist = h->nlist, nlp = (int)round_up(nlist, 4);
    h->w_probelist.ensure((size_t)nq * nprobe * 4); h->w_dis0.ensure((size_t)nq * nprobe * 4); h->w_segstart.ensure((size_t)nq * (nprobe + 1) * 8);
    const int KPp = std::max(16, pow2ceil(nprobe)), BUFp = std::max(2 * KPp, 256);
    h->w_probekeys.ensure((size_t)nq * KPp * 8);
    select_rows(h, h->w_coarse.as<float>(), nlp, nullptr, 0, nlist, 0, nq, KPp, BUFp, nprobe, h->w_probekeys.as<uint64_t>(), false);
    // probe set-up
    launch_probe_setup(h->w_probekeys.as<uint64_t>(), KPp, nq, nprobe, h->d_len.as<int64_t>(), pad_to,
                       h->w_probelist.as<int32_t>(), h->w_dis0.as<float>(), h->w_segstart.as<int64_t>(), h->st);
}

// A group passes over its list's rows once, so the larger the group the fewer passes: 16 (k_list_scan2<_, 1>: two workgroups per CU), 64
// (the 8-wave form, queries in LDS) or 128 (k_list_scan3, queries in registers: d = 384 / 512 / 768 / 1024).  Measured at 20M x 768, batch
// 1024 (profiles/r05_ivfflat_wide.md): 16 wins at 8 probing queries per list, 64 from 16 on, 128 from 64 on; the 32-query form lost everywhere and
// is only reachable through the parameter: "ivf_qtiles" 0 forces 16, 2 or 3 ask for 32, 4 and more for 64, 8 for 128, each lowered to what the LDS holds.
int list_scan_qtiles(const rsx_index* h, int64_t npairs, bool allow_128) {
    if (h->ivf_qtiles == 0) return 1;
    const int64_t qpl = npairs / std::max(1, h->nlist);
    int ls_qt = h->ivf_qtiles > 1 ? h->ivf_qtiles : (qpl >= 48 && allow_128 ? 8 : qpl >= 12 ? 4 : 1);
    if (ls_qt == 8 && !allow_128) ls_qt = 4;
    if (ls_qt != 8) ls_qt = std::min(ls_qt == 3 ? 2 : ls_qt, list_scan2_max_qtiles(h->ld));
    if (ls_qt != 2 && ls_qt != 4 && ls_qt != 8) ls_qt = 1;
    return ls_qt;
}
ListScanArgs list_scan_args(rsx_index* h, int64_t nq, int64_t tmax, const PairArea& pr) {
    const int64_t npairs = pr.npairs;
    ListScanArgs a{};
    a.ld = h->ld;
    a.bias = h->metric == RSX_METRIC_L2 ? h->w_misc.as<float>() : nullptr;
    a.list_base = h->d_base.as<int64_t>(); a.list_len = h->d_len.as<int64_t>();
    a.pairs_sorted = pr.pairs_sorted; a.pair_off = pr.pair_off; a.group_off = pr.group_off; a.total_groups = pr.total_groups;
    a.probe_list = h->w_probelist.as<int32_t>(); a.seg_start = h->w_segstart.as<int64_t>();
    a.nlist = pr.nlist; a.nprobe = pr.nprobe; a.flat_mode = 0; a.nq = (int)nq;
    a.temp = h->w_temp.as<float>(); a.tstride = tmax;
    a.max_groups = (int)std::min<int64_t>(npairs, npairs / 16 + std::min<int64_t>(pr.nlist, npairs));
    return a;
}

const float* l2_bias_rows(rsx_index* h) {
    h->w_misc.ensure((size_t)h->total_cap * 4);
    launch_bias_from_norms(h->norms.as<float>(), h->w_misc.as<float>(), h->total_cap, h->st);
    return h->w_misc.as<float>();
}
