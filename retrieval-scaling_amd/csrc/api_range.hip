// api_range.hip — rsx_range_search's host driver (faiss Index::range_search on Flat and IVF-Flat handles).  Per internal
// batch: the queries' fp16 / fp32 copies, the per-query threshold (k_range_tau), the EXISTING filtered scans with that fixed threshold
// (launch_flat_gemm_filter / the 16- and 64-query forms of k_list_scan2 behind launch_list_scan), one read-back of the candidate counters,
// a second scan with rows sized from the counts for the queries whose row overflowed, then k_range.hip's back end: exact re-score,
// membership, counts, lims, ordering, emission.  Every result is exact; what cannot be served ends the call with an error code.
// The coarse stage, the selection call and the pair grouping restate, for this driver's needs, helpers that are static in api_search.hip.
#include "rsx_range.h"

namespace {

// |approx - exact| of the fp16-MFMA scans for any stored vector: the terms of api_search.hip's finalize_args (derived there), which
// k_finalize's certificate and k_range_tau combine as  rel |q| xmax + abs (|q| + xmax)
struct ScanBound { float rel, rel_qlossy, xmax, abs; };
ScanBound scan_bound(const rsx_index* h) {
    const float u24 = 5.9604645e-8f, u11 = 4.8828125e-4f, d = (float)h->d;
    ScanBound b;
    b.xmax = sqrtf(h->max_norm2) * 1.0000002f;
    b.rel = (d + 2.0f) * u24 * 1.01f + (h->storage_f16 ? 0.0f : u11 * 1.002f);
    b.rel_qlossy = u11 * 1.002f + u11 * u11;
    b.abs = sqrtf(d) * u24 + (h->metric == RSX_METRIC_L2 ? (d + 4.0f) * u24 * b.xmax : 0.0f);
    return b;
}

// top k of every row of fp32 scores [nrows, n] (row stride given) into state [nrows, KP]: api_search.hip's select_rows without a running state
void select_top(rsx_index* h, const float* scores, int64_t row_stride, int64_t n, int64_t nrows, int KP, int BUF, int k, uint64_t* state) {
    int64_t seg_len = round_up(std::max<int64_t>(4096, (int64_t)8 * BUF), 256);
    if (KP >= 1024 && n <= 131072) seg_len = round_up(n, 256);
    const int nseg = (int)std::max<int64_t>(1, (n + seg_len - 1) / seg_len);
    SelectArgs a{};
    a.in = scores; a.in_is_keys = 0; a.row_stride = row_stride; a.n_uniform = n; a.seg_len = seg_len; a.nseg = nseg;
    a.nrows = nrows; a.KP = KP; a.BUF = BUF; a.k = k;
    if (nseg == 1) { a.out = state; a.out_row_stride = KP; launch_select(a, h->st); return; }
    h->w_keys1.ensure((size_t)nrows * nseg * KP * 8);
    a.out = h->w_keys1.as<uint64_t>(); a.out_row_stride = (int64_t)nseg * KP;
    launch_select(a, h->st);
    SelectArgs b{};
    b.in = h->w_keys1.p; b.in_is_keys = 1; b.row_stride = (int64_t)nseg * KP; b.n_uniform = (int64_t)nseg * KP;
    b.seg_len = round_up((int64_t)nseg * KP, 256); b.nseg = 1;
    b.out = state; b.out_row_stride = KP; b.nrows = nrows; b.KP = KP; b.BUF = BUF; b.k = k;
    launch_select(b, h->st);
}

// what the IVF scans need of the list directory
struct IvfGeometry { int nprobe; int64_t tmax, maxlen; };
IvfGeometry ivf_geometry(const rsx_index* h) {
    IvfGeometry g{};
    g.nprobe = std::min(h->nprobe, h->nlist);
    std::vector<int64_t> t((size_t)h->nlist);
    for (int l = 0; l < h->nlist; l++) t[(size_t)l] = round_up(h->h_len[(size_t)l], 16);
    std::partial_sort(t.begin(), t.begin() + g.nprobe, t.end(), std::greater<int64_t>());
    for (int j = 0; j < g.nprobe; j++) g.tmax += t[(size_t)j];
    g.maxlen = g.nprobe > 0 ? t[0] : 0;
    g.tmax = std::max<int64_t>(round_up(g.tmax, 256), 256);
    return g;
}
// upper bound of the (list, tile, group) work items of a list-major scan (api_search.hip: max_scan_items)
int64_t scan_items_bound(const rsx_index* h, int64_t nq, int nprobe, int G, int tile_rows) {
    std::vector<int64_t> t((size_t)h->nlist);
    int64_t all = 0;
    for (int l = 0; l < h->nlist; l++) { t[(size_t)l] = (h->h_len[(size_t)l] + tile_rows - 1) / tile_rows; all += t[(size_t)l]; }
    std::partial_sort(t.begin(), t.begin() + nprobe, t.end(), std::greater<int64_t>());
    int64_t tq = 0;
    for (int j = 0; j < nprobe; j++) tq += t[(size_t)j];
    return (nq * tq + G - 1) / G + all + 8;
}

// one scan's inputs: nq queries (fp16 rows padded to nq_pad), their thresholds, (IVF) their probes; its candidate rows
struct ScanSet {
    const __half* Q16; int64_t nq, nq_pad; const uint64_t* tau;
    const int32_t* probe_list; const int64_t* seg_start;
    uint64_t* cand; unsigned long long* cnt; int cap;
};

void scan_flat(rsx_index* h, const ScanSet& s, const float* bias) {
    launch_flat_gemm_filter(s.Q16, (int)s.nq_pad, (int)s.nq, h->data.p, h->storage_f16, 0, h->ntotal, h->ld, bias, s.tau, 1, s.cand, s.cnt, s.cap, h->st);
}

// pair grouping + the filtered list scan.  Groups of 16 or 64 probing queries (k_list_scan2), chosen from the probing queries per list;
// "ivf_qtiles" 0 forces 16, 2 or 3 ask for 32, 4 and more for 64, each lowered to what list_scan2_max_qtiles(ld) lets the LDS hold.  The
// 128-query form (k_list_scan3) is not taken by this driver.
void scan_ivf(rsx_index* h, const ScanSet& s, const IvfGeometry& g, const float* bias) {
    const int nlist = h->nlist, nprobe = g.nprobe, ld = h->ld;
    const int64_t npairs = s.nq * nprobe;
    const int ls2_rows = list_scan2_chunk_rows(h->storage_f16, ld);
    int ls_qt = h->ivf_qtiles == 0 ? 1 : h->ivf_qtiles > 1 ? std::min(h->ivf_qtiles, 4) : (npairs / std::max(1, nlist) >= 12 ? 4 : 1);
    ls_qt = std::min(ls_qt == 3 ? 2 : ls_qt, list_scan2_max_qtiles(ld));
    if (ls_qt != 2 && ls_qt != 4) ls_qt = 1;
    const int chunk_rows = ls_qt >= 4 ? 2 * ls2_rows : ls2_rows;
    // the pairs grouped by list, carved out of w_pairs as api_search.hip's PairArea does
    h->w_pairs.ensure((size_t)(npairs + 5 * (size_t)(nlist + 1) + 8) * 4);
    int32_t* pairs_sorted = h->w_pairs.as<int32_t>();
    int32_t *cnt = pairs_sorted + npairs, *cursor = cnt + (nlist + 1), *pair_off = cursor + (nlist + 1), *group_off = pair_off + (nlist + 1),
            *item_off = group_off + (nlist + 1), *total_groups = item_off + (nlist + 1), *total_items = total_groups + 1;
    PairGroupArgs pg{};
    pg.probe_list = s.probe_list; pg.list_len = h->d_len.as<int64_t>();
    pg.pair_off = pair_off; pg.group_off = group_off; pg.item_off = item_off; pg.total_groups = total_groups; pg.total_items = total_items;
    pg.pairs_sorted = pairs_sorted; pg.npairs = (int)npairs; pg.nlist = nlist; pg.G = 16 * ls_qt; pg.tile_rows = chunk_rows;
    launch_group_pairs(pg, cnt, cursor, nprobe, nprobe, h->st);
    ListScanArgs a{};
    a.Q16 = s.Q16; a.ld = ld; a.X = h->data.p; a.x_f16 = h->storage_f16; a.bias = bias;
    a.list_base = h->d_base.as<int64_t>(); a.list_len = h->d_len.as<int64_t>();
    a.pairs_sorted = pairs_sorted; a.pair_off = pair_off; a.group_off = group_off; a.total_groups = total_groups;
    a.probe_list = s.probe_list; a.seg_start = s.seg_start; a.nlist = nlist; a.nprobe = nprobe; a.nq = (int)s.nq;
    a.tstride = g.tmax;
    a.chunk_rows = chunk_rows; a.qtiles = ls_qt;
    a.max_groups = (int)std::min<int64_t>(npairs, npairs / 16 + std::min<int64_t>(nlist, npairs));
    a.max_chunks = (int)std::max<int64_t>(1, (g.maxlen + chunk_rows - 1) / chunk_rows);
    a.item_off = item_off; a.total_items = total_items; a.max_items = (int)scan_items_bound(h, s.nq, nprobe, 16 * ls_qt, chunk_rows);
    a.tau_key = s.tau; a.tau_stride = 1; a.cand = s.cand; a.cand_cnt = s.cnt; a.cand_cap = s.cap;
    launch_list_scan(a, h->st);
}

int64_t pow2ceil64(int64_t x) { int64_t p = 1; while (p < x) p <<= 1; return p; }
// keys of a second-pass row for a query the first pass counted m candidates for: a power of two with room for a count that differs in the last bits
int64_t group_row(int64_t m) { return pow2ceil64(m + m / 64 + 16); }

struct Timer {       // profile > 0: stream time between two points
    hipEvent_t e0 = nullptr, e1 = nullptr; hipStream_t st;
    Timer(bool on, hipStream_t s) : st(s) { if (on) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); } }
    void start() { if (e0) (void)hipEventRecord(e0, st); }
    void stop() { if (e1) (void)hipEventRecord(e1, st); }
    double ms() { float m = 0; if (e0 && e1) (void)hipEventElapsedTime(&m, e0, e1); return m; }      // after a synchronisation of the stream
    ~Timer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

}  // namespace

rsx_range_result* range_impl(rsx_index* h, int64_t nq, const void* q, int dtype, float radius) {
    if (nq < 0) RSX_THROW(RSX_ERR_INVALID, "range_search: nq = %lld", (long long)nq);
    if (!std::isfinite(radius)) RSX_THROW(RSX_ERR_INVALID, "range_search: the radius must be finite");
    if (!h->trained) RSX_THROW(RSX_ERR_NOT_TRAINED, "range_search before train");
    if (nq > 0 && !q) RSX_THROW(RSX_ERR_INVALID, "range_search: null pointer");
    const bool ivf = h->kind == KIND_IVFFLAT, q_dev = is_device_ptr(q), l2 = h->metric == RSX_METRIC_L2;
    const int d = h->d, ld = h->ld;
    const size_t esz = dtype == RSX_F16 ? 2 : 4;
    if (ivf && h->ntotal > 0 && list_scan2_chunk_rows(h->storage_f16, ld) == 0)
        RSX_THROW(RSX_ERR_UNSUPPORTED, "range_search: an IndexIVFFlat whose rows are stored as fp32 has no filtered list scan in this build");
    std::unique_ptr<rsx_range_result> R(new rsx_range_result());
    R->nq = nq; R->on_device = q_dev ? 1 : 0; R->device = h->device;
    std::vector<int64_t> lims((size_t)nq + 1, 0);
    std::vector<std::pair<std::unique_ptr<DevBuf>, std::unique_ptr<DevBuf>>> chunks;      // device results: a batch's D and I
    std::vector<int64_t> chunk_n;

    IvfGeometry geo{};
    if (ivf && h->ntotal > 0 && nq > 0) {
        geo = ivf_geometry(h);
        if (geo.nprobe > 4096) RSX_THROW(RSX_ERR_UNSUPPORTED, "range_search: %d probed lists per query exceed this build's maximum of 4096", geo.nprobe);
        if (geo.tmax >= ((int64_t)1 << 32)) RSX_THROW(RSX_ERR_UNSUPPORTED, "range_search: probed lists exceed 2^32 vectors per query");
    }
    Timer t_all(h->profile > 0, h->st), t_back(h->profile > 0, h->st);
    double back_ms = 0.0, n_cand = 0.0, n_over = 0.0;
    if (h->ntotal > 0 && nq > 0) {
        t_all.start();
        const float* bias = nullptr;
        if (l2) {
            h->w_misc.ensure((size_t)h->total_cap * 4);
            launch_range_bias(h->norms.as<float>(), h->w_misc.as<float>(), h->total_cap, h->st);
            bias = h->w_misc.as<float>();
        }
        const ScanBound sb = scan_bound(h);
        const int nprobe = geo.nprobe;
        // first-pass capacity: "range_cand_cap" (default 65536 keys), a power of two (the sort's network), never more than a query can see
        const int64_t visible = ivf ? geo.tmax : h->ntotal;
        const int cap1 = (int)std::min<int64_t>((int64_t)1 << 30, pow2ceil64(std::max<int64_t>(64, std::min<int64_t>(h->range_cand_cap > 0 ? h->range_cand_cap : 65536, visible))));
        const int64_t qb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(std::max(1, h->query_batch), 32768), h->temp_budget / ((int64_t)cap1 * 8)));
        const int64_t* ids = (h->kind == KIND_FLAT && !h->custom_ids) ? nullptr : h->ids.as<int64_t>();
        std::vector<unsigned long long> cnts;
        std::vector<int32_t> rcnt, nmem_h;
        std::vector<uint64_t*> kptr;
        std::vector<int64_t> lims_b;
        for (int64_t q0 = 0; q0 < nq; q0 += qb) {
            const int64_t nb = std::min(qb, nq - q0), nq_pad = nb > 128 ? round_up(nb, 256) : 128;
            const void* dq = (const char*)q + (size_t)q0 * d * esz;
            if (!q_dev) {
                h->w_qin.ensure((size_t)nb * d * esz);
                HIPCHECK(hipMemcpyAsync(h->w_qin.p, dq, (size_t)nb * d * esz, hipMemcpyHostToDevice, h->st));
                dq = h->w_qin.p;
            }
            // 1. the queries as `search` converts them: fp32 copy, fp16 operand, the "lossy query" flag
            h->w_q32.ensure((size_t)nb * ld * 4); h->w_q16.ensure((size_t)nq_pad * ld * 2); h->w_flag.ensure(sizeof(int));
            launch_convert_to_f32(dq, dtype == RSX_F16, d, nb, d, h->w_q32.as<float>(), ld, h->st);
            HIPCHECK(hipMemsetAsync(h->w_flag.p, 0, sizeof(int), h->st));
            launch_convert_to_f16(dq, dtype == RSX_F16, nb, d, h->w_q16.as<__half>(), ld, nq_pad, h->w_flag.as<int>(), h->st);
            if (ivf) {
                // the coarse stage by the exact route: the oracle's probe order (api_search.hip: coarse_quantiser)
                const int nlp = (int)round_up(h->nlist, 4);
                h->w_probelist.ensure((size_t)nb * nprobe * 4); h->w_dis0.ensure((size_t)nb * nprobe * 4); h->w_segstart.ensure((size_t)nb * (nprobe + 1) * 8);
                h->w_coarse.ensure((size_t)nb * nlp * 4);
                launch_gemm_exact_scores(h->w_q32.p, 0, nb, ld, h->d_centroids.as<float>(), h->nlist, d, h->w_coarse.as<float>(), nlp, h->st);
                const int KPp = std::max(16, pow2ceil(nprobe)), BUFp = std::max(2 * KPp, 256);
                h->w_probekeys.ensure((size_t)nb * KPp * 8);
                select_top(h, h->w_coarse.as<float>(), nlp, h->nlist, nb, KPp, BUFp, nprobe, h->w_probekeys.as<uint64_t>());
                launch_probe_setup(h->w_probekeys.as<uint64_t>(), KPp, nb, nprobe, h->d_len.as<int64_t>(), 16, h->w_probelist.as<int32_t>(),
                                   h->w_dis0.as<float>(), h->w_segstart.as<int64_t>(), h->st);
            }
            // 2. thresholds (and the counters' reset)
            h->w_tau.ensure((size_t)nb * 8); h->w_candcnt.ensure((size_t)nb * 8 * CCS);
            RangeTauArgs ta{};
            ta.Q32 = h->w_q32.as<float>(); ta.ldq = ld; ta.d = d; ta.nq = nb; ta.metric = h->metric; ta.radius = radius;
            ta.cert_rel = sb.rel; ta.cert_rel_qlossy = sb.rel_qlossy; ta.cert_xmax = sb.xmax; ta.cert_abs = sb.abs; ta.cert_qflag = h->w_flag.as<int>();
            ta.tau = h->w_tau.as<uint64_t>(); ta.cand_cnt = h->w_candcnt.as<unsigned long long>();
            launch_range_tau(ta, h->st);
            // 3. the scan with the fixed thresholds
            h->w_cand.ensure((size_t)nb * cap1 * 8);
            ScanSet s1{h->w_q16.as<__half>(), nb, nq_pad, h->w_tau.as<uint64_t>(), h->w_probelist.as<int32_t>(), h->w_segstart.as<int64_t>(),
                       h->w_cand.as<uint64_t>(), h->w_candcnt.as<unsigned long long>(), cap1};
            if (ivf) scan_ivf(h, s1, geo, bias); else scan_flat(h, s1, bias);
            // 4. the counters count past the capacity: one read-back tells every query's candidate count
            cnts.resize((size_t)nb * CCS);
            HIPCHECK(hipMemcpyAsync(cnts.data(), h->w_candcnt.p, (size_t)nb * 8 * CCS, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipStreamSynchronize(h->st));
            t_back.start();
            rcnt.assign((size_t)nb, 0); kptr.assign((size_t)nb, nullptr);
            std::vector<int64_t> over;
            int max1 = 0;
            for (int64_t i = 0; i < nb; i++) {
                const unsigned long long c = cnts[(size_t)i * CCS];
                n_cand += (double)c;
                if (c > (unsigned long long)cap1) { over.push_back(i); continue; }
                rcnt[(size_t)i] = (int32_t)c; max1 = std::max(max1, (int)c);
                kptr[(size_t)i] = h->w_cand.as<uint64_t>() + (size_t)i * cap1;
            }
            n_over += (double)over.size();
            h->w_rg_cnt.ensure((size_t)nb * 4); h->w_rg_nmem.ensure((size_t)nb * 4); h->w_rg_lims.ensure((size_t)(nb + 1) * 8); h->w_rg_kptr.ensure((size_t)nb * 8);
            HIPCHECK(hipMemcpyAsync(h->w_rg_cnt.p, rcnt.data(), (size_t)nb * 4, hipMemcpyHostToDevice, h->st));
            HIPCHECK(hipMemsetAsync(h->w_rg_nmem.p, 0, (size_t)nb * 4, h->st));
            // 5. back end on the rows that held: exact re-score + membership, ordering
            RangeRowsArgs ra{};
            ra.cand = h->w_cand.as<uint64_t>(); ra.cap = cap1; ra.nrows = nb; ra.rcnt = h->w_rg_cnt.as<int32_t>(); ra.qsel = nullptr;
            ra.kind = h->kind; ra.metric = h->metric; ra.radius = radius;
            ra.Q32 = h->w_q32.as<float>(); ra.ldq = ld; ra.d = d; ra.X = h->data.p; ra.x_f16 = h->storage_f16; ra.ld = ld;
            ra.probe_list = h->w_probelist.as<int32_t>(); ra.seg_start = h->w_segstart.as<int64_t>(); ra.nprobe = nprobe; ra.list_base = h->d_base.as<int64_t>();
            ra.ids = ids; ra.nmem = h->w_rg_nmem.as<int32_t>(); ra.max_cnt = max1;
            launch_range_rescore(ra, h->st);
            launch_range_sort(ra, h->st);
            // ... and the overflowed queries again, rows sized from their counts, in groups the temp budget holds; a group's members are kept
            // (sorted keys) until the batch's lims are known
            std::vector<std::unique_ptr<DevBuf>> kept;
            for (size_t i0 = 0; i0 < over.size();) {
                int64_t maxc = 0; size_t i1 = i0;
                while (i1 < over.size()) {
                    const int64_t m = std::max<int64_t>(maxc, (int64_t)cnts[(size_t)over[i1] * CCS]);
                    if (m > ((int64_t)1 << 29) || (int64_t)(i1 - i0 + 1) * group_row(m) * 8 > h->temp_budget) break;
                    maxc = m; i1++;
                }
                if (i1 == i0) RSX_THROW(RSX_ERR_OOM, "range_search: a query has %llu candidates; their row does not fit the temp budget (temp_budget_mb)",
                                        cnts[(size_t)over[i0] * CCS]);
                const int64_t gn = (int64_t)(i1 - i0), gn_pad = gn > 128 ? round_up(gn, 256) : 128;
                const int capg = (int)group_row(maxc);
                DevBuf g_cand, g_cnt, g_q16, g_tau, g_sel, g_rcnt, g_pl, g_ss, g_koff;
                g_cand.ensure((size_t)gn * capg * 8); g_cnt.ensure((size_t)gn * 8 * CCS); g_q16.ensure((size_t)gn_pad * ld * 2); g_tau.ensure((size_t)gn * 8);
                g_sel.ensure((size_t)gn * 4); g_rcnt.ensure((size_t)gn * 4); g_koff.ensure((size_t)gn * 8);
                std::vector<int32_t> sel((size_t)gn), grc((size_t)gn);
                for (int64_t r = 0; r < gn; r++) sel[(size_t)r] = (int32_t)over[i0 + (size_t)r];
                HIPCHECK(hipMemcpyAsync(g_sel.p, sel.data(), (size_t)gn * 4, hipMemcpyHostToDevice, h->st));
                HIPCHECK(hipMemsetAsync(g_q16.p, 0, (size_t)gn_pad * ld * 2, h->st));
                HIPCHECK(hipMemsetAsync(g_cnt.p, 0, (size_t)gn * 8 * CCS, h->st));
                launch_range_gather_rows(h->w_q16.p, g_q16.p, (int64_t)ld * 2, g_sel.as<int32_t>(), gn, h->st);
                launch_range_gather_rows(h->w_tau.p, g_tau.p, 8, g_sel.as<int32_t>(), gn, h->st);
                if (ivf) {
                    g_pl.ensure((size_t)gn * nprobe * 4); g_ss.ensure((size_t)gn * (nprobe + 1) * 8);
                    launch_range_gather_rows(h->w_probelist.p, g_pl.p, (int64_t)nprobe * 4, g_sel.as<int32_t>(), gn, h->st);
                    launch_range_gather_rows(h->w_segstart.p, g_ss.p, (int64_t)(nprobe + 1) * 8, g_sel.as<int32_t>(), gn, h->st);
                }
                ScanSet sg{g_q16.as<__half>(), gn, gn_pad, g_tau.as<uint64_t>(), g_pl.as<int32_t>(), g_ss.as<int64_t>(), g_cand.as<uint64_t>(),
                           g_cnt.as<unsigned long long>(), capg};
                if (ivf) scan_ivf(h, sg, geo, bias); else scan_flat(h, sg, bias);
                std::vector<unsigned long long> gc((size_t)gn * CCS);
                HIPCHECK(hipMemcpyAsync(gc.data(), g_cnt.p, (size_t)gn * 8 * CCS, hipMemcpyDeviceToHost, h->st));
                HIPCHECK(hipStreamSynchronize(h->st));
                int maxg = 0;
                // The group may run another form of the scan than the first pass did (query padding, probing queries per list), and nothing pins
                // the two forms' scores to the same bits: any count the row holds is a valid candidate set (both scans obey the same bound).
                // A count past the row cannot be served from it.
                for (int64_t r = 0; r < gn; r++) {
                    if (gc[(size_t)r * CCS] > (unsigned long long)capg)
                        RSX_THROW(RSX_ERR_OOM, "range_search: the second scan of a query found %llu candidates for a row of %d (the first scan counted %llu)",
                                  gc[(size_t)r * CCS], capg, cnts[(size_t)sel[(size_t)r] * CCS]);
                    grc[(size_t)r] = (int32_t)gc[(size_t)r * CCS]; maxg = std::max(maxg, grc[(size_t)r]);
                }
                HIPCHECK(hipMemcpyAsync(g_rcnt.p, grc.data(), (size_t)gn * 4, hipMemcpyHostToDevice, h->st));
                RangeRowsArgs rg = ra;
                rg.cand = g_cand.as<uint64_t>(); rg.cap = capg; rg.nrows = gn; rg.rcnt = g_rcnt.as<int32_t>(); rg.qsel = g_sel.as<int32_t>(); rg.max_cnt = maxg;
                launch_range_rescore(rg, h->st);
                launch_range_sort(rg, h->st);
                nmem_h.resize((size_t)nb);
                HIPCHECK(hipMemcpyAsync(nmem_h.data(), h->w_rg_nmem.p, (size_t)nb * 4, hipMemcpyDeviceToHost, h->st));
                HIPCHECK(hipStreamSynchronize(h->st));
                std::vector<int64_t> koff((size_t)gn);
                int64_t tot = 0; int maxm = 0;
                for (int64_t r = 0; r < gn; r++) { koff[(size_t)r] = tot; tot += nmem_h[(size_t)sel[(size_t)r]]; maxm = std::max(maxm, (int)nmem_h[(size_t)sel[(size_t)r]]); }
                kept.emplace_back(new DevBuf());
                kept.back()->ensure((size_t)std::max<int64_t>(tot, 1) * 8);
                HIPCHECK(hipMemcpyAsync(g_koff.p, koff.data(), (size_t)gn * 8, hipMemcpyHostToDevice, h->st));
                rg.max_cnt = maxm;
                launch_range_compact(rg, g_koff.as<int64_t>(), kept.back()->as<uint64_t>(), h->st);
                for (int64_t r = 0; r < gn; r++) kptr[(size_t)sel[(size_t)r]] = kept.back()->as<uint64_t>() + koff[(size_t)r];
                HIPCHECK(hipStreamSynchronize(h->st));      // the group's buffers go away here
                i0 = i1;
            }
            // counts -> lims; the batch's lims run on from the previous batch's last
            launch_range_lims(h->w_rg_nmem.as<int32_t>(), nb, lims[(size_t)q0], h->w_rg_lims.as<int64_t>(), h->st);
            lims_b.resize((size_t)nb + 1);
            HIPCHECK(hipMemcpyAsync(lims_b.data(), h->w_rg_lims.p, (size_t)(nb + 1) * 8, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipMemcpyAsync(h->w_rg_kptr.p, kptr.data(), (size_t)nb * 8, hipMemcpyHostToDevice, h->st));
            HIPCHECK(hipStreamSynchronize(h->st));
            int maxn = 0;
            for (int64_t i = 0; i < nb; i++) {
                lims[(size_t)(q0 + i + 1)] = lims_b[(size_t)i + 1];
                maxn = (int)std::max<int64_t>(maxn, lims_b[(size_t)i + 1] - lims_b[(size_t)i]);
            }
            const int64_t tot_b = lims_b[(size_t)nb] - lims_b[0];
            if (tot_b > 0) {
                std::unique_ptr<DevBuf> bD(new DevBuf()), bI(new DevBuf());
                bD->ensure((size_t)tot_b * 4); bI->ensure((size_t)tot_b * 8);
                RangeEmitArgs ea{};
                ea.kptr = h->w_rg_kptr.as<uint64_t*>(); ea.nmem = h->w_rg_nmem.as<int32_t>(); ea.lims = h->w_rg_lims.as<int64_t>(); ea.nq = nb;
                ea.kind = h->kind; ea.metric = h->metric; ea.probe_list = ra.probe_list; ea.seg_start = ra.seg_start; ea.nprobe = nprobe;
                ea.list_base = ra.list_base; ea.ids = ids; ea.D = bD->as<float>(); ea.I = bI->as<int64_t>(); ea.max_cnt = maxn;
                launch_range_emit(ea, h->st);
                launch_range_ties(ea, h->st);
                t_back.stop();
                if (!q_dev) {
                    R->h_D.resize((size_t)lims_b[(size_t)nb]); R->h_I.resize((size_t)lims_b[(size_t)nb]);
                    HIPCHECK(hipMemcpyAsync(R->h_D.data() + lims_b[0], bD->p, (size_t)tot_b * 4, hipMemcpyDeviceToHost, h->st));
                    HIPCHECK(hipMemcpyAsync(R->h_I.data() + lims_b[0], bI->p, (size_t)tot_b * 8, hipMemcpyDeviceToHost, h->st));
                }
                HIPCHECK(hipStreamSynchronize(h->st));
                if (q_dev) { chunks.emplace_back(std::move(bD), std::move(bI)); chunk_n.push_back(tot_b); }
            } else {
                t_back.stop();
                HIPCHECK(hipStreamSynchronize(h->st));
            }
            back_ms += t_back.ms();
        }
        t_all.stop();
        HIPCHECK(hipStreamSynchronize(h->st));
        HIPCHECK(hipGetLastError());
        if (h->profile > 0) { h->timing["range_ms"] += t_all.ms(); h->timing["range_backend_ms"] += back_ms; }
    }
    R->total = lims[(size_t)nq];
    h->timing["range_calls"] += 1.0;
    h->timing["range_candidates"] += n_cand;
    h->timing["range_results"] += (double)R->total;
    h->timing["range_overflow_queries"] += n_over;
    if (!q_dev) { R->h_lims.swap(lims); return R.release(); }
    R->d_lims.reset(new DevBuf());
    R->d_lims->ensure((size_t)(nq + 1) * 8);
    HIPCHECK(hipMemcpy(R->d_lims->p, lims.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice));
    if (chunks.size() == 1) { R->d_D = std::move(chunks[0].first); R->d_I = std::move(chunks[0].second); }
    else if (!chunks.empty()) {
        R->d_D.reset(new DevBuf()); R->d_I.reset(new DevBuf());
        R->d_D->ensure((size_t)R->total * 4); R->d_I->ensure((size_t)R->total * 8);
        int64_t off = 0;
        for (size_t c = 0; c < chunks.size(); c++) {
            HIPCHECK(hipMemcpyAsync(R->d_D->as<float>() + off, chunks[c].first->p, (size_t)chunk_n[c] * 4, hipMemcpyDeviceToDevice, h->st));
            HIPCHECK(hipMemcpyAsync(R->d_I->as<int64_t>() + off, chunks[c].second->p, (size_t)chunk_n[c] * 8, hipMemcpyDeviceToDevice, h->st));
            off += chunk_n[c];
        }
        HIPCHECK(hipStreamSynchronize(h->st));
    }
    return R.release();
}
