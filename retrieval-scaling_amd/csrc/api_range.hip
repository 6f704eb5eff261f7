// api_range.hip — rsx_range_search's host driver (faiss Index::range_search on Flat and IVF-Flat handles).  Per internal
// batch: the queries' fp16 / fp32 copies, (IVF) the probes, the per-query threshold (k_range_tau), the EXISTING filtered scans with that
// fixed threshold (launch_flat_gemm_filter / the 16- and 64-query forms of k_list_scan2 behind launch_list_scan), one read-back of the
// candidate counters, k_range.hip's back end on the rows that held (exact re-score, membership, ordering), the same scan and ranking
// with rows sized from the counts for the queries whose row overflowed, then lims and emission.  Every result is exact; what cannot be
// served ends the call with an error code.  Query conversion, coarse stage, selection, pair grouping, scan arguments and the scans' error
// bound are the search driver's own stages (rsx_stages.h); range_impl at the end of the file is the list of this driver's.
#include "rsx_range.h"

namespace {

// one scan's inputs: nq queries (fp16 rows padded to nq_pad), their thresholds, (IVF) their probes; its candidate rows: row r belongs to
// query qsel[r] of the batch (null: r) and holds rcnt[r] keys once the pass has read the counters
struct ScanSet {
    const __half* Q16; int64_t nq, nq_pad; const uint64_t* tau;
    const int32_t* probe_list; const int64_t* seg_start;
    uint64_t* cand; unsigned long long* cnt; int cap;
    const int32_t* qsel; int32_t* rcnt;
};
// what one call fixes for all of its batches, and what they add up
struct RangeCall {
    rsx_index* h; const void* q; int dtype; float radius; bool ivf, q_dev;
    int nprobe = 0; int64_t tmax = 0, maxlen = 0;        // IVF: the probed lists per query, a query's padded rows, the longest padded list
    const float* bias = nullptr; const int64_t* ids = nullptr; ScanBound sb{};
    int cap1 = 0; int64_t qb = 1;                         // keys of a first-pass row; queries per batch
    StreamTimer t_all, t_back;
    double back_ms = 0.0, n_cand = 0.0, n_over = 0.0;
    rsx_range_result* R = nullptr;
    std::vector<int64_t> lims;
    std::vector<std::pair<std::unique_ptr<DevBuf>, std::unique_ptr<DevBuf>>> chunks;      // device results: a batch's D and I
    std::vector<int64_t> chunk_n;
    RangeCall(rsx_index* hh, const void* qq, int dt, float r)
        : h(hh), q(qq), dtype(dt), radius(r), ivf(hh->kind == KIND_IVFFLAT), q_dev(is_device_ptr(qq)), t_all(hh->profile > 0, hh->st), t_back(hh->profile > 0, hh->st) {}
};
// one internal batch: queries [q0, q0 + nb)
struct RangeBatch {
    int64_t q0, nb, nq_pad;
    std::vector<unsigned long long> cnts;              // what the first scan counted per query
    std::vector<int32_t> rcnt;                         // ... and the keys its row holds (0: overflowed)
    std::vector<int64_t> over;                         // the queries whose row overflowed
    std::vector<uint64_t*> kptr;                       // every query's sorted members
    std::vector<std::unique_ptr<DevBuf>> kept;         // ... of the overflow groups, until the batch's lims are known
};

// pair grouping + the filtered list scan, in groups of 16, 32 or 64 probing queries (list_scan_qtiles: the 128-query form k_list_scan3 is
// not taken by this driver, and "scan_chunk" does not apply to it)
void scan_ivf(const RangeCall& C, const ScanSet& s) {
    rsx_index* h = C.h;
    const int nprobe = C.nprobe, ls_qt = list_scan_qtiles(h, s.nq * nprobe, false);
    const int chunk_rows = (ls_qt >= 4 ? 2 : 1) * list_scan2_chunk_rows(h->storage_f16, h->ld);
    const PairArea pr(h, s.nq, nprobe, h->nlist, s.probe_list);
    pr.group(16 * ls_qt, chunk_rows, nprobe, 0, h->st);
    ListScanArgs a = list_scan_args(h, s.nq, C.tmax, pr);
    a.Q16 = s.Q16; a.X = h->data.p; a.x_f16 = h->storage_f16;
    a.probe_list = s.probe_list; a.seg_start = s.seg_start; a.temp = nullptr;      // the set's own probes; no score rows
    a.chunk_rows = chunk_rows; a.qtiles = ls_qt;
    a.max_chunks = (int)std::max<int64_t>(1, (C.maxlen + chunk_rows - 1) / chunk_rows);
    a.item_off = pr.item_off; a.total_items = pr.total_items; a.max_items = (int)max_scan_items(h, s.nq, nprobe, 16 * ls_qt, chunk_rows);
    a.tau_key = s.tau; a.tau_stride = 1; a.cand = s.cand; a.cand_cnt = s.cnt; a.cand_cap = s.cap;      // the fixed thresholds
    launch_list_scan(a, h->st);
}
// The step both passes run, in two halves around what each pass does with the counts.  First: scan a ScanSet and read its counters (they
// count past the capacity: one read-back tells every row's candidate count)
void scan_counts(const RangeCall& C, const ScanSet& s, std::vector<unsigned long long>& cnts) {
    rsx_index* h = C.h;
    if (C.ivf) scan_ivf(C, s);
    else launch_flat_gemm_filter(s.Q16, (int)s.nq_pad, (int)s.nq, h->data.p, h->storage_f16, 0, h->ntotal, h->ld, C.bias, s.tau, 1, s.cand, s.cnt, s.cap, h->st);
    cnts.resize((size_t)s.nq * CCS);
    HIPCHECK(hipMemcpyAsync(cnts.data(), s.cnt, (size_t)s.nq * 8 * CCS, hipMemcpyDeviceToHost, h->st));
    HIPCHECK(hipStreamSynchronize(h->st));
}
// Second, once the pass has copied the keys each row holds to s.rcnt (at most max_cnt): the back end, exact re-score + membership, ordering
RangeRowsArgs rank_rows(const RangeCall& C, const ScanSet& s, int max_cnt) {
    rsx_index* h = C.h;
    RangeRowsArgs ra{};
    ra.cand = s.cand; ra.cap = s.cap; ra.nrows = s.nq; ra.rcnt = s.rcnt; ra.qsel = s.qsel;
    ra.kind = h->kind; ra.metric = h->metric; ra.radius = C.radius;
    ra.Q32 = h->w_q32.as<float>(); ra.ldq = h->ld; ra.d = h->d; ra.X = h->data.p; ra.x_f16 = h->storage_f16; ra.ld = h->ld;
    ra.probe_list = h->w_probelist.as<int32_t>(); ra.seg_start = h->w_segstart.as<int64_t>(); ra.nprobe = C.nprobe; ra.list_base = h->d_base.as<int64_t>();
    ra.ids = C.ids; ra.nmem = h->w_rg_nmem.as<int32_t>(); ra.max_cnt = max_cnt;
    launch_range_rescore(ra, h->st);
    launch_range_sort(ra, h->st);
    return ra;
}
// keys of a second-pass row for a query the first pass counted m candidates for: a power of two with room for a count that differs in the last bits
int64_t group_row(int64_t m) { return pow2ceil64(m + m / 64 + 16); }

// what the whole call needs: the directory's geometry (IVF), the L2 bias, the scans' bound, the first-pass capacity and the batch size
void plan_call(RangeCall& C) {
    rsx_index* h = C.h;
    if (C.ivf) {
        C.nprobe = std::min(h->nprobe, h->nlist);
        const auto padded = top_probe_sum(h, C.nprobe, 16, 16);      // the nprobe longest lists, padded as the probe set-up pads them
        C.tmax = std::max<int64_t>(round_up(padded.first, 256), 256); C.maxlen = padded.second;
        if (C.nprobe > 4096) RSX_THROW(RSX_ERR_UNSUPPORTED, "range_search: %d probed lists per query exceed this build's maximum of 4096", C.nprobe);
        if (C.tmax >= ((int64_t)1 << 32)) RSX_THROW(RSX_ERR_UNSUPPORTED, "range_search: probed lists exceed 2^32 vectors per query");
    }
    C.t_all.start();
    if (h->metric == RSX_METRIC_L2) C.bias = l2_bias_rows(h);
    C.sb = scan_cert_bound(h);
    // first-pass capacity: "range_cand_cap" (default 65536 keys), a power of two (the sort's network), never more than a query can see
    const int64_t visible = C.ivf ? C.tmax : h->ntotal;
    C.cap1 = (int)std::min<int64_t>((int64_t)1 << 30, pow2ceil64(std::max<int64_t>(64, std::min<int64_t>(h->range_cand_cap > 0 ? h->range_cand_cap : 65536, visible))));
    C.qb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(std::max(1, h->query_batch), 32768), h->temp_budget / ((int64_t)C.cap1 * 8)));
    C.ids = (h->kind == KIND_FLAT && !h->custom_ids) ? nullptr : h->ids.as<int64_t>();
}

// 1. the queries as `search` converts them: fp32 copy, fp16 operand, the "lossy query" flag
void convert_stage(RangeCall& C, const RangeBatch& B) {
    rsx_index* h = C.h;
    const void* dq = (const char*)C.q + (size_t)B.q0 * h->d * (C.dtype == RSX_F16 ? 2 : 4);
    if (!C.q_dev) dq = stage_rows(h, h->w_qin, dq, B.nb, h->d, C.dtype);
    convert_scan_queries(h, dq, C.dtype, B.nb, B.nq_pad);
}
// 2. thresholds (and the counters' reset)
void threshold_stage(RangeCall& C, const RangeBatch& B) {
    rsx_index* h = C.h;
    h->w_tau.ensure((size_t)B.nb * 8); h->w_candcnt.ensure((size_t)B.nb * 8 * CCS);
    RangeTauArgs ta{};
    ta.Q32 = h->w_q32.as<float>(); ta.ldq = h->ld; ta.d = h->d; ta.nq = B.nb; ta.metric = h->metric; ta.radius = C.radius;
    ta.cert_rel = C.sb.rel; ta.cert_rel_qlossy = C.sb.rel_qlossy; ta.cert_xmax = C.sb.xmax; ta.cert_abs = C.sb.abs; ta.cert_qflag = h->w_flag.as<int>();
    ta.tau = h->w_tau.as<uint64_t>(); ta.cand_cnt = h->w_candcnt.as<unsigned long long>();
    launch_range_tau(ta, h->st);
}
// 3. - 5. the scan with the fixed thresholds, the count read-back, the back end on the rows that held; the others go to B.over
void first_pass(RangeCall& C, RangeBatch& B) {
    rsx_index* h = C.h; const int64_t nb = B.nb;
    h->w_cand.ensure((size_t)nb * C.cap1 * 8);
    h->w_rg_cnt.ensure((size_t)nb * 4); h->w_rg_nmem.ensure((size_t)nb * 4); h->w_rg_lims.ensure((size_t)(nb + 1) * 8); h->w_rg_kptr.ensure((size_t)nb * 8);
    const ScanSet s1{h->w_q16.as<__half>(), nb, B.nq_pad, h->w_tau.as<uint64_t>(), h->w_probelist.as<int32_t>(), h->w_segstart.as<int64_t>(),
                     h->w_cand.as<uint64_t>(), h->w_candcnt.as<unsigned long long>(), C.cap1, nullptr, h->w_rg_cnt.as<int32_t>()};
    scan_counts(C, s1, B.cnts);
    C.t_back.start();
    B.rcnt.assign((size_t)nb, 0); B.kptr.assign((size_t)nb, nullptr);
    int max1 = 0;
    for (int64_t i = 0; i < nb; i++) {
        const unsigned long long c = B.cnts[(size_t)i * CCS];
        C.n_cand += (double)c;
        if (c > (unsigned long long)C.cap1) { B.over.push_back(i); continue; }
        B.rcnt[(size_t)i] = (int32_t)c; max1 = std::max(max1, (int)c); B.kptr[(size_t)i] = h->w_cand.as<uint64_t>() + (size_t)i * C.cap1;
    }
    C.n_over += (double)B.over.size();
    HIPCHECK(hipMemcpyAsync(s1.rcnt, B.rcnt.data(), (size_t)nb * 4, hipMemcpyHostToDevice, h->st));
    HIPCHECK(hipMemsetAsync(h->w_rg_nmem.p, 0, (size_t)nb * 4, h->st));      // the batch's member counts start here
    rank_rows(C, s1, max1);
}

// one group of overflowed queries B.over[i0, i1): their fp16 rows, thresholds and probes gathered into a compact batch, scanned and ranked
// in rows of capg keys; the members are kept (sorted keys) until the batch's lims are known
void overflow_group(RangeCall& C, RangeBatch& B, size_t i0, size_t i1, int capg) {
    rsx_index* h = C.h; const int ld = h->ld, nprobe = C.nprobe;
    const int64_t gn = (int64_t)(i1 - i0), gn_pad = gn > 128 ? round_up(gn, 256) : 128;
    DevBuf g_cand, g_cnt, g_q16, g_tau, g_sel, g_rcnt, g_pl, g_ss, g_koff;
    g_cand.ensure((size_t)gn * capg * 8); g_cnt.ensure((size_t)gn * 8 * CCS); g_q16.ensure((size_t)gn_pad * ld * 2); g_tau.ensure((size_t)gn * 8);
    g_sel.ensure((size_t)gn * 4); g_rcnt.ensure((size_t)gn * 4); g_koff.ensure((size_t)gn * 8);
    std::vector<int32_t> sel((size_t)gn), grc((size_t)gn), nmem_h((size_t)B.nb);
    std::vector<unsigned long long> gc;
    for (int64_t r = 0; r < gn; r++) sel[(size_t)r] = (int32_t)B.over[i0 + (size_t)r];
    HIPCHECK(hipMemcpyAsync(g_sel.p, sel.data(), (size_t)gn * 4, hipMemcpyHostToDevice, h->st));
    HIPCHECK(hipMemsetAsync(g_q16.p, 0, (size_t)gn_pad * ld * 2, h->st));
    HIPCHECK(hipMemsetAsync(g_cnt.p, 0, (size_t)gn * 8 * CCS, h->st));
    launch_range_gather_rows(h->w_q16.p, g_q16.p, (int64_t)ld * 2, g_sel.as<int32_t>(), gn, h->st);
    launch_range_gather_rows(h->w_tau.p, g_tau.p, 8, g_sel.as<int32_t>(), gn, h->st);
    if (C.ivf) {
        g_pl.ensure((size_t)gn * nprobe * 4); g_ss.ensure((size_t)gn * (nprobe + 1) * 8);
        launch_range_gather_rows(h->w_probelist.p, g_pl.p, (int64_t)nprobe * 4, g_sel.as<int32_t>(), gn, h->st);
        launch_range_gather_rows(h->w_segstart.p, g_ss.p, (int64_t)(nprobe + 1) * 8, g_sel.as<int32_t>(), gn, h->st);
    }
    const ScanSet sg{g_q16.as<__half>(), gn, gn_pad, g_tau.as<uint64_t>(), g_pl.as<int32_t>(), g_ss.as<int64_t>(), g_cand.as<uint64_t>(),
                     g_cnt.as<unsigned long long>(), capg, g_sel.as<int32_t>(), g_rcnt.as<int32_t>()};
    scan_counts(C, sg, gc);
    // The group may run another form of the scan than the first pass did (query padding, probing queries per list), and nothing pins
    // the two forms' scores to the same bits: any count the row holds is a valid candidate set (both scans obey the same bound).
    // A count past the row cannot be served from it.
    int maxg = 0;
    for (int64_t r = 0; r < gn; r++) {
        if (gc[(size_t)r * CCS] > (unsigned long long)capg)
            RSX_THROW(RSX_ERR_OOM, "range_search: the second scan of a query found %llu candidates for a row of %d (the first scan counted %llu)",
                      gc[(size_t)r * CCS], capg, B.cnts[(size_t)sel[(size_t)r] * CCS]);
        grc[(size_t)r] = (int32_t)gc[(size_t)r * CCS]; maxg = std::max(maxg, grc[(size_t)r]);
    }
    HIPCHECK(hipMemcpyAsync(g_rcnt.p, grc.data(), (size_t)gn * 4, hipMemcpyHostToDevice, h->st));
    RangeRowsArgs rg = rank_rows(C, sg, maxg);
    HIPCHECK(hipMemcpyAsync(nmem_h.data(), h->w_rg_nmem.p, (size_t)B.nb * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHECK(hipStreamSynchronize(h->st));
    std::vector<int64_t> koff((size_t)gn);
    int64_t tot = 0; int maxm = 0;
    for (int64_t r = 0; r < gn; r++) { koff[(size_t)r] = tot; tot += nmem_h[(size_t)sel[(size_t)r]]; maxm = std::max(maxm, (int)nmem_h[(size_t)sel[(size_t)r]]); }
    B.kept.emplace_back(new DevBuf());
    B.kept.back()->ensure((size_t)std::max<int64_t>(tot, 1) * 8);
    HIPCHECK(hipMemcpyAsync(g_koff.p, koff.data(), (size_t)gn * 8, hipMemcpyHostToDevice, h->st));
    rg.max_cnt = maxm;
    launch_range_compact(rg, g_koff.as<int64_t>(), B.kept.back()->as<uint64_t>(), h->st);
    for (int64_t r = 0; r < gn; r++) B.kptr[(size_t)sel[(size_t)r]] = B.kept.back()->as<uint64_t>() + koff[(size_t)r];
    HIPCHECK(hipStreamSynchronize(h->st));      // the group's buffers go away here
}
// the overflowed queries again, rows sized from their counts, in groups the temp budget holds
void overflow_stage(RangeCall& C, RangeBatch& B) {
    for (size_t i0 = 0; i0 < B.over.size();) {
        int64_t maxc = 0; size_t i1 = i0;
        while (i1 < B.over.size()) {
            const int64_t m = std::max<int64_t>(maxc, (int64_t)B.cnts[(size_t)B.over[i1] * CCS]);
            if (m > ((int64_t)1 << 29) || (int64_t)(i1 - i0 + 1) * group_row(m) * 8 > C.h->temp_budget) break;
            maxc = m; i1++;
        }
        if (i1 == i0) RSX_THROW(RSX_ERR_OOM, "range_search: a query has %llu candidates; their row does not fit the temp budget (temp_budget_mb)",
                                B.cnts[(size_t)B.over[i0] * CCS]);
        overflow_group(C, B, i0, i1, (int)group_row(maxc));
        i0 = i1;
    }
}

// counts -> lims (the batch's run on from the previous batch's last), then D / I of the batch at its lims
void emit_stage(RangeCall& C, RangeBatch& B) {
    rsx_index* h = C.h; rsx_range_result* R = C.R; const int64_t nb = B.nb;
    launch_range_lims(h->w_rg_nmem.as<int32_t>(), nb, C.lims[(size_t)B.q0], h->w_rg_lims.as<int64_t>(), h->st);
    std::vector<int64_t> lims_b((size_t)nb + 1);
    HIPCHECK(hipMemcpyAsync(lims_b.data(), h->w_rg_lims.p, (size_t)(nb + 1) * 8, hipMemcpyDeviceToHost, h->st));
    HIPCHECK(hipMemcpyAsync(h->w_rg_kptr.p, B.kptr.data(), (size_t)nb * 8, hipMemcpyHostToDevice, h->st));
    HIPCHECK(hipStreamSynchronize(h->st));
    int maxn = 0;
    for (int64_t i = 0; i < nb; i++) {
        C.lims[(size_t)(B.q0 + i + 1)] = lims_b[(size_t)i + 1];
        maxn = (int)std::max<int64_t>(maxn, lims_b[(size_t)i + 1] - lims_b[(size_t)i]);
    }
    const int64_t tot_b = lims_b[(size_t)nb] - lims_b[0];
    std::unique_ptr<DevBuf> bD(new DevBuf()), bI(new DevBuf());
    if (tot_b > 0) {
        bD->ensure((size_t)tot_b * 4); bI->ensure((size_t)tot_b * 8);
        RangeEmitArgs ea{};
        ea.kptr = h->w_rg_kptr.as<uint64_t*>(); ea.nmem = h->w_rg_nmem.as<int32_t>(); ea.lims = h->w_rg_lims.as<int64_t>(); ea.nq = nb;
        ea.kind = h->kind; ea.metric = h->metric; ea.probe_list = h->w_probelist.as<int32_t>(); ea.seg_start = h->w_segstart.as<int64_t>(); ea.nprobe = C.nprobe;
        ea.list_base = h->d_base.as<int64_t>(); ea.ids = C.ids; ea.D = bD->as<float>(); ea.I = bI->as<int64_t>(); ea.max_cnt = maxn;
        launch_range_emit(ea, h->st);
        launch_range_ties(ea, h->st);
    }
    C.t_back.stop();
    if (tot_b > 0 && !C.q_dev) {
        R->h_D.resize((size_t)lims_b[(size_t)nb]); R->h_I.resize((size_t)lims_b[(size_t)nb]);
        HIPCHECK(hipMemcpyAsync(R->h_D.data() + lims_b[0], bD->p, (size_t)tot_b * 4, hipMemcpyDeviceToHost, h->st));
        HIPCHECK(hipMemcpyAsync(R->h_I.data() + lims_b[0], bI->p, (size_t)tot_b * 8, hipMemcpyDeviceToHost, h->st));
    }
    HIPCHECK(hipStreamSynchronize(h->st));
    if (tot_b > 0 && C.q_dev) { C.chunks.emplace_back(std::move(bD), std::move(bI)); C.chunk_n.push_back(tot_b); }
    C.back_ms += C.t_back.ms();
}

// the call's counters, and lims / D / I handed to the result (device callers: the batches' chunks laid end to end)
void finish_call(RangeCall& C, int64_t nq) {
    rsx_index* h = C.h; rsx_range_result* R = C.R;
    R->total = C.lims[(size_t)nq];
    h->timing["range_calls"] += 1.0;
    h->timing["range_candidates"] += C.n_cand;
    h->timing["range_results"] += (double)R->total;
    h->timing["range_overflow_queries"] += C.n_over;
    if (!C.q_dev) { R->h_lims.swap(C.lims); return; }
    R->d_lims.reset(new DevBuf());
    R->d_lims->ensure((size_t)(nq + 1) * 8);
    HIPCHECK(hipMemcpy(R->d_lims->p, C.lims.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice));
    if (C.chunks.size() == 1) { R->d_D = std::move(C.chunks[0].first); R->d_I = std::move(C.chunks[0].second); }
    else if (!C.chunks.empty()) {
        R->d_D.reset(new DevBuf()); R->d_I.reset(new DevBuf());
        R->d_D->ensure((size_t)R->total * 4); R->d_I->ensure((size_t)R->total * 8);
        int64_t off = 0;
        for (size_t c = 0; c < C.chunks.size(); c++) {
            HIPCHECK(hipMemcpyAsync(R->d_D->as<float>() + off, C.chunks[c].first->p, (size_t)C.chunk_n[c] * 4, hipMemcpyDeviceToDevice, h->st));
            HIPCHECK(hipMemcpyAsync(R->d_I->as<int64_t>() + off, C.chunks[c].second->p, (size_t)C.chunk_n[c] * 8, hipMemcpyDeviceToDevice, h->st));
            off += C.chunk_n[c];
        }
        HIPCHECK(hipStreamSynchronize(h->st));
    }
}

}  // namespace

rsx_range_result* range_impl(rsx_index* h, int64_t nq, const void* q, int dtype, float radius) {
    if (nq < 0) RSX_THROW(RSX_ERR_INVALID, "range_search: nq = %lld", (long long)nq);
    if (!std::isfinite(radius)) RSX_THROW(RSX_ERR_INVALID, "range_search: the radius must be finite");
    if (!h->trained) RSX_THROW(RSX_ERR_NOT_TRAINED, "range_search before train");
    if (nq > 0 && !q) RSX_THROW(RSX_ERR_INVALID, "range_search: null pointer");
    RangeCall C(h, q, dtype, radius);
    if (C.ivf && h->ntotal > 0 && list_scan2_chunk_rows(h->storage_f16, h->ld) == 0)
        RSX_THROW(RSX_ERR_UNSUPPORTED, "range_search: an IndexIVFFlat whose rows are stored as fp32 has no filtered list scan in this build");
    std::unique_ptr<rsx_range_result> R(new rsx_range_result());
    R->nq = nq; R->on_device = C.q_dev ? 1 : 0; R->device = h->device;
    C.R = R.get(); C.lims.assign((size_t)nq + 1, 0);
    if (h->ntotal > 0 && nq > 0) {
        plan_call(C);
        for (int64_t q0 = 0; q0 < nq; q0 += C.qb) {
            const int64_t nb = std::min(C.qb, nq - q0);
            RangeBatch B{q0, nb, nb > 128 ? round_up(nb, 256) : 128};
            convert_stage(C, B);
            if (C.ivf) { coarse_exact_scores(h, nb); coarse_exact_probes(h, nb, C.nprobe, 16); }      // the exact route: the oracle's probe order
            threshold_stage(C, B);
            first_pass(C, B);
            overflow_stage(C, B);
            emit_stage(C, B);
        }
        C.t_all.stop();
        HIPCHECK(hipStreamSynchronize(h->st));
        HIPCHECK(hipGetLastError());
        if (h->profile > 0) { h->timing["range_ms"] += C.t_all.ms(); h->timing["range_backend_ms"] += C.back_ms; }
    }
    finish_call(C, nq);
    return R.release();
}
