// api_search.hip — the search drivers: search_batch (one internal batch: coarse quantiser, probe selection, table build, threshold
// pre-pass, scan, selection, exact re-rank, certificate fallbacks) and search_impl (one rsx_search call).  Shared declarations: rsx_host.h;
// the stages that range_search runs as well: rsx_stages.h.
#include <chrono>
#include <cstring>
#include "rsx_stages.h"

// ---------------------------------------------------------------------------------------
// search
// ---------------------------------------------------------------------------------------
// profile = -1: events around the dominant scan launch ONLY (an event record is ~5 us of stream time: eight marks per batch are 1.5 % of the
// headline batch — bench.py times its `value` in this mode and takes the stage breakdown from a separate pass in mode 1)
struct StageTimer {
    rsx_index* h; bool on; bool scan_only; std::string prefix;
    hipEvent_t ev[64]; const char* name[64]; int n = 0;
    StageTimer(rsx_index* hh, const char* pre = "") : h(hh), on(hh->profile != 0), scan_only(hh->profile == -1), prefix(pre) {}
    void record(const char* nm) {
        (void)hipEventCreate(&ev[n]);
        (void)hipEventRecord(ev[n], h->st);
        name[n] = nm; n++;
    }
    void mark(const char* nm) {
        if (!on || n >= 64) return;
        if (scan_only && !(n == 1 && std::strcmp(nm, "scan") == 0)) return;
        record(nm);
    }
    void pre_scan() { if (on && scan_only && n == 0) record("prescan"); }      // right before the dominant scan's launch
    void finish() {
        if (!on || n == 0) return;
        (void)hipEventSynchronize(ev[n - 1]);
        for (int i = 1; i < n; i++) {
            float ms = 0; (void)hipEventElapsedTime(&ms, ev[i - 1], ev[i]);
            h->timing[prefix + name[i]] += ms;
        }
        float tot = 0; (void)hipEventElapsedTime(&tot, ev[0], ev[n - 1]);
        h->timing[prefix + "total"] += tot;
        for (int i = 0; i < n; i++) (void)hipEventDestroy(ev[i]);
        n = 0;
    }
};

static void kp_for(const rsx_index* h, int k, bool fast, int& KP, int& BUF) {
    int want;
    // fast IVF-PQ scan: K' = the candidates re-scored exactly per query.  With the round-3 threshold (k_pq_prepass: the sample's
    // k-th best approximate score minus 2 eps) the scan admits what the data needs — measured on the bench mixture ~130 keys
    // for k = 10, ~500 for k = 100, ~2300 for k = 1000, ~3400 for k = 2000 — and K' only has to hold them: 3k, at least
    // k + 118, at most 4096 (k_finalize sorts K' candidates in LDS).  A query with more candidates keeps its best K' by
    // approximate score and is still certified against the K'-th one (k_finalize) or re-run exactly.
    if (h->kind == KIND_IVFPQ && fast) want = h->pq_fast_kp > 0 ? std::max(k, h->pq_fast_kp) : std::min(4096, std::max(k + 118, 3 * k));
    else if (h->kind == KIND_IVFPQ) want = (k >= 512) ? k : k + 4;
    else want = k + std::max(8, k / 16);
    KP = std::max(16, pow2ceil(want));
    BUF = std::max(2 * KP, (h->kind == KIND_IVFPQ && fast) ? 512 : 256);
}

// filtered search (h->sel): -inf over the unselected columns of Flat score rows [nq, tstride] whose column c is slot slot0 + c
static void sel_apply_flat(rsx_index* h, float* temp, int64_t tstride, int64_t nq, int64_t n, int64_t slot0) {
    if (!h->sel) return;
    SelApplyArgs sa{};
    sa.temp = temp; sa.tstride = tstride; sa.nq = nq; sa.mask = h->sel_mask.as<uint32_t>(); sa.flat_n = n; sa.slot0 = slot0;
    launch_sel_apply(sa, h->st);
}

// ---------------------------------------------------------------------------------------
// the batch plan: every route decision of one internal batch, made once (plan_batch)
// ---------------------------------------------------------------------------------------
struct BatchPlan {
    int64_t nq, nq_pad; int k; bool allow_fast;     // nq_pad: query tiles of 128 (k_flat_gemm) or 256 (k_flat_gemm2)
    bool rot, sliced;          // IVF-PQ block layouts (rotated, sliced): transposed tables, work-item scans
    bool fast;                 // the IVF-PQ 8-bit fast scan: approximate scores, certified in k_finalize
    int KP, BUF;               // selection state: K' keys per query, the selection's buffer
    bool certify;              // Flat / IVF-Flat: the fp16 scans are certified and the uncertain queries re-run exactly
    bool coarse_fast, q16_direct;
    bool pq_fused_lut, tab_expected, lut_pass0_early;
    bool sl_eight; int ngq;    // sliced layout: eight queries per gather; 4-query records per work item of the filtered scan
    // the in-scan candidate filters in effect: the knobs, all off for a filtered search (h->sel), which takes the routes whose scans write
    // complete score rows
    int flat_filter, ivf_filter, pq_filter;
    int nprobe, pad_to;        // IVF: probed lists per query; list padding of the score rows
    int64_t tmax, maxlen;      // IVF: a query's score row (the nprobe longest padded lists, at least 256) and the longest of those lists
    bool needs_score_rows;     // the IVF-PQ fast scan with in-kernel filtering and the one-launch threshold pre-pass never writes a score row
    bool staged;               // IndexPQ (rsx_index::flat_pq): the staged filtered scan over the one list (pq_staged_scan)
};
static BatchPlan plan_batch(rsx_index* h, int64_t nq, const void* dq, int dtype, int k, bool allow_fast) {
    BatchPlan P{};
    const bool pq = h->kind == KIND_IVFPQ;
    P.nq = nq; P.nq_pad = nq > 128 ? round_up(nq, 256) : 128; P.k = k; P.allow_fast = allow_fast;
    P.flat_filter = h->sel ? 0 : h->flat_filter; P.ivf_filter = h->sel ? 0 : h->ivf_filter; P.pq_filter = h->sel ? 0 : h->pq_filter;
    P.rot = pq && pq_rot_family(h->CB); P.sliced = pq && h->CB == PQ_SLICED;
    P.nprobe = std::min(h->nprobe, h->nlist);
    // IVFPQ fast path: needs the 16-byte-granule layout, 16-bit integer sums, and K' <= 4096.  The sliced layout has ONE fast kernel: the
    // filtered scan behind the one-launch pre-pass (every other setting takes the exact scan)
    // METRIC_L2: the table depends on the (query, list) pair, so IVF-PQ keeps the exact scan (k_pq_scan_l2) — but an IndexPQ is one list with a
    // ZERO centroid: a per-query table again, built negated (k_pq_lut8f<_, true>), and served by the staged scan below or not at all
    const bool l2 = h->metric == RSX_METRIC_L2;
    P.fast = allow_fast && pq && (!l2 || h->flat_pq) && h->pq_fast != 0 && h->scan_kernel == 0 && (h->CB == 16 || pq_rot_family(h->CB)) && h->M * 255 < 65536;
    if (P.fast) { kp_for(h, k, true, P.KP, P.BUF); if (P.KP > 4096) P.fast = false; }
    // IndexPQ: one list scanned by every query — the work-item scans of the block layouts, in stages (no score rows).  Every
    // other layout and setting of such a handle takes the one-list IVF-PQ routes (score rows cut by the temp budget) and is as correct
    P.staged = P.fast && h->flat_pq && P.rot && P.pq_filter != 0 && h->pq_prepass_fused != 0 && h->M == h->Mpad && pq_rot_applies(h->M);
    // (L2: the negated table comes from the VALU builders, and the per-query one must be available — every M the staged route admits fits its LDS up to dsub 60)
    if (l2 && !(P.staged && pq_lut8_fused_lds(h->M, h->Mpad, h->dsub) <= 160 * 1024 - 64)) P.fast = P.staged = false;
    if (P.fast && P.sliced && !((P.nprobe > 1 || P.staged) && P.pq_filter != 0 && h->pq_prepass_fused != 0)) P.fast = false;
    kp_for(h, k, P.fast, P.KP, P.BUF);
    P.certify = h->kind != KIND_IVFPQ && allow_fast && h->flat_cert != 0;
    // fast coarse quantiser (round 6): fp16 MFMA scores of all lists + exact chains of the candidates; needs the re-run machinery behind it
    P.coarse_fast = h->kind != KIND_FLAT && allow_fast && h->coarse_fast != 0 && (pq ? P.fast : P.certify) && nq >= 32 &&
                    P.nprobe <= CP_MAXPROBE && h->nlist <= CP_MAXLIST && h->nlist > P.nprobe && !h->h_centroids.empty() &&
                    coarse_pick_lds(h->nlist, h->d, P.nprobe) <= 150 * 1024;
    // ... whose fp16 operand is the caller's own batch when that is fp16, unpadded (d = ld) and whole tiles: the fp32 copy then rides in the
    // GEMM's launch (extra grid rows) instead of a conversion launch of its own
    P.q16_direct = pq && P.coarse_fast && dtype == RSX_F16 && h->d == h->ld && nq % 128 == 0 && ((uintptr_t)dq & 15) == 0;
    P.pq_fused_lut = pq && P.fast && pq_lut8_fused_lds(h->M, h->Mpad, h->dsub) <= 160 * 1024 - 64;
    // the finalize-from-the-row kernel (k_pq_final_tab) will serve this batch: let the table builder store the fp32 tables for it
    // (M KiB per query, 100 MB at M = 96 / batch 1024) instead of every query's workgroup re-deriving its table from the 786 KB codebook
    P.tab_expected = P.pq_fused_lut && P.rot && h->pq_final_tab != 0 && (h->pq_final_tab == 2 || P.KP >= 512 || h->dsub > 8) &&
                     (P.nprobe > 1 || P.staged) && P.pq_filter != 0 && h->pq_prepass_fused != 0 && pq_final_tab_capacity(h->M, h->CB, k) > 0;
    // L2 always stores them: every exact re-score (k_finalize, k_pq_rescore_all, k_pq_final_tab) then READS its entries, and the code that
    // re-derives inner-product entries from the codebook needs no second metric
    P.tab_expected = P.tab_expected || (P.fast && l2);
    // the matrix-core table build will serve this batch and the fast coarse quantiser runs: its first pass rides in the probe-pick launch
    P.lut_pass0_early = P.coarse_fast && P.pq_fused_lut && h->dsub == 8 && h->lut_tiled != 0 && h->metric == RSX_METRIC_INNER_PRODUCT &&
                        h->pq_lut_early != 0;
    // sliced layout: eight queries per gather (two records per item) where lists are long and shared by several queries; a handful of
    // queries (about one per probed list) or short lists take the four-query single-pass scan (k_pq_scan_sl4).  pq_q8: 1 = choose,
    // 2 = always eight, 0 = always four
    P.sl_eight = P.sliced && (h->pq_q8 == 2 || (h->pq_q8 != 0 && nq * (int64_t)P.nprobe >= (int64_t)3 * h->nlist && h->ntotal >= (int64_t)4096 * h->nlist));
    P.ngq = P.sliced ? (P.sl_eight ? 2 : 1) : P.rot ? pq_scan_rot_ngq(h->M, true, h->pq_q8) : 1;     // (M = 16: 4)
    if (h->kind != KIND_FLAT) {
        P.pad_to = pq ? 64 : 16;
        const auto padded = top_probe_sum(h, P.nprobe, P.pad_to, P.pad_to);    // the nprobe longest lists, padded: sum and maximum
        P.tmax = std::max<int64_t>(round_up(padded.first, 256), 256); P.maxlen = padded.second;
    }
    // score rows [nq, tmax]: every path but the filtered IVF-PQ fast scan with the one-launch pre-pass fills (part of) them.  At the
    // reference's nprobe 512 a row is 35 MB: allocating it unconditionally used to cut a 1024-query batch into four internal
    // batches (round 4: 4x the fixed stages, a quarter of the queries per list group)
    P.needs_score_rows = !(P.fast && (P.nprobe > 1 || P.staged) && P.pq_filter != 0 && h->pq_prepass_fused != 0);
    return P;
}
// Keys a query's candidate row can hold (filtered IVF-PQ fast scan, filtered IVF-Flat list scan).  The IVF-PQ threshold is valid by
// construction, so the row must hold every vector within 2 eps of the query's k-th best: ~700 keys at M = 96 / k = 10, but
// eps grows as the tables get coarser — at M = 16 (48 dimensions per 8-bit table entry) the measured mean is 1800 and the maximum 23 000
// at k = 10.  An overflowing row sends its query to the exact re-run, so small M gets four times the room (8 B x nq x cap of HBM).
// M = 0: rows of full vectors (IVF-Flat).
static int64_t cand_row_cap(int k, int M) {
    int64_t cap = k > 512 ? 131072 : (k > 64 ? 65536 : 16384);
    if (M > 0 && M <= 32) cap = std::min<int64_t>(cap * 4, 262144);
    return cap;
}
// the candidate rows [nq, cap] and their counters; returns cap (never more than a score row)
static int alloc_cand_rows(rsx_index* h, const BatchPlan& P, int M) {
    const int cap = (int)std::min<int64_t>(std::max<int64_t>(P.tmax, 1024), cand_row_cap(P.k, M));
    h->w_cand.ensure((size_t)P.nq * cap * 8);
    h->w_candcnt.ensure((size_t)P.nq * 8 * CCS);
    return cap;
}
// merge key rows [nrows, cap] (row r holds cnt[r * CCS] keys) into state rows [nrows, KP]: one wave per row, the whole row one segment
static void merge_key_rows(rsx_index* h, const void* keys, const unsigned long long* cnt, int cap, int64_t nrows, const uint64_t* init,
                           uint64_t* out, int KP, int BUF, const int32_t* row_filter = nullptr) {
    SelectArgs b{};
    b.in = keys; b.in_is_keys = 1; b.row_stride = cap;
    b.row_n = reinterpret_cast<const int64_t*>(cnt); b.row_n_stride = CCS; b.n_uniform = cap;
    b.seg_len = round_up(cap, 256); b.nseg = 1; b.idx_base = 0;
    b.init = init; b.out = out; b.out_row_stride = KP;
    b.nrows = nrows; b.KP = KP; b.BUF = BUF; b.k = KP; b.row_filter = row_filter;
    launch_select(b, h->st);
}
// what one batch's stages leave for the later ones
struct BatchResult {
    bool filtered = false;         // in-kernel candidate filtering: candidate rows instead of score rows
    bool fused_pre_used = false;   // ... whose threshold came from the one-launch pre-pass (complete candidate rows: second chance)
    int cand_cap = 0;
    bool use_gather = false; PQGatherArgs gs{};   // ... whose candidates are gathered and selected in one launch
    bool flag_overflows = false;   // IVF-Flat filtered scan: a few candidate rows overflowed — k_finalize sends their queries to the exact re-run
    bool tab_fits = false, use_tab = false;     // k_pq_final_tab can settle the candidate rows / finalizes this batch
};
static void search_batch(rsx_index* h, int64_t nq, const void* dq, int dtype, int k, float* dD, int64_t* dI, bool allow_fast = true);
// Queries whose certificate failed (h->w_uncertain, written by k_finalize) are re-run through the exact path of their index
// kind and their result rows replaced — rare, and what makes the fast paths EXACT rather than "almost always right".
// temp_bytes_per_query > 0 bounds the exact path's score buffer (Flat / IVF-Flat): the re-run proceeds in chunks.
// coarse_live: the batch's k_coarse_pick wrote per-query flags behind the certificate's.
static void rerun_uncertified(rsx_index* h, int64_t nq, const void* dq, int dtype, int k, float* dD, int64_t* dI,
                              size_t temp_bytes_per_query, bool coarse_live, const std::function<void()>& second_chance = nullptr) {
    std::vector<int32_t> bad_v;
    const int32_t* bad;
    auto read_flags = [&]() {
        // the fast coarse quantiser's per-query flags (k_coarse_pick: 2 = its candidate row overflowed or a score was not finite) sit behind the
        // certificate's [nq, 2 nq): one copy fetches both, and a flagged query goes to the exact re-run whatever the certificate said
        // (the flag words live in page-locked host memory mapped into the device: the kernels wrote them across the bus, no copy command)
        const size_t words = (size_t)nq * (coarse_live ? 2 : 1);
        int32_t* dst;
        if (h->w_uncertain.host_mapped) {
            HIPCHECK(hipStreamSynchronize(h->st));
            bad_v.assign(h->w_uncertain.as<int32_t>(), h->w_uncertain.as<int32_t>() + words);
            dst = bad_v.data();
        } else {
            if (nq <= 4096 && h->pin_flags.ensure(8192 * 4)) dst = h->pin_flags.as<int32_t>();
            else { bad_v.resize(words); dst = bad_v.data(); }
            HIPCHECK(hipMemcpyAsync(dst, h->w_uncertain.p, words * 4, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipStreamSynchronize(h->st));
        }
        if (coarse_live)
            for (int64_t q = 0; q < nq; q++) if (dst[(size_t)(nq + q)]) { dst[(size_t)q] |= 2; h->timing["coarse_redo_queries"] += 1.0; }
        bad = dst;
    };
    read_flags();
    if (second_chance) {
        // flag 1 = the certificate could not clear the query although none of its candidates was dropped: every vector that
        // can matter is still in its candidate row — re-rank from a larger K' there before paying for an exact scan
        int64_t n1 = 0;
        for (int64_t q = 0; q < nq; q++) n1 += bad[(size_t)q] == 1;
        if (n1 > 0) {
            h->timing["second_chance_queries"] += (double)n1;
            second_chance();
            read_flags();
        }
    }
    const int d = h->d;
    const size_t esz = dtype == RSX_F16 ? 2 : 4;
    std::vector<int64_t> badq;
    int64_t n_over = 0;
    for (int64_t q = 0; q < nq; q++) if (bad[(size_t)q]) {
        badq.push_back(q); n_over += (bad[(size_t)q] & 2) != 0;
        if (bad[(size_t)q] & 4) { h->timing["fallback_tie_queries"] += 1.0; h->timing["fallback_tie_max"] = std::max(h->timing["fallback_tie_max"], (double)(bad[(size_t)q] >> 8)); }
    }
    h->timing["fallback_overflow_queries"] += (double)n_over;     // of the fallbacks: candidate buffer / survivor segment overflows
    const int64_t nbad = (int64_t)badq.size();
    h->timing["fallback_queries"] += (double)nbad;
    h->timing["fast_queries"] += (double)nq;
    if (nbad == 0) return;
    int64_t chunk = nbad;
    if (temp_bytes_per_query > 0) chunk = std::max<int64_t>(1, std::min<int64_t>(nbad, (int64_t)(((size_t)2 << 30) / temp_bytes_per_query)));
    const size_t qrow = (size_t)d * esz;
    h->w_fbq.ensure((size_t)chunk * qrow);
    h->w_fbD.ensure((size_t)chunk * k * 4);
    h->w_fbI.ensure((size_t)chunk * k * 8);
    for (int64_t c0 = 0; c0 < nbad; c0 += chunk) {
        const int64_t nb = std::min(chunk, nbad - c0);
        // gather the uncertified queries into one contiguous batch, search it exactly, scatter the rows back
        for (int64_t i = 0; i < nb; i++)
            HIPCHECK(hipMemcpyAsync((char*)h->w_fbq.p + (size_t)i * qrow, (const char*)dq + (size_t)badq[(size_t)(c0 + i)] * qrow, qrow,
                                    hipMemcpyDeviceToDevice, h->st));
        search_batch(h, nb, h->w_fbq.p, dtype, k, h->w_fbD.as<float>(), h->w_fbI.as<int64_t>(), false);
        for (int64_t i = 0; i < nb; i++) {
            HIPCHECK(hipMemcpyAsync(dD + badq[(size_t)(c0 + i)] * k, h->w_fbD.as<float>() + i * k, (size_t)k * 4, hipMemcpyDeviceToDevice, h->st));
            HIPCHECK(hipMemcpyAsync(dI + badq[(size_t)(c0 + i)] * k, h->w_fbI.as<int64_t>() + i * k, (size_t)k * 8, hipMemcpyDeviceToDevice, h->st));
        }
    }
}
// queries: fp32 copy (exact re-rank, coarse quantiser, LUT) [nq, ld]; fp16 copy for the scans
static void convert_queries(rsx_index* h, const BatchPlan& P, const void* dq, int dtype, StageTimer& tm) {
    const int64_t nq = P.nq; const int d = h->d, ld = h->ld;
    if (h->kind != KIND_IVFPQ) convert_scan_queries(h, dq, dtype, nq, P.nq_pad);
    else {
        h->w_q32.ensure((size_t)nq * ld * 4);
        if (!P.coarse_fast) launch_convert_to_f32(dq, dtype == RSX_F16, d, nq, d, h->w_q32.as<float>(), ld, h->st);
        else if (!P.q16_direct) {
            h->w_q16.ensure((size_t)round_up(nq, 128) * ld * 2);
            launch_convert_to_f32_f16(dq, dtype == RSX_F16, d, nq, d, h->w_q32.as<float>(), h->w_q16.as<__half>(), ld, round_up(nq, 128), h->st);
        }
    }
    h->w_state.ensure((size_t)nq * P.KP * 8);
    if (!P.q16_direct) tm.mark("convert");       // (nothing was launched for it otherwise: the widening rides in the coarse GEMM)
}
// the fp32 tables k_pq_final_tab reads, stored by the table builder (plan: tab_expected; search_batch sizes them)
static float* lut32_out(rsx_index* h, const BatchPlan& P) { return P.tab_expected ? h->w_lut.as<float>() : nullptr; }
// everything that can refuse this search is checked BEFORE work is forked onto the side stream
static void check_supported(rsx_index* h, const BatchPlan& P) {
    if (h->kind == KIND_FLAT) return;
    if (P.nprobe > 4096) RSX_THROW(RSX_ERR_UNSUPPORTED, "search: %d probed lists per query exceed this build's maximum of 4096", P.nprobe);
    if (P.tmax >= ((int64_t)1 << 32)) RSX_THROW(RSX_ERR_UNSUPPORTED, "probed lists exceed 2^32 vectors per query");
    // IndexPQ: ONE list.  The list-wide scans address a list's codes with 32-bit byte offsets (an inverted list never comes near 2 GiB); past
    // that only the routes that do not are served: the staged scan (a tile per item), k_pq_scan_rot_exact and k_pq_scan_l2 (64-bit row addresses)
    if (h->flat_pq && h->h_len[0] * (int64_t)h->Mpad >= ((int64_t)1 << 31) && !(P.staged || (!P.fast && (P.rot || h->metric == RSX_METRIC_L2))))
        RSX_THROW(RSX_ERR_UNSUPPORTED, "IndexPQ: %lld x %d bytes of codes are served by the staged scan and the exact scans of the rotated / sliced layouts only "
                  "(this search was routed elsewhere: M = %d, pq_layout, pq_fast / pq_filter / scan_kernel)", (long long)h->h_len[0], h->Mpad, h->M);
}
// the table build's arguments; its caller adds probe_dis0 / nprobe, pass0_done, pg
static PQLutArgs pq_lut_args(rsx_index* h, const BatchPlan& P, void* lut_ws) {
    PQLutArgs a{};
    a.lut32 = P.pq_fused_lut ? nullptr : h->w_lut.as<float>();
    a.Q32 = h->w_q32.as<float>(); a.ldq = h->ld; a.codebooks = h->d_codebooks.as<float>(); a.dsub = h->dsub; a.nq = P.nq; a.M = h->M; a.Mpad = h->Mpad;
    a.lut8 = h->w_lut8.as<uint8_t>(); a.qparam = h->w_qparam.p; a.ws = lut_ws;
    a.transposed = P.sliced ? 2 : P.rot ? 1 : 0; a.metric = h->metric; a.lut32_out = lut32_out(h, P);
    return a;
}
// the stored rows of a KIND_IVFSQ index, as the exact re-scores decode them
static SqRows sq_rows(rsx_index* h) {
    return SqRows{h->data.as<uint8_t>(), h->d_sq.as<float>(), h->by_residual ? h->d_centroids.as<float>() : nullptr, h->d_base.as<int64_t>(), h->nlist};
}
static FinalizeArgs finalize_args(rsx_index* h, const BatchPlan& P, float* dD, int64_t* dI) {
    const int d = h->d, ld = h->ld;
    FinalizeArgs fa{};
    fa.kind = h->kind; fa.metric = h->metric; fa.state = h->w_state.as<uint64_t>(); fa.KP = P.KP; fa.k = P.k; fa.nq = P.nq;
    fa.list_base = h->d_base.as<int64_t>(); fa.ids = (h->kind == KIND_FLAT && !h->custom_ids) ? nullptr : h->ids.as<int64_t>();
    fa.Q32 = h->w_q32.as<float>(); fa.ldq = ld; fa.d = d;
    fa.X = h->data.p; fa.x_f16 = h->storage_f16; fa.ld = ld; fa.D = dD; fa.I = dI;
    if (P.certify) {
        // Flat / IVF-Flat re-score rows of 2 d bytes that sit anywhere in HBM: only the k + max(8, k / 16) best approximate candidates the
        // certificate needs, not the power of two the selection and the sort round them up to (round 5: k = 1000 re-read 2048 rows per query)
        // (only where the certificate runs: with flat_cert = 0 there is no second pass, and the uncertified mode keeps re-ranking all
        //  K' candidates as it always did: ADVICE r5)
        fa.KPv = std::min(P.KP, P.k + std::max(8, P.k / 16));
        // |approx - exact| of the fp16-MFMA scan for any stored vector: scan_cert_bound (derived there)
        const ScanBound sb = scan_cert_bound(h);
        h->w_uncertain.ensure((size_t)P.nq * 8);
        fa.uncertain = h->w_uncertain.as<int32_t>(); fa.cert_qflag = h->w_flag.as<int>();
        fa.cert_rel = sb.rel; fa.cert_rel_qlossy = sb.rel_qlossy; fa.cert_xmax = sb.xmax; fa.cert_abs = sb.abs;
    }
    if (h->kind == KIND_IVFSQ) {
        fa.sq = sq_rows(h);
        fa.X = nullptr;
        if (P.certify) {
            // The scan's score of a stored vector x^ (k_sq_list_scan) is  (sum_j (hi_j + lo_j) b_j) / s + const_q (+ <q, c_l>) (+ -|x^|^2/2)
            // with b_j = code_j - 128, q'_j = q_j vdiff_j / 255, (hi, lo) the fp16 split of q' s, const_q = sum_j q_j vmin_j + 128.5 sum_j q'_j;
            // the exact score is the fp64 product of q with x^_j = fl(c_lj + fl(vmin_j + fl(vdiff_j fl((code_j + 0.5) / 255)))).  Per unit of |q|,
            // with r = max_j vdiff_j / 255 (|q'| <= r |q|), B = the largest |b| of a stored row (tracked by the encoder), V = |vdiff|, W = |vmin|,
            // C = the largest centroid norm, X = the largest |x^| (Cauchy-Schwarz: sum_j |q'_j b_j| <= |q'| B):
            //   fp32 accumulation of the 2 ld products of a row (hi and lo)               (2 d + 2) 2^-24 r B
            //   the split: |q' s - hi - lo| <= 2^-22 |q' s|                                2^-21 r B        (2^-22 (1 + 2^-11), rounded up)
            //   ... or <= 2^-14 where a half is below the fp16 normal range (s puts the largest |q'_j| at >= 2^13)   sqrt(d) 2^-27 r B
            //   q' itself: two fp32 roundings                                              2 2^-24 r B
            //   the decode's three roundings (|x^_j - its real-number value| <= 2^-24 (3 |vdiff_j| + |vmin_j|)), const_q rounded to fp32
            //   (|const_q| <= |q| (W + V)), the three fp32 operations that assemble the score  10 2^-24 (V + W)
            //   by_residual: the coarse score <q, c_l> is a chain of d fp32 fmaf, it enters two of those operations, and c + r^ is rounded   2^-24 ((d + 4) C + 2 X)
            // No term for the queries' own precision: the factors come from the fp32 queries.  cert_abs (the score's own fp32 rounding, the L2
            // norm term) stays as for stored rows.  tests/sq_ref.py restates this bound (cert_eps) for the host-side precondition test.
            const float u24 = 5.9604645e-8f, fd = (float)d;
            const float rel_b = ((2.0f * fd + 2.0f) * u24 + 4.76837158e-7f + sqrtf(fd) * 7.4505806e-9f + 2.0f * u24) * 1.01f;
            const float rB = (h->sq_vdmax / 255.0f) * sqrtf((float)h->sq_bn2) * 1.00001f;
            float cq = rel_b * rB + 10.0f * u24 * 1.01f * (h->sq_nvdiff + h->sq_nvmin);
            if (h->by_residual) cq += u24 * 1.01f * ((fd + 4.0f) * cent_cmax(h) + 2.0f * fa.cert_xmax);
            fa.cert_rel = 0.0f; fa.cert_rel_qlossy = 0.0f; fa.cert_q = cq;
        }
    }
    return fa;
}
// exact mode (allow_fast = false) and small batches: whole score rows, then one selection
static void flat_score_rows(rsx_index* h, const BatchPlan& P, const float* bias, StageTimer& tm) {
    const int64_t nq = P.nq, N = h->ntotal, tstride = round_up(N, 16); const int ld = h->ld;
    h->w_temp.ensure((size_t)nq * tstride * 4);
    if (!P.allow_fast) {
        // exact mode (queries the certificate could not clear): fp64 scores of every row, rounded once = the canonical
        // scores themselves, then the ordinary selection
        ExactScoreArgs ea{};
        ea.kind = KIND_FLAT; ea.metric = h->metric; ea.nq = nq; ea.Q32 = h->w_q32.as<float>(); ea.ldq = ld; ea.d = h->d;
        ea.X = h->data.p; ea.x_f16 = h->storage_f16; ea.ld = ld; ea.flat_n = N;
        ea.temp = h->w_temp.as<float>(); ea.tstride = tstride;
        launch_exact_scores(ea, h->st);
    } else {
        // small batch: stream the database once per group of 16 queries (list-scan kernel)
        ListScanArgs a{};
        a.Q16 = h->w_q16.as<__half>(); a.ld = ld; a.X = h->data.p; a.x_f16 = h->storage_f16; a.bias = bias;
        a.list_base = h->d_base.as<int64_t>(); a.list_len = h->d_len.as<int64_t>();
        a.flat_mode = 1; a.flat_n = N; a.nq = (int)nq; a.nprobe = 1; a.nlist = 1;
        a.temp = h->w_temp.as<float>(); a.tstride = tstride;
        a.chunk_rows = 1024;
        if (list_scan2_chunk_rows(h->storage_f16, ld) > 0 && round_up(N, 16) / list_scan2_chunk_rows(h->storage_f16, ld) < 65535)
            a.chunk_rows = list_scan2_chunk_rows(h->storage_f16, ld);     // LDS-DMA streaming kernel
        a.max_groups = (int)((nq + 15) / 16);
        a.max_chunks = (int)((round_up(N, 16) + a.chunk_rows - 1) / a.chunk_rows);
        if (a.max_chunks > 65535) { a.chunk_rows = (int)round_up((round_up(N, 16) + 65534) / 65535, 64); a.max_chunks = (int)((round_up(N, 16) + a.chunk_rows - 1) / a.chunk_rows); }
        launch_list_scan(a, h->st);
    }
    sel_apply_flat(h, h->w_temp.as<float>(), tstride, nq, N, 0);      // filtered search: the unselected rows leave the score rows
    tm.mark("scan");
    // threshold = the KP-th approximate key (not the k-th): the exact re-rank needs the true top-KP
    select_rows(h, h->w_temp.as<float>(), tstride, nullptr, 0, N, 0, nq, P.KP, P.BUF, P.KP, h->w_state.as<uint64_t>(), false);
    tm.mark("select");
}
// full batches: chunked GEMM — a threshold phase through the score buffer, then filtered GEMM stages (fa: their deferred counters)
static void flat_staged(rsx_index* h, const BatchPlan& P, const float* bias, FinalizeArgs& fa, StageTimer& tm) {
    const int64_t nq = P.nq, N = h->ntotal, CH = 65536; const int ld = h->ld, KP = P.KP;
    uint64_t* state = h->w_state.as<uint64_t>();
    h->w_temp.ensure((size_t)P.nq_pad * CH * 4);
    launch_fill_u64(state, nq * KP, 0, h->st);
    // chunk 0 through the score buffer: its top-K' gives every query a running threshold
    int64_t done_rows = 0;
    auto chunk_pass = [&](int64_t v0, int64_t vend) {
        int64_t nv = std::min<int64_t>(CH, vend - v0);
        launch_flat_gemm(h->w_q16.as<__half>(), (int)P.nq_pad, h->data.p, h->storage_f16, v0, nv, ld, bias,
                         h->w_temp.as<float>(), CH, h->st);
        sel_apply_flat(h, h->w_temp.as<float>(), CH, nq, nv, v0);
        select_rows(h, h->w_temp.as<float>(), CH, nullptr, 0, nv, (uint32_t)v0, nq, KP, P.BUF, KP, state, true);
    };
    // Threshold phase: the K'-th key of the first rows is a threshold for everything behind them, so a filtered pass over
    // the rows [a, b) keeps ~K' (b - a) / a keys per query.  One 65536-row chunk is right for k = 10 (K' = 32: 5 k keys at
    // 10M rows).  For the reference's n_docs = 1000 (K' = 2048) one chunk let 310 k keys through, overflowed every candidate row
    // and fell back to 153 chunk passes (550 ms per batch, round 4); 160 K' rows and ONE filtered launch over the rest still
    // emitted 62 k keys per query — 64 M atomically placed keys, the filtered GEMM 27.8 instead of 17.4 ms — behind five
    // chunk selections of 0.93 ms.  Now: flat_pre_mult x K' rows through the score buffer (default 16, in units: below), then the rest
    // in STAGES of geometrically growing row ranges, each one filtered launch + one selection that tightens the threshold for
    // the next: S stages of ratio r = (N / first)^(1/S) emit ~S K' (r - 1) keys.  Measured at 10M x 768, batch 1024
    // (profiles/r04_flat_staged_filter.md): k = 1000 36.5 -> 23.3 ms (S = 5), k = 10 18.9 -> 17.2 ms (S = 2: even 5 k keys
    // per query cost the single filtered launch 1.6 ms), k = 100 17.8 ms.
    // (round 6: for small K' the threshold phase and the stage boundaries count in UNITS of a quarter chunk — at K' = 32 the selection
    //  over a full 65536-column chunk cost 0.43 ms of a 16.9 ms batch, four times what a 16384-row threshold phase needs; the
    //  stages pass ~1.5 k keys per query instead of ~700, which the queued epilogue does not notice.  Larger K': half a chunk and 16 K' rows —
    //  k = 1000: scan0 1.32 -> 0.62 ms, one stage more, 20.07 -> 19.68 ms per batch (profiles/r06_large_k_flat.md).  flat_pre_unit: rows, 0 = default)
    const int64_t U = h->flat_pre_unit > 0 ? std::min<int64_t>(CH, round_up(h->flat_pre_unit, 256)) : (KP <= 64 ? CH / 4 : CH / 2);
    const int64_t nchunks = (N + U - 1) / U;          // ... in units
    const int64_t n0 = std::min<int64_t>(nchunks, std::max<int64_t>(1, ((int64_t)KP * std::max(1, h->flat_pre_mult) + U - 1) / U));
    for (int64_t c = 0; c < n0; c++) chunk_pass(c * U, std::min<int64_t>(N, (c + 1) * U));
    done_rows = std::min<int64_t>(n0 * U, N);
    tm.mark("scan0");
    if (done_rows < N && P.flat_filter != 0) {
        int S = h->flat_stages;
        if (S <= 0) S = KP <= 64 ? 2 : std::min(6, std::max(1, (int)lround(log((double)nchunks / (double)n0) / log(3.0))));
        const double r = pow((double)nchunks / (double)n0, 1.0 / S);
        const int cap = KP <= 64 ? 32768 : 131072;
        h->w_cand.ensure((size_t)nq * cap * 8);
        // With the certificate behind it (the default) a stage does not wait for its counts: every stage owns a set of per-query
        // counters, the selection clamps an overflowed row to the buffer, and k_finalize flags a query any of whose stage rows
        // overflowed — it joins the exact re-run like a query the certificate could not clear.  Round 6: the count read-back +
        // host synchronisation per stage (five at the reference's n_docs = 1000) left the GPU idle between the stages.
        // flat_cert = 0 has no re-run behind it and keeps the per-stage check (an overflowed stage is redone chunk by chunk).
        const bool deferred = P.certify;
        const size_t cc_stride = (size_t)nq * CCS;
        h->w_candcnt.ensure(cc_stride * 8 * (deferred ? (size_t)S : 1));
        if (deferred) HIPCHECK(hipMemsetAsync(h->w_candcnt.p, 0, cc_stride * 8 * (size_t)S, h->st));
        std::vector<unsigned long long> cnts(deferred ? 0 : cc_stride);
        int stages_run = 0;
        for (int st_ = 0; st_ < S && done_rows < N; st_++) {
            // stage boundaries on chunk multiples (the database tiles of the GEMM stay aligned)
            int64_t endc = st_ == S - 1 ? nchunks : std::min<int64_t>(nchunks, std::max<int64_t>(done_rows / U + 1, (int64_t)llround((double)n0 * pow(r, st_ + 1))));
            const int64_t end = std::min<int64_t>(N, endc * U);
            unsigned long long* cc = h->w_candcnt.as<unsigned long long>() + (deferred ? cc_stride * (size_t)st_ : 0);
            // ONE GEMM launch over the stage's rows whose epilogue keeps only keys beating the running K'-th key
            if (!deferred) HIPCHECK(hipMemsetAsync(cc, 0, cc_stride * 8, h->st));
            launch_flat_gemm_filter(h->w_q16.as<__half>(), (int)P.nq_pad, (int)nq, h->data.p, h->storage_f16, done_rows,
                                    end - done_rows, ld, bias, state + (KP - 1), KP, h->w_cand.as<uint64_t>(), cc, cap, h->st);
            tm.mark("scan");
            bool filtered_ok = true;
            if (!deferred) {
                HIPCHECK(hipMemcpyAsync(cnts.data(), cc, cc_stride * 8, hipMemcpyDeviceToHost, h->st));
                HIPCHECK(hipStreamSynchronize(h->st));
                for (int64_t qi = 0; qi < nq; qi++) if (cnts[(size_t)qi * CCS] > (unsigned long long)cap) { filtered_ok = false; break; }
            }
            if (filtered_ok) {
                merge_key_rows(h, h->w_cand.p, cc, cap, nq, state, state, KP, P.BUF);
                tm.mark("select");
            } else {
                h->timing["flat_filter_overflows"] += 1;   // adversarial order: redo this stage's rows chunk by chunk
                for (int64_t v0 = done_rows; v0 < end; v0 += CH) chunk_pass(v0, end);
                tm.mark("scan");
            }
            done_rows = end;
            stages_run = st_ + 1;
        }
        if (deferred) { fa.cand_cnt = h->w_candcnt.as<unsigned long long>(); fa.cand_cap = cap; fa.cand_cnt_n = stages_run; fa.cand_cnt_stride = (int64_t)cc_stride; }
    }
    if (done_rows < N) {       // flat_filter = 0 (or a filtered search)
        for (int64_t v0 = done_rows; v0 < N; v0 += CH) chunk_pass(v0, N);
        tm.mark("scan");
    }
}
static void flat_scan(rsx_index* h, const BatchPlan& P, FinalizeArgs& fa, StageTimer& tm) {
    // ranking score = <q,x> - |x|^2/2 ; bias buffer holds -|x|^2/2 (derived from norms)
    if (h->metric == RSX_METRIC_L2) h->w_misc.ensure((size_t)h->ntotal * 4);
    const float* bias = h->metric == RSX_METRIC_L2 ? h->w_misc.as<float>() : nullptr;
    if (h->ntotal == 0) launch_fill_u64(h->w_state.as<uint64_t>(), P.nq * P.KP, 0, h->st);
    else if (!P.allow_fast || P.nq <= 32) flat_score_rows(h, P, bias, tm);
    else flat_staged(h, P, bias, fa, tm);
}
// coarse quantiser + the top-nprobe lists of every query: w_probelist, w_dis0, w_segstart (the fast form also writes the per-query
// flags behind w_uncertain's certificate words that rerun_uncertified merges)
static void coarse_quantiser(rsx_index* h, const BatchPlan& P, const void* dq, int dtype, StageTimer& tm) {
    const int64_t nq = P.nq; const int d = h->d, ld = h->ld, nlist = h->nlist, nprobe = P.nprobe;
    if (P.coarse_fast) {
        const int nlp = (int)round_up(nlist, 4);   // row stride of the coarse scores: 16-byte aligned rows for k_select
        h->w_probelist.ensure((size_t)nq * nprobe * 4); h->w_dis0.ensure((size_t)nq * nprobe * 4); h->w_segstart.ensure((size_t)nq * (nprobe + 1) * 8);
        const int64_t nqp = h->kind == KIND_IVFPQ ? round_up(nq, 128) : P.nq_pad;
        const int64_t nl128 = round_up(nlist, 128);
        if (h->cent16_gen != h->cent_gen || !h->cent16.p) {       // the centroids' fp16 copy, once per centroid set
            h->cent16.ensure((size_t)nl128 * ld * 2);
            launch_convert_to_f16(h->d_centroids.p, 0, nlist, d, h->cent16.as<__half>(), ld, nl128, nullptr, h->st);
            h->cent16_gen = h->cent_gen;
        }
        h->w_coarse.ensure((size_t)nqp * nlp * 4);
        if (P.q16_direct) launch_coarse_approx((const __half*)dq, nqp, h->cent16.as<__half>(), nlist, ld, h->w_coarse.as<float>(), nlp, h->st, h->w_q32.as<float>(), nq * (int64_t)ld);
        else launch_coarse_approx(h->w_q16.as<__half>(), nqp, h->cent16.as<__half>(), nlist, ld, h->w_coarse.as<float>(), nlp, h->st);
        tm.mark("coarse");
        h->w_uncertain.ensure((size_t)nq * 8);
        CoarsePickArgs cp{};
        cp.approx = h->w_coarse.as<float>(); cp.nlp = nlp; cp.nlist = nlist; cp.Q32 = h->w_q32.as<float>(); cp.ld = ld; cp.d = d;
        cp.C = h->d_centroids.as<float>(); cp.cmax = cent_cmax(h);
        cp.ef = (dtype == RSX_F16 ? 1.0f : 2.0f) * 4.8828125e-4f;        // centroids rounded to fp16; fp32 queries as well
        cp.nprobe = nprobe; cp.list_len = h->d_len.as<int64_t>(); cp.pad_to = P.pad_to;
        cp.probe_list = h->w_probelist.as<int32_t>(); cp.dis0 = h->w_dis0.as<float>(); cp.seg_start = h->w_segstart.as<int64_t>();
        cp.bad = h->w_uncertain.as<int32_t>() + nq;
        if (P.lut_pass0_early) {      // pass 0 of the table build needs the queries only: extra workgroups of this launch
            h->w_lutws.ensure(pq_lut8_tiled_ws(nq, h->Mpad));
            cp.lp0 = LutPass0Args{h->w_q32.as<float>(), ld, h->d_codebooks.as<float>(), h->M, h->Mpad, nq, reinterpret_cast<float*>(h->w_lutws.p),
                                  pq_lut_pass0_blocks(nq, h->Mpad)};
        }
        launch_coarse_pick(cp, nq, h->st);
    } else { coarse_exact_scores(h, nq); tm.mark("coarse"); coarse_exact_probes(h, nq, nprobe, P.pad_to); }
    tm.mark("select_probe");
}
// profile >= 2: the vectors this batch scans
static void count_scanned(rsx_index* h, const BatchPlan& P, StageTimer& tm) {
    const int nlist = h->nlist;
    std::vector<int32_t> pl((size_t)P.nq * P.nprobe);
    HIPCHECK(hipMemcpyAsync(pl.data(), h->w_probelist.p, pl.size() * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHECK(hipStreamSynchronize(h->st));
    double tot = 0;
    std::vector<int32_t> pc((size_t)nlist, 0);
    for (int32_t l : pl) if (l >= 0) { tot += (double)h->h_len[(size_t)l]; pc[(size_t)l]++; }
    h->timing["scanned_vectors"] += tot;
    // the same batch seen list-major: vectors of every list probed at least once (what HBM must deliver), and vectors x
    // groups of 4 probing queries (what the IVF-PQ fast scan gathers)
    // (queries per table gather of the scan this index takes: 8 for the sliced layout and the M = 64 eight-query form, 16 at M = 16, else 4)
    const int gq = 4 * P.ngq;
    double uniq = 0, grp = 0;
    for (int l = 0; l < nlist; l++)
        if (pc[(size_t)l]) { uniq += (double)h->h_len[(size_t)l]; grp += (double)h->h_len[(size_t)l] * ((pc[(size_t)l] + gq - 1) / gq); }
    h->timing["scanned_unique_vectors"] += uniq; h->timing["scanned_group_vectors"] += grp; h->timing["scan_group_queries"] = (double)gq;
    tm.mark("count");
}
// work-item records + run descriptors + survivor logs of the rotated-layout scan (items work items of ngq records); log_cap: keys per log
static void* rot_scan_ws(rsx_index* h, int k, int64_t items, int ngq, int& log_cap) {
    // the log pool = (persistent workgroups x 64 logs x log_cap keys): 1 / 2 / 4 GiB by k, never more than a quarter of the
    // temp budget.  A log that fills up only sends the queries of its later runs to the exact re-run (counted); the pool is
    // touched where survivors land, so its size costs nothing per batch; reported by rsx_get "workspace_bytes"
    const int nwg = pq_scan_rot_max_wgs(h->M) * ngq;
    int64_t pool = (int64_t)(k <= 64 ? 1 : k <= 512 ? 2 : 4) << 30;
    pool = std::min(pool, std::max<int64_t>(h->temp_budget / 4, (int64_t)64 << 20));
    int64_t cap = pool / 8 / ((int64_t)nwg * 64);
    cap = std::max<int64_t>(64, cap / 16 * 16);
    if (h->pq_log_cap > 0) cap = h->pq_log_cap;            // tests starve the logs to force the overflow path
    log_cap = (int)std::min<int64_t>(cap, (int64_t)1 << 24);
    h->w_itemdesc.ensure(pq_scan_rot_ws(items * ngq, log_cap, nwg));
    return h->w_itemdesc.p;
}
// the 8-bit tables + per-query parameters; pg: the (query, probe) pairs grouped by list in the same launch (matrix-core form only)
static void build_pq_tables(rsx_index* h, const BatchPlan& P, void* lut_ws, const PairGroupArgs* pg, StageTimer& tm) {
    PQLutArgs la = pq_lut_args(h, P, lut_ws);
    la.probe_dis0 = h->w_dis0.as<float>(); la.nprobe = P.nprobe;
    la.pass0_done = P.lut_pass0_early; la.pg = pg;
    launch_pq_lut8(la, h->st);
    tm.mark("lut8");
}
// the fast scan's tiles and its threshold pre-pass: vectors per lane (vpl, tile_rows = 1024 vpl), the pre-pass sample and its form
struct PqGeometry { int vpl, tile_rows, pre_vpl, pre_rows; bool fused_pre, pre4; };
// the four-query pre-pass anchors its threshold on exact scores (k_pq_prepass4): inner-product IVF-PQ searches; IndexPQ's
// staged thresholds keep a_k - 2 eps (its L2 form has negated tables, and its stages tighten the threshold themselves)
static bool pq_anchor_applies(const rsx_index* h, const BatchPlan& P) {
    return h->pq_tau_anchor != 0 && !P.staged && h->metric == RSX_METRIC_INNER_PRODUCT && h->M == h->Mpad;
}
static PqGeometry pq_geometry(const rsx_index* h, const BatchPlan& P, bool filtered) {
    const int nlist = h->nlist, k = P.k; const int64_t pairs = P.nq * P.nprobe;
    PqGeometry g{};
    int64_t avg_slabs = std::max<int64_t>(1, (h->ntotal / std::max(1, nlist) + 63) / 64);
    // rotated layout: persistent workgroups draw items dynamically, so the tile is the whole (average) list — one table
    // staging per (list, query group) — as long as that leaves a few thousand items to balance over 256 CUs
    int vpl = 8;
    if (P.rot) { vpl = 32; while (vpl > 8 && 16 * (vpl / 2) >= avg_slabs) vpl /= 2; }
    if (h->scan_chunk > 0) vpl = std::max(1, std::min(P.rot ? 64 : 16, h->scan_chunk / 1024));
    else {
        // enough items to balance the chip: a few thousand for a full batch; for a handful of queries every (query, list)
        // pair is its own group and each item stages a whole table, so one item per CU is the better trade
        const int64_t groups_est = pairs <= nlist / 4 ? pairs : pairs / 4 + 1;
        const int64_t want_items = pairs <= nlist / 4 ? 256 : 2048;
        while (vpl > 1 && groups_est * ((avg_slabs + 16 * vpl - 1) / (16 * vpl)) < want_items) vpl /= 2;
    }
    if (vpl != 64 && vpl != 32 && vpl != 16 && vpl != 8 && vpl != 4 && vpl != 2) vpl = 1;
    g.vpl = vpl; g.tile_rows = 64 * 16 * vpl;
    // the pre-pass only has to produce a threshold: it scores a (smaller) prefix of the closest list
    g.pre_vpl = vpl;
    if (filtered && h->pq_pre_rows > 0) {
        while (g.pre_vpl > 1 && 64 * 16 * g.pre_vpl > h->pq_pre_rows) g.pre_vpl /= 2;
        while (g.pre_vpl > 1 && 64 * 16 * g.pre_vpl < P.KP * 4) g.pre_vpl *= 2;   // ... but well above K' candidates
        if (g.pre_vpl > vpl) g.pre_vpl = vpl;
    }
    g.pre_rows = filtered ? 64 * 16 * g.pre_vpl : g.tile_rows;
    // one-launch pre-pass (k_pq_prepass: score a prefix of the closest list with byte gathers on the query's own table,
    // 16-bit integer sums in LDS, k-th largest by a radix walk -> threshold a_k - 2 eps) when its LDS footprint allows;
    // else grouping + scan of the prefix + selection (K'-th key of the prefix as the threshold)
    g.fused_pre = filtered && h->pq_prepass_fused != 0;
    if (g.fused_pre) {
        // the sample's k-th best score is the threshold: the sample must be a large part of the closest list once k is large
        // (measured at 24k-vector lists: a 2048-vector prefix gives ~1000 candidates per query for k = 10 but ~20000 for
        // k = 100) — 160 k vectors, at least pq_pre_rows, at most 32768 (64 KiB of 16-bit sums in LDS)
        // (round 3, measured on the bench index at k = 10: 2048 / 4096 / 8192 / 16384 sample rows leave 1046 / 633 / 372 / 217
        // candidates per query; the pre-pass costs 85 / 131 / 239 / 446 us and the scan 2.50 / 2.41 / 2.43 / 2.42 ms: 4096 is
        // the best total for a full batch, a few queries keep the cheaper 2048)
        int64_t base_rows = h->pq_pre_rows > 0 ? h->pq_pre_rows : 2048;
        if (P.nq <= 64) base_rows = std::min<int64_t>(base_rows, 2048);
        int64_t want_rows = std::max<int64_t>(base_rows, std::min<int64_t>(h->pq_pre_max, (int64_t)h->pq_pre_mult * k));
        want_rows = std::min<int64_t>(round_up(want_rows, 64), round_up(std::max<int64_t>(P.maxlen, 64), 64));
        // small k, full batch, rotated layout: the 4-queries-per-workgroup form (k_pq_prepass4) — its sample is what fits the LDS
        // beside the four-query table image (3520 rows at M = 96)
        // (k <= 25 at the default pq_pre_rows; an explicit smaller pq_pre_rows shrinks the sample, not the range of k)
        g.pre4 = P.rot && h->pq_prepass4 != 0 && P.nq >= 64 && (int64_t)160 * k <= std::max<int64_t>(base_rows, 4096) && pq_prepass4_max_rows(h->Mpad) >= 1024;
        // (with the exact anchor, pq_tau_anchor, the sample stays what it was: 2048 anchored rows measured the same ms per batch on the
        // headline as 3520, but on the informative mixture they let more keys through than the parent rule's 3520 — profiles/tau_anchor.md)
        if (g.pre4) want_rows = std::min<int64_t>(want_rows, pq_prepass4_max_rows(h->Mpad));
        g.pre_rows = (int)want_rows;
        g.fused_pre = (size_t)g.pre_rows * 2 + (size_t)h->Mpad * 256 + 2048 <= 150 * 1024;
        if (!g.fused_pre) g.pre_rows = 64 * 16 * g.pre_vpl;
    }
    return g;
}
// the one-launch threshold pre-pass behind the table build (and the pair grouping where it rides along); the two-call search parks
// behind it.  Returns whether the pairs are grouped already
// (staged flat scan: no pairs to group, no emission — its stages scan every tile — and no parking: the thresholds keep moving)
static bool pq_prepass(rsx_index* h, const BatchPlan& P, BatchResult& R, const PairArea& pr, const PqGeometry& g, void* lut_ws, StageTimer& tm) {
    const int64_t nq = P.nq; const int nlist = h->nlist;
    R.cand_cap = alloc_cand_rows(h, P, h->M);
    PQPrepassArgs pa{};
    pa.codes = h->data.as<uint8_t>(); pa.list_base = h->d_base.as<int64_t>(); pa.list_len = h->d_len.as<int64_t>();
    pa.probe_list = h->w_probelist.as<int32_t>(); pa.probe_dis0 = h->w_dis0.as<float>(); pa.seg_start = h->w_segstart.as<int64_t>();
    pa.lut8 = h->w_lut8.as<uint8_t>(); pa.qparam = h->w_qparam.as<float>();
    pa.nprobe = P.nprobe; pa.Mpad = h->Mpad; pa.pre_rows = g.pre_rows; pa.KP = P.KP; pa.CB = h->CB; pa.k = P.k;
    pa.state = h->w_state.as<uint64_t>(); pa.cand_cnt = h->w_candcnt.as<unsigned long long>();
    h->w_tau.ensure((size_t)nq * 8); pa.tau = h->w_tau.as<uint64_t>();
    if (pq_anchor_applies(h, P)) { pa.codebooks = h->d_codebooks.as<float>(); pa.dsub = h->dsub; pa.Q32 = h->w_q32.as<float>(); pa.ldq = h->ld; }
    if (P.rot && !P.staged) {       // the sample's own candidates leave from the pre-pass; the scan drops that (query, list, tile 0)
        h->w_excl.ensure((size_t)nq * 2);
        pa.cand = h->w_cand.as<uint64_t>(); pa.cand_cap = R.cand_cap; pa.tile_rows = g.tile_rows; pa.excl = h->w_excl.as<uint16_t>();
    }
    const bool group_in_tables = !P.staged && lut_ws && h->pq_group_fused != 0 && pr.npairs <= PG_MAX_PAIRS &&
                                 nlist <= PG_BLOCKS * PG_MAX_LPB;
    PairGroupArgs pg{};
    bool grouped = false;
    if (group_in_tables) {      // the pairs grouped by list by extra workgroups of the table launch
        if (!h->w_pgflags.p) { h->w_pgflags.ensure((size_t)PG_BLOCKS * 16); HIPCHECK(hipMemsetAsync(h->w_pgflags.p, 0, (size_t)PG_BLOCKS * 16, h->st)); }
        pg = pr.args(4 * P.ngq, g.tile_rows, 0);
        pg.flags = h->w_pgflags.as<uint32_t>(); pg.nb = PG_BLOCKS;
        if (++h->pg_epoch == 0) h->pg_epoch = 1;
        pg.epoch = h->pg_epoch;
        grouped = true;
    }
    build_pq_tables(h, P, lut_ws, group_in_tables ? &pg : nullptr, tm);
    // large k: the histogram form of the four-query pre-pass (any sample size, several lists; pq_prepass4 = 2 keeps k_pq_prepass)
    const bool pre4big = P.rot && !g.pre4 && h->pq_prepass4 == 1 && nq >= 64 && h->Mpad >= 32 && g.pre_rows <= 32768;
    if (g.pre4 && launch_pq_prepass4(pa, nq, h->st) == 0) {
        if (h->profile >= 2) { h->timing["pq_prepass4_batches"] += 1; h->timing["pq_anchored_batches"] += pa.codebooks ? 1 : 0; h->timing["pq_pre_rows_used"] = (double)g.pre_rows; }
    } else if (!(pre4big && launch_pq_prepass4_big(pa, nq, h->st) == 0))
        launch_pq_prepass(pa, nq, h->st);
    R.fused_pre_used = true;
    if (!P.staged && h->tc && h->tc->active && P.allow_fast && std::this_thread::get_id() == h->tc->worker) {
        // two-call search: the thresholds are final on the device; hand them to the caller and wait for rsx_search_scan
        HIPCHECK(hipStreamSynchronize(h->st));
        rsx_index::TwoCall& t = *h->tc; std::unique_lock<std::mutex> lk(t.mu);
        t.tau = h->w_tau.as<uint64_t>(); t.ntau = nq; t.parked = true;
        t.cv.notify_all();
        t.cv.wait(lk, [&] { return t.go; });
        t.parked = false; t.tau = nullptr; t.ntau = 0;
    }
    return grouped;
}
// What every list-major scan takes: the per-pair arguments, the grouping and the bound of its work items (the kernels' grid).  A bound that
// is not in (0, 0x7fffff00] becomes 0, which every scan launcher refuses (-1): it never wraps into the 32-bit field.
template <typename Args>
static void scan_common(Args& A, const PQScanArgs& b, const PairView& v, int64_t max_items) {
    A.b = b;
    A.pairs_sorted = v.pairs_sorted; A.pair_off = v.pair_off; A.group_off = v.group_off; A.total_groups = v.total_groups;
    A.item_off = v.item_off; A.total_items = v.total_items; A.nlist = v.nlist;
    A.max_items = (max_items <= 0 || max_items > 0x7fffff00) ? 0 : (int)max_items;
}
// ... and the batch's 8-bit tables for the fast scans; a call site adds its own: threshold and candidate rows, prune, pace, excl, qitems, the tile set
static PQScan8Args scan8_args(rsx_index* h, const PQScanArgs& b, const PairView& v, int64_t max_items) {
    PQScan8Args A{};
    scan_common(A, b, v, max_items);
    A.lut8 = h->w_lut8.as<uint8_t>(); A.qp = h->w_qparam.as<PQQParam>();
    return A;
}
// how a work-item scan of the block layouts is launched: its tile (1024 vpl rows), rot_scan_ws' workspace, the plan's eight-query choice
static PQRotLaunch rot_launch(const rsx_index* h, const BatchPlan& P, int vpl, void* ws, int log_cap) {
    return PQRotLaunch{vpl, ws, log_cap, P.sliced ? (P.sl_eight ? 1 : 0) : h->pq_q8};
}
// the main filtered scan: every (query, probe) pair, only the keys above the query's threshold reach its candidate row
static bool pq_filtered_scan(rsx_index* h, const BatchPlan& P, BatchResult& R, PQScanArgs& a, const PairArea& pr, const PqGeometry& g,
                             bool grouped, StageTimer& tm) {
    const int64_t nq = P.nq; const int nprobe = P.nprobe, KP = P.KP;
    uint64_t* state = h->w_state.as<uint64_t>();
    tm.mark("scan0");
    if (!g.fused_pre) {
        R.cand_cap = alloc_cand_rows(h, P, h->M);
        // multi-launch form: top-K' of the scored prefix of the closest list, row prefix
        // [0, min(seg_start[q][1], pre_rows)), written as the threshold key + counter reset
        select_rows(h, h->w_temp.as<float>(), P.tmax, h->w_segstart.as<int64_t>() + 1, nprobe + 1,
                    std::min<int64_t>(P.maxlen, g.pre_rows), 0, nq, KP, P.BUF, KP, state, false,
                    h->w_candcnt.as<unsigned long long>());
        // The pre-pass is only a threshold: keep its K'-th key and let the main scan score EVERYTHING (the
        // prefix included), so the scan kernel carries no per-slab "already scored" test and no key can
        // arrive twice (the prefix keys above the threshold come back through the candidate buffer).
        // (the selection wrote only the K'-th key of each query and reset the query's candidate counter)
        // (a stage mark is an event record: ~5 us of stream time in profile mode — none for a stage that launched nothing)
        tm.mark("select0");
    }
    if (!grouped) { pr.group(4 * P.ngq, g.tile_rows, nprobe, 0, h->st); tm.mark("group"); }
    const int64_t mi = max_scan_items(h, nq, nprobe, 4 * P.ngq, g.tile_rows);
    int log_cap = 64;
    void* rws = P.rot ? rot_scan_ws(h, P.k, mi, P.ngq, log_cap) : nullptr;
    // threshold keys: one per query from the one-launch pre-pass, else the K'-th key the selection left in the state rows
    const uint64_t* tau_ptr = g.fused_pre ? h->w_tau.as<uint64_t>() : state + (KP - 1);
    const int64_t tau_stride = g.fused_pre ? 1 : KP;
    // candidate gather + selection in one launch when the (probe rank, tile) table of a query is small (rsx_internal.h)
    const int gs_tmax = (int)((P.maxlen + g.tile_rows - 1) / g.tile_rows);
    R.use_gather = P.rot && h->pq_gather != 0 && pq_gather_select_applies(nprobe, gs_tmax, KP);
    if (P.rot && h->pq_gather != 0 && !R.use_gather) h->timing["pq_gather_declined"] += 1;
    if (R.use_gather) {
        h->w_qitems.ensure((size_t)nq * nprobe * gs_tmax * 4);
        PQGatherArgs& gs = R.gs;
        gs.probe_list = h->w_probelist.as<int32_t>(); gs.list_len = h->d_len.as<int64_t>(); gs.nprobe = nprobe;
        gs.tile_rows = g.tile_rows; gs.tmax = gs_tmax; gs.qitems = h->w_qitems.as<int32_t>();
        gs.seg_desc = pq_scan_rot_ws_desc(rws, mi * P.ngq); gs.log_keys = pq_scan_rot_ws_keys(rws, mi * P.ngq);
        gs.cand = h->w_cand.as<uint64_t>(); gs.cand_cnt = h->w_candcnt.as<unsigned long long>(); gs.cand_cap = R.cand_cap;
        gs.state = state; gs.KP = KP;
    }
    tm.pre_scan();
    PQScan8Args A = scan8_args(h, a, pr.view(), mi);
    A.tau_key = tau_ptr; A.tau_stride = tau_stride;
    A.cand = h->w_cand.as<uint64_t>(); A.cand_cnt = h->w_candcnt.as<unsigned long long>(); A.cand_cap = R.cand_cap;
    if (!P.rot) return launch_pq_scan8(A, g.vpl, h->st) == 0;
    A.prune = h->pq_prune; A.pace = h->pq_pace & 0xffff;
    if (g.fused_pre) A.excl = h->w_excl.as<uint16_t>();
    if (R.use_gather) A.qitems = h->w_qitems.as<int32_t>();
    A.qitems_tmax = gs_tmax;
    return launch_pq_scan_rot(A, rot_launch(h, P, g.vpl, rws, log_cap), h->st) == 0;
}
// IndexPQ (faiss.IndexPQ: one list, every query scans every code): the staged filtered scan.  The filtered IVF-PQ scan takes ONE threshold
// from a sample of its closest list; over N rows in exchangeable order a threshold from R0 rows lets ~N k / R0 rows through — 49 000 per
// query at N = 10M, k = 10, R0 = 2048, three candidate rows' worth.  Here the threshold tightens while the scan runs, as the staged Flat
// GEMM's does (flat_staged): stage s scans a SET of the list's tiles with tau_s (work items of that set only: k_pq_rot_items' tile-set
// form, the work-item scans unchanged), k_pq_stage_gather moves the survivors into the candidate rows, derives tau_(s+1) = max(tau_s,
// a_k - 2 eps) from the row's k-th best approximate key and compacts the row to it.  Stage sizes grow geometrically (each stage
// `growth` times the rows scanned before it: ~k growth new rows per query and stage beside the 2 eps band), and the tiles of a stage
// are spread over the whole list (tile number j -> (j mul) mod T, mul ~ 0.618 T coprime to T), so a corpus added source by source or in
// sorted order meets every stage with a sample of all of it.  After the last stage the row holds every vector whose approximate score
// reaches the final tau — the invariant k_pq_final_tab / k_finalize and the second chance rely on; an overflowed row or log flags its
// query alone for the exact re-run.  Beside the codes nothing grows with N: candidate rows (cand_row_cap), survivor logs, one stage's items.
static void pq_staged_scan(rsx_index* h, const BatchPlan& P, BatchResult& R, PQScanArgs& a, PqGeometry g, void* lut_ws, StageTimer& tm) {
    const int64_t nq = P.nq, N = h->h_len[0];
    // tiles: at least 64 of them where the index allows it (the stages need something to grow over), never more rows than the work-item scans' largest tile
    int vpl = h->scan_chunk > 0 ? g.vpl : 32;
    if (h->scan_chunk <= 0) while (vpl > 1 && (N + 1024 * vpl - 1) / (1024 * vpl) < 64) vpl /= 2;
    g.vpl = vpl; g.tile_rows = 1024 * vpl;
    const int T = (int)std::max<int64_t>(1, (N + g.tile_rows - 1) / g.tile_rows);
    const PairArea none(h, 0, 1, 1);
    pq_prepass(h, P, R, none, g, lut_ws, tm);
    tm.mark("scan0");
    // the stage boundaries, in tiles
    const double growth = (h->pq_flat_growth > 0 ? h->pq_flat_growth : 300) / 100.0;
    const int max_stages = h->pq_flat_max_stages > 0 ? h->pq_flat_max_stages : 12;
    const int64_t first_rows = h->pq_flat_first > 0 ? h->pq_flat_first : std::max<int64_t>(65536, (int64_t)4 * g.pre_rows);
    const int c0 = (int)std::min<int64_t>(T, std::max<int64_t>(1, (first_rows + g.tile_rows - 1) / g.tile_rows));
    double ratio = 1.0 + growth;
    if (T > c0 && max_stages > 1 && std::log((double)T / c0) / std::log(ratio) > max_stages - 1) ratio = std::pow((double)T / c0, 1.0 / (max_stages - 1));
    std::vector<int> ends;      // ends[s]: tiles scanned once stage s is done; a stage never holds more tiles than the gather's LDS describes
    {
        double c = c0;
        for (int prev = 0; prev < T;) {
            const int want = max_stages == 1 ? T : (int)std::min<double>(T, std::ceil(c));
            const int e = std::min(std::max(want, prev + 1), prev + PQ_STAGE_MAX_TILES);
            ends.push_back(e); prev = e;
            if (e >= want) c *= ratio;
        }
    }
    const int S = (int)ends.size();
    int tmax = 0;
    for (int s_ = 0; s_ < S; s_++) tmax = std::max(tmax, ends[(size_t)s_] - (s_ ? ends[(size_t)s_ - 1] : 0));
    int mul = (int)std::llround(0.6180339887 * T);
    if (mul < 1) mul = 1;
    auto gcd = [](int x, int y) { while (y) { const int t = x % y; x = y; y = t; } return x; };
    while (gcd(mul, T) != 1) mul++;
    // the work items of a stage: every group of G queries x the stage's tiles.  One list, so the pair grouping is known on the host: the pairs
    // in query order, one entry of pair_off / group_off, and per stage item_off = {0, groups x tiles}
    const int G = 4 * P.ngq, ng = (int)((nq + G - 1) / G);
    std::vector<int32_t>& hd = h->stage_host;
    hd.assign((size_t)nq + 8 + (size_t)4 * S, 0);
    for (int64_t i = 0; i < nq; i++) hd[(size_t)i] = (int32_t)i;
    hd[(size_t)nq + 1] = (int32_t)nq; hd[(size_t)nq + 3] = ng; hd[(size_t)nq + 4] = ng;
    for (int s_ = 0; s_ < S; s_++) {
        const int nt = ends[(size_t)s_] - (s_ ? ends[(size_t)s_ - 1] : 0);
        hd[(size_t)nq + 8 + (size_t)4 * s_ + 1] = ng * nt; hd[(size_t)nq + 8 + (size_t)4 * s_ + 2] = ng * nt;
    }
    h->w_stagedir.ensure(hd.size() * 4);
    HIPCHECK(hipMemcpyAsync(h->w_stagedir.p, hd.data(), hd.size() * 4, hipMemcpyHostToDevice, h->st));
    const int32_t* sd = h->w_stagedir.as<int32_t>();
    const int64_t mi = (int64_t)ng * tmax + 8;
    int log_cap = 64;
    void* rws = rot_scan_ws(h, P.k, mi, P.ngq, log_cap);
    h->w_qitems.ensure((size_t)nq * tmax * 4);
    PQStageArgs ga{};
    ga.qitems = h->w_qitems.as<int32_t>(); ga.tmax = tmax;
    ga.seg_desc = pq_scan_rot_ws_desc(rws, mi * P.ngq); ga.log_keys = pq_scan_rot_ws_keys(rws, mi * P.ngq);
    ga.cand = h->w_cand.as<uint64_t>(); ga.cand_cnt = h->w_candcnt.as<unsigned long long>(); ga.cand_cap = R.cand_cap;
    ga.qparam = h->w_qparam.as<float>(); ga.k = P.k; ga.tau = h->w_tau.as<uint64_t>();
    // the one list's grouping in the staged directory; item_off / total_items and the first tile number: per stage
    PQScan8Args A = scan8_args(h, a, PairView{sd, sd + nq, sd + nq + 2, sd + nq + 4, nullptr, nullptr, 1}, mi);
    A.tau_key = h->w_tau.as<uint64_t>(); A.tau_stride = 1;
    A.cand = h->w_cand.as<uint64_t>(); A.cand_cnt = h->w_candcnt.as<unsigned long long>(); A.cand_cap = R.cand_cap;
    A.pace = h->pq_pace & 0xffff;
    A.qitems = h->w_qitems.as<int32_t>(); A.qitems_tmax = tmax;
    A.tile_mul = mul; A.tile_mod = T;
    for (int s_ = 0; s_ < S; s_++) {
        const int j0 = s_ ? ends[(size_t)s_ - 1] : 0, nt = ends[(size_t)s_] - j0;
        A.item_off = sd + nq + 8 + 4 * s_; A.total_items = A.item_off + 2; A.tile_j0 = j0;
        if (s_ == S - 1) tm.pre_scan();
        if (launch_pq_scan_rot(A, rot_launch(h, P, g.vpl, rws, log_cap), h->st) != 0)
            RSX_THROW(RSX_ERR_UNSUPPORTED, "IndexPQ staged scan: no kernel for M=%d at a batch of %lld queries (the sliced 8-query scan takes at most 4 GiB of 8-bit tables per batch)", h->M, (long long)P.nq);
        tm.mark("scan");
        ga.ntiles = nt; ga.nrecs = (int64_t)ng * nt * P.ngq; ga.last = s_ == S - 1;
        launch_pq_stage_gather(ga, nq, h->st);
        tm.mark("select");
    }
    h->timing["pq_flat_stages"] += (double)S;
    R.filtered = true;
}
// 8-bit tables, 4 queries per LDS read; approximate scores, certified in k_finalize
static void pq_fast_scan(rsx_index* h, const BatchPlan& P, BatchResult& R, PQScanArgs& a, StageTimer& tm) {
    const int64_t nq = P.nq; const int nlist = h->nlist, nprobe = P.nprobe;
    h->w_lut8.ensure((size_t)nq * h->Mpad * 256); h->w_qparam.ensure((size_t)nq * 16); h->w_uncertain.ensure((size_t)nq * 8);
    void* lut_ws = nullptr;
    if (P.pq_fused_lut && h->dsub == 8 && h->lut_tiled != 0) { h->w_lutws.ensure(pq_lut8_tiled_ws(nq, h->Mpad)); lut_ws = h->w_lutws.p; }
    const PairArea pr(h, nq, nprobe, nlist);
    // Two stages, so that only a sliver of the scores ever leaves the scan kernel:
    //  stage 1: score ONLY the first tile of each query's closest list (probe rank 0) into the score
    //           buffer and take its top-K' -> state0; its K'-th key is a lower bound of the query's final
    //           K'-th best key;
    //  stage 2: scan everything else (all probes, all tiles, minus that piece) in the multi-query groups,
    //           appending to a small per-query candidate buffer only the keys that beat the bound
    //           (wave-aggregated atomics); a final select merges them with state0.
    // A full candidate buffer marks the query uncertain (-> exact fallback), so this is always exact.
    R.filtered = (nprobe > 1 || P.staged) && P.pq_filter != 0;
    const PqGeometry g = pq_geometry(h, P, R.filtered);
    bool done = true, grouped = false;
    if (P.staged) {
        if (!g.fused_pre) RSX_THROW(RSX_ERR_UNSUPPORTED, "IndexPQ staged scan: the threshold pre-pass does not fit (M=%d)", h->M);
        pq_staged_scan(h, P, R, a, g, lut_ws, tm);
    }
    else if (g.fused_pre) grouped = pq_prepass(h, P, R, pr, g, lut_ws, tm);
    else {
        build_pq_tables(h, P, lut_ws, nullptr, tm);
        h->w_temp.ensure((size_t)nq * P.tmax * 4);       // this form scores a prefix / everything into the score rows
        a.temp = h->w_temp.as<float>();
        pr.group(4, g.pre_rows, R.filtered ? 1 : nprobe, R.filtered ? 1 : 0, h->st);
        tm.mark("group");
        const int64_t mi = R.filtered ? (nq + nlist + 8) : max_scan_items(h, nq, nprobe, 4, g.tile_rows);
        int log_cap = 64;
        void* rws = P.rot ? rot_scan_ws(h, P.k, mi, 1, log_cap) : nullptr;
        const int vpl = R.filtered ? g.pre_vpl : g.vpl;
        const PQScan8Args A = scan8_args(h, a, pr.view(), mi);      // no threshold: every score goes to the score rows
        done = (P.rot ? launch_pq_scan_rot(A, rot_launch(h, P, vpl, rws, log_cap), h->st) : launch_pq_scan8(A, vpl, h->st)) == 0;
    }
    if (done && R.filtered && !P.staged) done = pq_filtered_scan(h, P, R, a, pr, g, grouped, tm);
    if (!done) RSX_THROW(RSX_ERR_UNSUPPORTED, "IVFPQ fast scan: no kernel for M=%d at a batch of %lld queries (the sliced 8-query scan takes at most 4 GiB of 8-bit tables per batch)", h->M, (long long)P.nq);
    // rotated layout, threshold by construction: finalize straight from the complete candidate row (k_pq_final_tab) when K'
    // is large or a table entry is a long chain (M = 16: dsub 48) — the K' cut, its certificate and the second chance disappear
    R.tab_fits = R.filtered && R.fused_pre_used && P.rot && h->pq_final_tab != 0 && pq_final_tab_capacity(h->M, h->CB, P.k) > 0;
    R.use_tab = R.tab_fits && (h->pq_final_tab == 2 || P.KP >= 512 || h->dsub > 8);
}
static void pq_exact_scan(rsx_index* h, const BatchPlan& P, PQScanArgs& a, StageTimer& tm) {
    const int64_t nq = P.nq, pairs = nq * P.nprobe; const int nlist = h->nlist;
    const bool pq_l2 = h->metric == RSX_METRIC_L2;      // per-(query, list) tables, built inside the scan (k_pq_scan_l2)
    if (h->scan_kernel != 1 && h->CB == 16 && !pq_l2) {
        // v2: list-major, two queries per LDS read
        int64_t avg_slabs = std::max<int64_t>(1, (h->ntotal / std::max(1, nlist) + 63) / 64);
        int vpl = 8;
        if (h->scan_chunk > 0) vpl = std::max(1, std::min(8, h->scan_chunk / 1024));
        else while (vpl > 1 && (pairs / 2 + 1) * ((avg_slabs + 16 * vpl - 1) / (16 * vpl)) < 2048) vpl /= 2;
        if (vpl != 8 && vpl != 4 && vpl != 2) vpl = 1;
        const int tile_rows = 64 * 16 * vpl;
        const PairArea pr(h, nq, P.nprobe, nlist);
        pr.group(2, tile_rows, P.nprobe, 0, h->st);
        tm.mark("group");
        PQScan2Args A{};
        scan_common(A, a, pr.view(), max_scan_items(h, nq, P.nprobe, 2, tile_rows));
        if (launch_pq_scan2(A, vpl, h->st) == 0) return;
    }
    const int64_t max_slabs = std::max<int64_t>(1, P.maxlen / 64); int64_t spc;
    if (h->scan_chunk > 0) spc = std::max<int64_t>(16, h->scan_chunk / 64);
    else {
        // enough work items to fill 256 CUs several times over, but no smaller than 32 slabs
        const int64_t want_items = 4096, chunks = std::max<int64_t>(1, (want_items + pairs - 1) / pairs);
        spc = std::max<int64_t>(32, (max_slabs + chunks - 1) / chunks);
    }
    a.slabs_per_chunk = (int)spc;
    a.max_chunks = (int)((max_slabs + spc - 1) / spc);
    if ((pq_l2 ? launch_pq_scan_l2(a, h->w_q32.as<float>(), h->ld, h->d_centroids.as<float>(), h->d_codebooks.as<float>(), h->d, h->dsub, h->st)
               : P.rot ? launch_pq_scan_rot_exact(a, h->st) : launch_pq_scan(a, h->st)) != 0)
        RSX_THROW(RSX_ERR_UNSUPPORTED, "IVFPQ scan: no kernel for M=%d", h->M);
}
static void pq_scan(rsx_index* h, const BatchPlan& P, BatchResult& R, StageTimer& tm) {
    // the exact kernels gather fp32 table entries; the fast path builds the table in LDS (when it fits)
    if (!P.pq_fused_lut && h->metric != RSX_METRIC_L2) {
        h->w_lut.ensure((size_t)P.nq * h->Mpad * 256 * 4);
        launch_pq_lut(h->w_q32.as<float>(), h->ld, P.nq, h->d, h->M, h->Mpad, h->d_codebooks.as<float>(), h->w_lut.as<float>(), h->st);
        tm.mark("lut");
    }
    PQScanArgs a{};
    a.codes = h->data.as<uint8_t>(); a.M = h->M; a.Mpad = h->Mpad; a.CB = h->CB;
    a.list_base = h->d_base.as<int64_t>(); a.list_len = h->d_len.as<int64_t>();
    a.lut = h->w_lut.as<float>(); a.probe_list = h->w_probelist.as<int32_t>(); a.probe_dis0 = h->w_dis0.as<float>();
    a.seg_start = h->w_segstart.as<int64_t>(); a.nq = P.nq; a.nprobe = P.nprobe;
    a.temp = h->w_temp.as<float>(); a.tstride = P.tmax;
    if (P.fast) pq_fast_scan(h, P, R, a, tm);
    else pq_exact_scan(h, P, a, tm);
    h->timing[P.allow_fast ? "scan_launches" : "fb_scan_launches"] += 1;
    tm.mark("scan");
}
// exact mode (see the Flat path): fp64 scores of every row of the probed lists into the score rows
static void ivf_flat_exact(rsx_index* h, const BatchPlan& P, StageTimer& tm) {
    ExactScoreArgs ea{};
    ea.kind = h->kind; ea.metric = h->metric; ea.nq = P.nq; ea.Q32 = h->w_q32.as<float>(); ea.ldq = h->ld; ea.d = h->d;
    ea.X = h->data.p; ea.x_f16 = h->storage_f16; ea.ld = h->ld; ea.temp = h->w_temp.as<float>(); ea.tstride = P.tmax;
    ea.probe_list = h->w_probelist.as<int32_t>(); ea.seg_start = h->w_segstart.as<int64_t>(); ea.nprobe = P.nprobe;
    ea.list_base = h->d_base.as<int64_t>(); ea.list_len = h->d_len.as<int64_t>();
    if (h->kind == KIND_IVFSQ) {      // the same fp64 scores against the decoded rows
        ea.X = nullptr;
        ea.sq = sq_rows(h);
        launch_sq_exact_scores(ea, h->st);
    } else
    launch_exact_scores(ea, h->st);
    tm.mark("scan");
}
// Same two-stage shape as the IVF-PQ fast path when the LDS-DMA kernel applies: score a prefix of every
// query's closest list, take its K'-th key as the query's threshold, then scan everything with the keys
// above it going to a small per-query candidate buffer instead of a full score row.  A full buffer
// (never seen at the bench sizes) falls back to the score-buffer path, so the result is always exact.
// Returns whether the batch was filtered; a holds the unfiltered scan's arguments again either way.
static bool ivf_flat_filtered(rsx_index* h, const BatchPlan& P, BatchResult& R, ListScanArgs& a, const PairArea& pr, int ls_qt, int item_rows,
                              int64_t pre_chunks, StageTimer& tm) {
    const int64_t nq = P.nq, tmax = P.tmax; const int nprobe = P.nprobe, KP = P.KP;
    uint64_t* state = h->w_state.as<uint64_t>();
    int64_t chunk_rows = a.chunk_rows;
    // ... of the closest list — of the EIGHT closest lists when K' is large: a query whose closest list holds fewer than K'
    // rows would get no threshold, keep every row of its 128 lists and overflow (the prefix of its score row then runs on
    // into the next lists' first rows)
    // (round 4: two lists, not eight — with 64 probing queries per list nearly every list is among some query's eight closest,
    //  and the 'sample' read 26 of the 31 GB: 3.4 + 0.8 ms of a 13.2 ms batch at nlist 2048 / nprobe 128 / k 1000; two lists
    //  leave 11.3 ms and as few candidates; ONE list overflows the queries whose closest list is short: profiles/r04_n_docs_1000.md)
    // ivf_pre_lists = 0 (default): the query's TWO closest lists.  ONE list is not enough even when it is long: at nlist 2048 /
    // nprobe 128 its K'-th key lets > 131072 keys of some queries through (the score-row pass follows: 27 instead of 11.7 ms); at
    // 100M / nprobe 32 it would do (28.7 against 29.8 ms) — two is the setting that is safe at both (profiles/r04_n_docs_1000.md).
    // (a per-query list count — two, and up to two more where the closest lists are short — cost 1-2 % on the bench configs and was
    //  removed in round 5: profiles/r04_n_docs_1000.md)
    const int pre_want = h->ivf_pre_lists > 0 ? h->ivf_pre_lists : 2;
    const int pre_lists = (KP >= 256 && (int64_t)pre_want * pre_chunks * chunk_rows <= tmax) ? std::min(pre_want, nprobe) : 1;
    a.max_chunks = (int)pre_chunks;                        // the first chunk(s) of ...
    a.qtiles = 1;                                          // (groups of 16 there: most lists are the closest of at most a few queries)
    const int64_t pre_stride = pre_lists > 1 ? pre_chunks * chunk_rows : 0;    // several lists: one slice of the sample buffer each
    if (pre_stride) {
        a.pre_stride = pre_stride; a.tstride = pre_lists * pre_stride;
        launch_fill_f32(h->w_temp.as<float>(), nq * a.tstride, -INFINITY, h->st);
    }
    pr.group(16, 0, pre_lists, 0, h->st);       // ... the closest list(s) only
    launch_list_scan(a, h->st);
    if (a.sq_codes) h->timing["ivfsq_scan_launches"] += 1;
    tm.mark("scan0");
    R.cand_cap = alloc_cand_rows(h, P, 0);
    // the pre-pass is only a threshold (see the IVF-PQ path): the K'-th key, candidate counters reset
    if (pre_stride) {
        select_rows(h, h->w_temp.as<float>(), a.tstride, nullptr, 0, a.tstride, 0,
                    nq, KP, P.BUF, KP, state, false, h->w_candcnt.as<unsigned long long>());
        a.pre_stride = 0; a.tstride = tmax;
    } else
        select_rows(h, h->w_temp.as<float>(), tmax, h->w_segstart.as<int64_t>() + 1, nprobe + 1,
                    std::min<int64_t>(P.maxlen, pre_chunks * chunk_rows), 0, nq, KP, P.BUF, KP, state, false,
                    h->w_candcnt.as<unsigned long long>());
    tm.mark("select0");
    pr.group(16 * ls_qt, item_rows, nprobe, 0, h->st);
    tm.mark("group");
    a.qtiles = ls_qt;
    if (ls_qt >= 4) { chunk_rows *= 2; a.chunk_rows = (int)chunk_rows; }      // 8 waves, 1024 rows per work item
    a.max_chunks = (int)std::max<int64_t>(1, (P.maxlen + chunk_rows - 1) / chunk_rows);
    if (item_rows == (int)chunk_rows) { a.item_off = pr.item_off; a.total_items = pr.total_items; a.max_items = (int)max_scan_items(h, nq, nprobe, 16 * ls_qt, item_rows); }
    a.tau_key = state + (KP - 1); a.tau_stride = KP;
    a.cand = h->w_cand.as<uint64_t>(); a.cand_cnt = h->w_candcnt.as<unsigned long long>(); a.cand_cap = R.cand_cap;
    launch_list_scan(a, h->st);
    if (a.sq_codes) h->timing["ivfsq_scan_launches"] += 1;
    tm.mark("scan");
    std::vector<unsigned long long> cnts((size_t)nq * CCS);
    HIPCHECK(hipMemcpyAsync(cnts.data(), h->w_candcnt.p, (size_t)nq * 8 * CCS, hipMemcpyDeviceToHost, h->st));
    HIPCHECK(hipStreamSynchronize(h->st));
    bool filtered = true;
    // A few overflowed rows (a query between clusters whose sample gave a weak threshold) no longer send the whole batch through the
    // unfiltered scan (10 -> 25 ms at nlist 2048 / nprobe 128 / k 1000 for ONE such query): with the certificate behind the search
    // k_finalize flags them (cand_cnt > cand_cap) and they alone join the exact re-run (~1.1 ms per query at that size with k_exact_scores_f16: up to nq / 128
    // of them are cheaper than the rescan); more overflows mean the threshold failed for this data, and the batch is rescanned
    int64_t n_over = 0;
    for (int64_t qi = 0; qi < nq; qi++) n_over += cnts[(size_t)qi * CCS] > (unsigned long long)R.cand_cap;
    if (n_over > 0 && !(P.certify && n_over <= (h->ivf_overflow_max > 0 ? (int64_t)h->ivf_overflow_max : std::max<int64_t>(2, nq / 128)))) filtered = false;
    if (filtered && n_over > 0) { R.flag_overflows = true; h->timing["ivf_filter_overflow_queries"] += (double)n_over; }
    a.tau_key = nullptr; a.cand = nullptr; a.cand_cnt = nullptr; a.cand_cap = 0;
    return filtered;
}
// group (query, probe) pairs by list, then list-major MFMA scan
static void ivf_flat_scan(rsx_index* h, const BatchPlan& P, BatchResult& R, StageTimer& tm) {
    const int64_t nq = P.nq, npairs = nq * P.nprobe; const int nlist = h->nlist, nprobe = P.nprobe, ld = h->ld;
    const PairArea pr(h, nq, nprobe, nlist);
    // probing queries per group of the LDS-DMA list scans (list_scan_qtiles; "scan_chunk" takes the batch to the older scan: groups of 16)
    int ls_qt = 1;
    if (h->scan_chunk <= 0 && list_scan2_chunk_rows(h->storage_f16, ld) > 0)
        ls_qt = list_scan_qtiles(h, npairs, list_scan3_applies(h->storage_f16, ld, h->metric == RSX_METRIC_L2) != 0);
    // (list, chunk, group) work items in list-major order for the LDS-DMA scan's XCD-aware 1-D grid (round 4): the groups of a
    // list chunk run on one XCD at the same moment and its rows cross HBM once — at nlist 2048 / nprobe 128 half of the lists
    // are probed by more than 64 queries, i.e. by two groups, which used to land on different XCDs (two fetches)
    const int ls2_rows = list_scan2_chunk_rows(h->storage_f16, ld);
    const bool ls_wide = ls_qt >= 4;     // the 8-wave forms: 1024 rows per work item
    const int item_rows = (h->scan_chunk <= 0 && ls2_rows > 0) ? (ls_wide ? 2 * ls2_rows : ls2_rows) : 0;
    pr.group(16 * ls_qt, item_rows, nprobe, 0, h->st);
    tm.mark("group");
    ListScanArgs a = list_scan_args(h, P.nq, P.tmax, pr);
    a.Q16 = h->w_q16.as<__half>(); a.X = h->data.p; a.x_f16 = h->storage_f16;
    int64_t chunk_rows = h->scan_chunk > 0 ? round_up(h->scan_chunk, 64) : 2048;
    int64_t want = 2048;  // work items
    while (chunk_rows > 256 && (int64_t)a.max_groups * ((P.maxlen + chunk_rows - 1) / chunk_rows) < want) chunk_rows /= 2;
    if (h->scan_chunk <= 0 && ls2_rows > 0) chunk_rows = ls2_rows;
    a.chunk_rows = (int)chunk_rows;
    a.qtiles = ls_qt;
    a.max_chunks = (int)std::max<int64_t>(1, (P.maxlen + chunk_rows - 1) / chunk_rows);
    // (ivf_filter: 1 = when the score rows would exceed ~2 GB — below that the second grouping pass and the
    //  count read-back cost more than the row traffic they save; 2 = always; 0 = never)
    // (round 4: for large k the pre-pass scores the first 4 K' rows of the closest list — up to 32 chunks — instead of giving up
    //  the filter when K' no longer fits one chunk: k = 1000 at nlist 2048 / nprobe 128 wrote and re-read 10 GB of score rows)
    const int64_t pre_chunks = std::max<int64_t>(1, ((int64_t)P.KP * std::max(1, h->ivf_pre_mult) + chunk_rows - 1) / chunk_rows);
    const bool want_filter = P.ivf_filter != 0 && nprobe > 1 && chunk_rows == ls2_rows &&
                             pre_chunks <= 32 && (P.ivf_filter > 1 || nq * P.tmax >= (int64_t)500000000);
    if (want_filter) R.filtered = ivf_flat_filtered(h, P, R, a, pr, ls_qt, item_rows, pre_chunks, tm);
    if (!R.filtered) {
        if (ls_wide && a.chunk_rows == ls2_rows) {     // 8 waves, 1024 rows per work item
            a.chunk_rows *= 2;
            a.max_chunks = (int)std::max<int64_t>(1, (P.maxlen + a.chunk_rows - 1) / a.chunk_rows);
        }
        if (!want_filter && item_rows > 0 && item_rows == a.chunk_rows) {     // (after a filtered attempt the grouping in place is the filtered scan's: same items)
            a.item_off = pr.item_off; a.total_items = pr.total_items; a.max_items = (int)max_scan_items(h, nq, nprobe, 16 * ls_qt, item_rows);
        }
        launch_list_scan(a, h->st);
        tm.mark("scan");
    }
}
// KIND_IVFSQ: the same stages over rows of code bytes (k_sq.hip).  The batch's query factors first (k_sq_query_factors), then ivf_flat_scan's
// grouping and, where the filter applies, ivf_flat_filtered's threshold pre-pass and candidate rows — with k_sq_list_scan behind
// launch_list_scan.  Two group forms: 16 probing queries (four waves, 512 rows per work item) and 64 (eight waves, 1024 rows), chosen as
// for IVF-Flat from the probing queries per list; "ivf_qtiles" 0 forces 16, >= 2 forces 64.  "scan_chunk" does not apply to this kind.
static void ivf_sq_scan(rsx_index* h, const BatchPlan& P, BatchResult& R, StageTimer& tm) {
    const int64_t nq = P.nq, npairs = nq * P.nprobe; const int nlist = h->nlist, nprobe = P.nprobe, ld = h->ld;
    h->w_sqhi.ensure((size_t)nq * ld * 2); h->w_sqlo.ensure((size_t)nq * ld * 2); h->w_sqc.ensure((size_t)nq * 8);
    launch_sq_query_factors(h->w_q32.as<float>(), ld, nq, nq, h->d, ld, h->d_sq.as<float>(), h->w_sqhi.as<__half>(), h->w_sqlo.as<__half>(),
                            h->w_sqc.as<float>(), h->st);
    tm.mark("sq_factors");
    const PairArea pr(h, nq, nprobe, nlist);
    const int64_t qpl = npairs / std::max(1, nlist);
    const int ls_qt = h->ivf_qtiles == 0 ? 1 : h->ivf_qtiles > 1 ? 4 : (qpl >= 12 ? 4 : 1);
    const int base_rows = sq_list_scan_chunk_rows(1), item_rows = sq_list_scan_chunk_rows(ls_qt);
    pr.group(16 * ls_qt, item_rows, nprobe, 0, h->st);
    tm.mark("group");
    ListScanArgs a = list_scan_args(h, P.nq, P.tmax, pr);
    a.sq_codes = h->data.as<uint8_t>(); a.sq_qhi = h->w_sqhi.as<__half>(); a.sq_qlo = h->w_sqlo.as<__half>(); a.sq_qc = h->w_sqc.as<float>();
    a.sq_dis0 = h->by_residual ? h->w_dis0.as<float>() : nullptr;
    a.chunk_rows = base_rows; a.qtiles = ls_qt;
    a.max_chunks = (int)std::max<int64_t>(1, (P.maxlen + base_rows - 1) / base_rows);
    const int64_t pre_chunks = std::max<int64_t>(1, ((int64_t)P.KP * std::max(1, h->ivf_pre_mult) + base_rows - 1) / base_rows);
    const bool want_filter = P.ivf_filter != 0 && nprobe > 1 && pre_chunks <= 32 && (P.ivf_filter > 1 || nq * P.tmax >= (int64_t)500000000);
    if (want_filter) R.filtered = ivf_flat_filtered(h, P, R, a, pr, ls_qt, item_rows, pre_chunks, tm);
    if (!R.filtered) {
        a.chunk_rows = item_rows; a.qtiles = ls_qt;
        a.max_chunks = (int)std::max<int64_t>(1, (P.maxlen + item_rows - 1) / item_rows);
        // (after a filtered attempt the grouping in place is the filtered scan's: the same groups and items)
        a.item_off = pr.item_off; a.total_items = pr.total_items; a.max_items = (int)max_scan_items(h, nq, nprobe, 16 * ls_qt, item_rows);
        launch_list_scan(a, h->st);
        h->timing["ivfsq_scan_launches"] += 1;
        tm.mark("scan");
    }
}
// per-query k-selection over the score rows (after a filtered search's selector mask) or the candidate rows
static void select_stage(rsx_index* h, const BatchPlan& P, const BatchResult& R, StageTimer& tm) {
    const int64_t nq = P.nq; uint64_t* state = h->w_state.as<uint64_t>();
    if (h->sel) {
        // filtered search (the plan turned the in-scan candidate filters off): the scans above wrote complete score rows —
        // approximate (certified fast scans) or exact — and the unselected rows leave them before the selection
        if (R.filtered) RSX_THROW(RSX_ERR_INVALID, "filtered search reached a scan without score rows");
        SelApplyArgs sa{};
        sa.temp = h->w_temp.as<float>(); sa.tstride = P.tmax; sa.nq = nq; sa.mask = h->sel_mask.as<uint32_t>(); sa.flat_n = -1;
        sa.probe_list = h->w_probelist.as<int32_t>(); sa.seg_start = h->w_segstart.as<int64_t>(); sa.nprobe = P.nprobe;
        sa.list_base = h->d_base.as<int64_t>(); sa.list_len = h->d_len.as<int64_t>();
        launch_sel_apply(sa, h->st);
        tm.mark("sel_apply");
    }
    if (R.filtered && R.use_gather) {
        PQGatherArgs gs = R.gs; if (R.use_tab) gs.KP = 0;        // gather only
        launch_pq_gather_select(gs, nq, h->st);
    } else if (R.filtered && R.use_tab) {
        // the compaction has laid the survivors end to end in the candidate rows already
    } else if (R.filtered) {
        // merge the filtered candidates (keys) into state0
        merge_key_rows(h, h->w_cand.p, h->w_candcnt.as<unsigned long long>(), R.cand_cap, nq, state, state, P.KP, P.BUF);
    } else {
        // fast scan: the certificate needs the TRUE top-K' by approximate score, so the selection threshold
        // is the K'-th key, not the k-th
        select_rows(h, h->w_temp.as<float>(), P.tmax, h->w_segstart.as<int64_t>() + P.nprobe, P.nprobe + 1, P.tmax, 0, nq, P.KP, P.BUF,
                    (P.fast || h->kind == KIND_IVFFLAT || h->kind == KIND_IVFSQ) ? P.KP : P.k, state, false);
    }
    tm.mark("select");
    if (R.filtered && h->profile >= 2) {   // diagnostics: keys that passed the in-kernel filter
        std::vector<unsigned long long> cnts((size_t)nq * CCS);
        HIPCHECK(hipMemcpyAsync(cnts.data(), h->w_candcnt.p, (size_t)nq * 8 * CCS, hipMemcpyDeviceToHost, h->st));
        HIPCHECK(hipStreamSynchronize(h->st));
        double tot = 0, mx = 0;
        for (int64_t qi = 0; qi < nq; qi++) { const double c = (double)cnts[(size_t)qi * CCS]; tot += c; mx = std::max(mx, c); }
        h->timing["cand_keys"] += tot; h->timing["cand_keys_max"] = std::max(h->timing["cand_keys_max"], mx);
    }
}
// large K' (the reference's n_docs = 100 ... 2000): thousands of candidates per query are re-scored, and in the scan layouts a candidate's
// M code bytes are M / 16 pieces in as many 64-byte sectors — the finalize then runs at the HBM's random-sector rate.  A row-major copy
// of the codes (pq_plain_stride(M) bytes per vector more — 128 at M = 96, so that a row is ONE 128-byte line: 288 GB of HBM hold it); built on the first such search of an
// index state, dropped by the next add.  rsx_set_param "pq_plain_codes" = 0 turns it off.
static void plain_codes(rsx_index* h, const BatchPlan& P, FinalizeArgs& fa) {
    if (!(P.rot && P.KP >= 256 && h->pq_plain_codes != 0 && h->M >= 32 && h->M % 16 == 0 && h->M == h->Mpad)) return;
    if (h->plain_gen != h->dir_gen || h->plain_of != h->data.p) {
        const size_t need = (size_t)std::max<int64_t>(h->total_cap, 1) * (size_t)pq_plain_stride(h->M);
        size_t fr = 0, tot = 0;
        h->plain_of = nullptr;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && (h->codes_plain.bytes >= need || fr > need + need / 8 + ((size_t)8 << 30))) {
            h->codes_plain.ensure(need);
            launch_pq_plain_rows(h->data.as<uint8_t>(), h->total_cap, h->M, h->CB, h->codes_plain.as<uint8_t>(), h->st);
            h->plain_gen = h->dir_gen; h->plain_of = h->data.p;
            h->timing["plain_codes_builds"] += 1;
        }
    }
    if (h->plain_of == h->data.p && h->plain_gen == h->dir_gen) { fa.codes_plain = h->codes_plain.as<uint8_t>(); fa.plain_stride = pq_plain_stride(h->M); }
}
static void finalize_stage(rsx_index* h, const BatchPlan& P, const BatchResult& R, FinalizeArgs& fa, StageTimer& tm) {
    const int64_t nq = P.nq;
    fa.probe_list = h->w_probelist.as<int32_t>(); fa.seg_start = h->w_segstart.as<int64_t>(); fa.nprobe = P.nprobe;
    if (R.flag_overflows) { fa.cand_cnt = h->w_candcnt.as<unsigned long long>(); fa.cand_cap = R.cand_cap; }     // IVF-Flat: certify_rows flags the overflowed rows' queries
    if (P.fast) {
        fa.pq_rescore = 1; fa.codes = h->data.as<uint8_t>(); fa.M = h->M; fa.Mpad = h->Mpad; fa.CB = h->CB;
        plain_codes(h, P, fa);
        fa.lut32 = P.pq_fused_lut ? nullptr : h->w_lut.as<float>();
        if (h->metric == RSX_METRIC_L2) fa.lut32 = lut32_out(h, P);       // the negated tables the builder stored (plan: tab_expected)
        fa.codebooks = h->d_codebooks.as<float>(); fa.dsub = h->dsub;
        fa.probe_dis0 = h->w_dis0.as<float>(); fa.qparam = h->w_qparam.p;
        fa.uncertain = h->w_uncertain.as<int32_t>();
        if (R.filtered) { fa.cand_cnt = h->w_candcnt.as<unsigned long long>(); fa.cand_cap = R.cand_cap; }
    }
    if (R.use_tab) {
        // (the tie scratch is allocated where k_pq_final_tab actually runs, not whenever it is a possible second chance)
        h->w_tiews.ensure((size_t)nq * R.cand_cap * 8);
        FinalizeArgs ft = fa; if (lut32_out(h, P)) ft.lut32 = lut32_out(h, P);
        if (h->profile >= 2) {      // diagnostics: how many candidates the 2 eps cut of k_pq_final_tab leaves to the exact re-score
            h->w_flag.ensure(16);
            HIPCHECK(hipMemsetAsync(h->w_flag.p, 0, 16, h->st));
            ft.stat = reinterpret_cast<unsigned long long*>(h->w_flag.p);
        }
        launch_pq_final_tab(ft, h->w_cand.as<uint64_t>(), R.cand_cap, h->w_tiews.as<uint64_t>(), h->st);
        if (h->profile >= 2) {
            unsigned long long v = 0;
            HIPCHECK(hipMemcpyAsync(&v, h->w_flag.p, 8, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipStreamSynchronize(h->st));
            h->timing["final_tab_rescored"] += (double)v;
        }
    }
    else launch_finalize(fa, h->st);
    tm.mark("finalize");
}
// the second chance of rerun_uncertified (flag 1): after the one-launch pre-pass the flagged queries' candidate rows are complete
static std::function<void()> pq_second_chance(rsx_index* h, const BatchPlan& P, const BatchResult& R, const FinalizeArgs& fa) {
    if (!(P.fast && R.filtered && R.fused_pre_used && !R.use_tab)) return nullptr;
    if (R.tab_fits)
        return [h, P, R, fa]() {       // settle them from there (k_pq_final_tab)
            h->timing["rescore_all_launches"] += 1;
            FinalizeArgs fr = fa; fr.row_filter = h->w_uncertain.as<int32_t>();
            h->w_tiews.ensure((size_t)P.nq * R.cand_cap * 8);
            launch_pq_final_tab(fr, h->w_cand.as<uint64_t>(), R.cand_cap, h->w_tiews.as<uint64_t>(), h->st);
        };
    return [h, P, R, fa]() {
        // the flagged queries' candidate rows are complete (threshold by construction) and did not overflow: score every
        // candidate exactly in place, then the best K2 >= k + 64 of them by (exact score, index) go through k_finalize for
        // the (score, id) order — no certificate needed, no exact scan
        h->timing["rescore_all_launches"] += 1;
        FinalizeArgs fr = fa; fr.row_filter = h->w_uncertain.as<int32_t>();
        launch_pq_rescore_all(fr, h->w_cand.as<uint64_t>(), R.cand_cap, h->st);
        const int KP2 = std::min(4096, std::max(128, pow2ceil(P.k + 64)));
        h->w_state2.ensure((size_t)P.nq * KP2 * 8);
        merge_key_rows(h, h->w_cand.p, h->w_candcnt.as<unsigned long long>(), R.cand_cap, P.nq, nullptr, h->w_state2.as<uint64_t>(),
                       KP2, 2 * KP2, h->w_uncertain.as<int32_t>());
        FinalizeArgs f2 = fa;
        f2.state = h->w_state2.as<uint64_t>(); f2.KP = KP2; f2.row_filter = h->w_uncertain.as<int32_t>(); f2.no_cert = 1;
        launch_finalize(f2, h->st);
    };
}
// one internal batch: queries -> (coarse quantiser, probes) -> scan -> selection -> finalize -> certificate re-runs
static void search_batch(rsx_index* h, int64_t nq, const void* dq, int dtype, int k, float* dD, int64_t* dI, bool allow_fast) {
    StageTimer tm(h, allow_fast ? "" : "fb_");
    const BatchPlan P = plan_batch(h, nq, dq, dtype, k, allow_fast);
    tm.mark("start");
    convert_queries(h, P, dq, dtype, tm);
    if (P.tab_expected) h->w_lut.ensure((size_t)nq * h->Mpad * 256 * 4);      // (lut32_out)
    check_supported(h, P);
    FinalizeArgs fa = finalize_args(h, P, dD, dI);
    if (h->kind == KIND_FLAT) {
        flat_scan(h, P, fa, tm);
        launch_finalize(fa, h->st); tm.mark("finalize"); tm.finish();
        if (P.certify && h->ntotal > 0) rerun_uncertified(h, nq, dq, dtype, k, dD, dI, (size_t)round_up(h->ntotal, 16) * 4, false);
        return;
    }
    coarse_quantiser(h, P, dq, dtype, tm);
    if (h->profile >= 2) count_scanned(h, P, tm);
    if (P.needs_score_rows) h->w_temp.ensure((size_t)nq * P.tmax * 4);
    BatchResult R;
    if (h->kind == KIND_IVFPQ) pq_scan(h, P, R, tm);
    else if (!allow_fast) ivf_flat_exact(h, P, tm);
    else if (h->kind == KIND_IVFSQ) ivf_sq_scan(h, P, R, tm);
    else ivf_flat_scan(h, P, R, tm);
    select_stage(h, P, R, tm);
    finalize_stage(h, P, R, fa, tm);
    if (!allow_fast && h->kind != KIND_IVFPQ) {
        // the exact re-run's selection cut a run of equal scores by column: the ids of that score by id (k_exact_tie_ids)
        ExactTieArgs ta{};
        ta.state = h->w_state.as<uint64_t>(); ta.KP = P.KP; ta.k = P.k; ta.nq = nq; ta.temp = h->w_temp.as<float>(); ta.tstride = P.tmax;
        ta.probe_list = h->w_probelist.as<int32_t>(); ta.seg_start = h->w_segstart.as<int64_t>(); ta.nprobe = P.nprobe;
        ta.list_base = h->d_base.as<int64_t>(); ta.list_len = h->d_len.as<int64_t>(); ta.ids = h->ids.as<int64_t>(); ta.I = dI;
        launch_exact_tie_ids(ta, h->st);
        tm.mark("tie_ids");
    }
    tm.finish();
    // (the re-run fills score rows: chunked by the budget; the fast coarse quantiser's flags are this batch's)
    if (P.fast || P.certify) rerun_uncertified(h, nq, dq, dtype, k, dD, dI, (size_t)P.tmax * 4, P.coarse_fast, pq_second_chance(h, P, R, fa));
}

// The slot mask of h->sel over the handle's storage (k_sel_mask), rebuilt only when the selector or the index state changed: every
// add / add_list / reset / re-layout bumps dir_gen (upload_dir), and a re-layout also moves the storage.
static void ensure_sel_mask(rsx_index* h) {
    const rsx_selector* s = h->sel;
    if (h->sel_mask.p && h->sel_mask_serial == s->serial && h->sel_mask_gen == h->dir_gen && h->sel_mask_of == h->data.p) return;
    const int64_t nslots = std::max<int64_t>(h->total_cap, h->ntotal);
    h->sel_mask.ensure((size_t)std::max<int64_t>(1, sel_mask_words(nslots)) * 4);
    const auto t0 = std::chrono::steady_clock::now();
    SelDevArgs a{};
    a.kind = s->kind; a.invert = s->invert; a.lo = s->lo; a.hi = s->hi;
    const size_t bytes = s->kind == RSX_SEL_BITMAP ? s->bitmap.size() : s->kind == RSX_SEL_BATCH ? s->ids.size() * 8 : 0;
    if (bytes) {
        const void* src = s->kind == RSX_SEL_BITMAP ? (const void*)s->bitmap.data() : (const void*)s->ids.data();
        h->sel_dev.ensure(bytes);
        HIPCHECK(hipMemcpyAsync(h->sel_dev.p, src, bytes, hipMemcpyHostToDevice, h->st));
    }
    a.bitmap = s->kind == RSX_SEL_BITMAP ? h->sel_dev.as<uint8_t>() : nullptr; a.nbytes = (int64_t)s->bitmap.size();
    a.ids = s->kind == RSX_SEL_BATCH ? h->sel_dev.as<int64_t>() : nullptr; a.nids = (int64_t)s->ids.size();
    const int64_t* slot_ids = (h->kind == KIND_FLAT && !h->custom_ids) ? nullptr : h->ids.as<int64_t>();     // (as k_finalize reads them)
    launch_sel_mask(a, slot_ids, nslots, h->sel_mask.as<uint32_t>(), h->st);
    HIPCHECK(hipStreamSynchronize(h->st));      // (the selector's host arrays may go away after the call)
    HIPCHECK(hipGetLastError());
    h->sel_mask_serial = s->serial; h->sel_mask_gen = h->dir_gen; h->sel_mask_of = h->data.p;
    h->timing["sel_mask_builds"] += 1;
    h->timing["sel_mask_ms"] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void search_impl(rsx_index* h, int64_t nq, const void* q, int dtype, int k, float* D, int64_t* I) {
    if (nq < 0 || k <= 0) RSX_THROW(RSX_ERR_INVALID, "search: nq=%lld k=%d", (long long)nq, k);
    if (k > 4096) RSX_THROW(RSX_ERR_UNSUPPORTED, "search: k = %d exceeds this build's maximum of 4096 (the reference backends' default k)", k);
    if (!h->trained) RSX_THROW(RSX_ERR_NOT_TRAINED, "search before train");
    if (nq == 0) return;
    if (!q || !D || !I) RSX_THROW(RSX_ERR_INVALID, "search: null pointer");
    bool q_dev = is_device_ptr(q), o_dev = is_device_ptr(D);
    if (o_dev != is_device_ptr(I)) RSX_THROW(RSX_ERR_INVALID, "search: D and I must both be host or both device pointers");
    size_t esz = dtype == RSX_F16 ? 2 : 4;

    if (h->ntotal == 0) {  // FAISS returns -1 / -inf for an empty index
        std::vector<float> hd((size_t)nq * k, h->metric == 0 ? -INFINITY : INFINITY);
        std::vector<int64_t> hi((size_t)nq * k, -1);
        HIPCHECK(hipMemcpy(D, hd.data(), hd.size() * 4, o_dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
        HIPCHECK(hipMemcpy(I, hi.data(), hi.size() * 8, o_dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
        return;
    }
    if (h->metric == RSX_METRIC_L2 && h->kind != KIND_IVFPQ) l2_bias_rows(h);
    if (h->sel) ensure_sel_mask(h);
    // batch size: bounded by the knob and by the score-buffer budget (the plan's row sizes depend on neither nq nor the query buffer)
    int64_t qb = std::max(1, h->query_batch);
    if (h->kind != KIND_FLAT) {
        const BatchPlan P = plan_batch(h, nq, nullptr, dtype, k, true);
        if (P.needs_score_rows) qb = std::max<int64_t>(1, std::min<int64_t>(qb, h->temp_budget / (P.tmax * 4)));
        else qb = std::max<int64_t>(1, std::min<int64_t>(qb, h->temp_budget / (cand_row_cap(k, h->M) * 16)));      // candidate row + tie scratch
    } else if (nq <= 32) {
        qb = 32;
    }
    for (int64_t q0 = 0; q0 < nq; q0 += qb) {
        int64_t nb = std::min(qb, nq - q0);
        const void* dq;
        const bool small = nb <= 64;      // latency path: stage through pinned memory (see PinBuf)
        if (q_dev) dq = (const char*)q + (size_t)q0 * h->d * esz;
        else {
            const size_t qbytes = (size_t)nb * h->d * esz;
            const char* src = (const char*)q + (size_t)q0 * h->d * esz;
            h->w_qin.ensure(qbytes);
            if (small && h->pin_q.ensure(qbytes)) { memcpy(h->pin_q.p, src, qbytes); src = h->pin_q.as<char>(); }
            HIPCHECK(hipMemcpyAsync(h->w_qin.p, src, qbytes, hipMemcpyHostToDevice, h->st));
            dq = h->w_qin.p;
        }
        float* dD; int64_t* dI;
        if (o_dev) { dD = D + q0 * k; dI = I + q0 * k; }
        else {
            h->w_D.ensure((size_t)nb * k * 4); h->w_I.ensure((size_t)nb * k * 8);
            dD = h->w_D.as<float>(); dI = h->w_I.as<int64_t>();
        }
        if (h->sel) h->timing["filtered_queries"] += (double)nb;
        search_batch(h, nb, dq, dtype, k, dD, dI);
        const size_t dbytes = (size_t)nb * k * 4, ibytes = (size_t)nb * k * 8;
        const bool pin_out = !o_dev && small && h->pin_out.ensure(round_up(dbytes, 16) + ibytes);
        if (pin_out) {
            HIPCHECK(hipMemcpyAsync(h->pin_out.p, dD, dbytes, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipMemcpyAsync(h->pin_out.as<char>() + round_up(dbytes, 16), dI, ibytes, hipMemcpyDeviceToHost, h->st));
        } else if (!o_dev) {
            HIPCHECK(hipMemcpyAsync(D + q0 * k, dD, dbytes, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipMemcpyAsync(I + q0 * k, dI, ibytes, hipMemcpyDeviceToHost, h->st));
        }
        HIPCHECK(hipStreamSynchronize(h->st));
        if (pin_out) {
            memcpy(D + q0 * k, h->pin_out.p, dbytes);
            memcpy(I + q0 * k, h->pin_out.as<char>() + round_up(dbytes, 16), ibytes);
        }
    }
    HIPCHECK(hipGetLastError());
}

