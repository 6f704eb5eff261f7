// api_sqflat.hip — the search driver of IndexScalarQuantizer (RSX_KIND_SQ, rsx_index::flat_sq).  The handle is an IVF-SQ index
// of ONE list (api_build.hip: create_flat_sq), so batches of at most 32 queries, an empty index and "flat_cert" = 0 go to search_impl and
// take that kind's one-list routes.  Larger batches take the staged int8 GEMM scan below: flat_staged's design (api_search.hip) — a
// threshold phase through the score buffer, geometrically growing stages of ONE filtered launch each against the running K'-th key with
// deferred per-stage counters, k_finalize with its certificate, a second search of the queries it cannot clear (sqf_rerun) — over k_sq_gemm
// (k_sq_gemm.hip) in place of k_flat_gemm2, the candidates re-scored from their decoded rows (k_finalize<SQ>: rescore_rows_sq).
// A key's index is the storage row: the one list starts at row 0 and a query's score row is that list, so k_finalize's probe tables map
// column c to row c.
#include "rsx_stages.h"
#include "rsx_sqflat.h"

namespace {

struct SqfPlan { int64_t nq, nq_pad; int k, KP, BUF, ldp, wmax; };

SqfPlan sqf_plan(const rsx_index* h, int64_t nq, int k) {
    SqfPlan P{};
    P.nq = nq; P.nq_pad = round_up(nq, 128); P.k = k;
    // K' of the row kinds (api_search.hip: kp_for), doubled below 1024 where it holds fewer than 2 k + 16 keys: the planes' bound is wider than
    // the fp16 scans', and the gap it has to clear grows with the depth of the cut (k = 100: K' = 256, where 128 re-ran 0.5 - 20 % of a
    // 10M-row batch; k_finalize still re-scores k + max(8, k / 16) rows first and the rest only where that does not certify)
    P.KP = std::max(16, pow2ceil(k + std::max(8, k / 16)));
    if (P.KP < 2 * k + 16 && P.KP < 1024) P.KP *= 2;
    P.BUF = std::max(2 * P.KP, 256);
    P.ldp = (int)round_up(h->ld, 128); P.wmax = sqflat_wmax(h->d);
    return P;
}

// the probe tables of the one list (w_probelist, w_dis0, w_segstart) and the fp32 queries: what k_finalize and the exact scores read
void sqf_queries(rsx_index* h, const void* dq, int dtype, int64_t nq, int64_t nq_pad) {
    convert_scan_queries(h, dq, dtype, nq, nq_pad);
    coarse_exact_scores(h, nq);
    coarse_exact_probes(h, nq, 1, 16);
}

// k_finalize's arguments for the handle's code rows and the bound of the int8 scan; rho = the batch's largest max_j |q'_j| / |q|
FinalizeArgs sqf_finalize_args(rsx_index* h, const SqfPlan& P, float* dD, int64_t* dI, float rho) {
    const int d = h->d, ld = h->ld;
    FinalizeArgs fa{};
    fa.kind = KIND_IVFSQ; fa.metric = h->metric; fa.state = h->w_state.as<uint64_t>(); fa.KP = P.KP; fa.k = P.k; fa.nq = P.nq;
    fa.list_base = h->d_base.as<int64_t>(); fa.ids = h->ids.as<int64_t>();
    fa.probe_list = h->w_probelist.as<int32_t>(); fa.seg_start = h->w_segstart.as<int64_t>(); fa.nprobe = 1;
    fa.Q32 = h->w_q32.as<float>(); fa.ldq = ld; fa.d = d; fa.X = nullptr; fa.x_f16 = 1; fa.ld = ld; fa.D = dD; fa.I = dI;
    fa.sq = SqRows{h->data.as<uint8_t>(), h->d_sq.as<float>(), nullptr, h->d_base.as<int64_t>(), 1};
    fa.KPv = std::min(P.KP, P.k + std::max(8, P.k / 16));
    const ScanBound sb = scan_cert_bound(h);
    h->w_uncertain.ensure((size_t)P.nq * 8);
    fa.uncertain = h->w_uncertain.as<int32_t>(); fa.cert_qflag = nullptr;
    fa.cert_rel = 0.0f; fa.cert_rel_qlossy = 0.0f; fa.cert_xmax = sb.xmax; fa.cert_abs = sb.abs;
    // The scan's score of a stored vector x^ is  fl(fl(fl(A) fl(1 / s)) + qc) (+ -|x^|^2 / 2)  with A = sum_j w_j b_j EXACT, b_j = code_j - 128,
    // w_j = rint(fl(q'_j s)), q'_j = fl(fl(q_j vdiff_j) / 255), s = fl(wmax / max_j |q'_j|); the exact score is the fp64 product of q with the
    // decoded x^.  Per unit of |q|, with r = max_j vdiff_j / 255 (|q'|_2 <= r |q|), rho = the largest max_j |q'_j| / |q| of the batch's queries
    // (k_sqflat_planes; rho <= r, and several times smaller unless a query is all in one dimension), B = the largest |b|_2 of a stored row
    // (kept by the encoder), V = |vdiff|, W = |vmin|:
    //   the rounding to integers: |w_j / s - q'_j| <= 1 / (2 s) + 2^-24 |q'_j|, summed against |b_j| with |b|_1 <= sqrt(d) B and
    //   1 / s <= (1 + 2^-23) max_j |q'_j| / wmax                                      (sqrt(d) / (2 wmax)) (1 + 2^-22) rho B  +  2^-24 r B
    //   fl(A), fl(1 / s) and their product, on |A / s| <= (1 + sqrt(d) / (2 wmax)) r B  4 2^-24 (1 + sqrt(d) / (2 wmax)) r B
    //   q' itself: two fp32 roundings                                                  2 2^-24 r B
    //   the decode's three roundings, qc rounded to fp32, the operations that assemble the score (finalize_args, api_search.hip)   10 2^-24 (V + W)
    // cert_abs (the score's own fp32 rounding, the L2 norm term) stays as for the other row kinds.  tests/sqflat_ref.py restates this bound
    // (cert_eps); tests/test_sqflat_host.py checks it against every (query, row) pair of the input sets.
    const float u24 = 5.9604645e-8f;
    const float hw = sqrtf((float)d) / (2.0f * (float)P.wmax);
    const float rel_b = (u24 + 4.0f * u24 * (1.0f + hw) + 2.0f * u24) * 1.01f;
    const float Bn = sqrtf((float)h->sq_bn2) * 1.00001f;
    const float r = (h->sq_vdmax / 255.0f) * 1.00001f;
    fa.cert_q = hw * 1.000001f * 1.01f * std::min(rho, r) * Bn + rel_b * r * Bn + 10.0f * u24 * 1.01f * (h->sq_nvdiff + h->sq_nvmin);
    return fa;
}

// merge key rows [nrows, cap] (row r holds cnt[r * CCS] keys) into state rows [nrows, KP] (api_search.hip: merge_key_rows)
void sqf_merge_key_rows(rsx_index* h, const void* keys, const unsigned long long* cnt, int cap, int64_t nrows, uint64_t* state, int KP, int BUF) {
    SelectArgs b{};
    b.in = keys; b.in_is_keys = 1; b.row_stride = cap;
    b.row_n = reinterpret_cast<const int64_t*>(cnt); b.row_n_stride = CCS; b.n_uniform = cap;
    b.seg_len = round_up(cap, 256); b.nseg = 1; b.idx_base = 0;
    b.init = state; b.out = state; b.out_row_stride = KP;
    b.nrows = nrows; b.KP = KP; b.BUF = BUF; b.k = KP;
    launch_select(b, h->st);
}

// The queries k_finalize flagged (certificate, or a stage row that overflowed) are gathered, searched again and their result rows replaced.
// The second search is search_impl over the handle as the one-list IVF-SQ index it is: k_sq_list_scan's fp16 scan, whose bound is several
// times tighter than the int8 planes' (one pass over the codes per 16 such queries), and behind it that kind's exact re-run
// (k_sq_exact_scores, equal scores by id) for what no certificate clears.  "fallback_queries" counts the queries flagged HERE; the ones that
// went on to the exact scores are "sqflat_exact_queries".
void sqf_rerun(rsx_index* h, int64_t nq, const void* dq, int dtype, int k, float* dD, int64_t* dI) {
    HIPCHECK(hipStreamSynchronize(h->st));
    std::vector<int32_t> bad((size_t)nq);
    if (h->w_uncertain.host_mapped) bad.assign(h->w_uncertain.as<int32_t>(), h->w_uncertain.as<int32_t>() + nq);
    else HIPCHECK(hipMemcpy(bad.data(), h->w_uncertain.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    std::vector<int64_t> badq;
    for (int64_t q = 0; q < nq; q++) if (bad[(size_t)q]) badq.push_back(q);
    const int64_t nbad = (int64_t)badq.size();
    h->timing["fallback_queries"] += (double)nbad;
    h->timing["fast_queries"] += (double)nq;
    if (nbad == 0) return;
    const size_t qrow = (size_t)h->d * (dtype == RSX_F16 ? 2 : 4);
    h->w_sqfbq.ensure((size_t)nbad * qrow);          // (buffers of their own: search_impl's re-run gathers into w_fbq / w_fbD / w_fbI)
    h->w_sqfbD.ensure((size_t)nbad * k * 4);
    h->w_sqfbI.ensure((size_t)nbad * k * 8);
    for (int64_t i = 0; i < nbad; i++)
        HIPCHECK(hipMemcpyAsync((char*)h->w_sqfbq.p + (size_t)i * qrow, (const char*)dq + (size_t)badq[(size_t)i] * qrow, qrow, hipMemcpyDeviceToDevice, h->st));
    HIPCHECK(hipStreamSynchronize(h->st));
    const double fb0 = h->timing["fallback_queries"], fq0 = h->timing["fast_queries"];
    search_impl(h, nbad, h->w_sqfbq.p, dtype, k, h->w_sqfbD.as<float>(), h->w_sqfbI.as<int64_t>());
    h->timing["sqflat_exact_queries"] += h->timing["fallback_queries"] - fb0;
    h->timing["fallback_queries"] = fb0; h->timing["fast_queries"] = fq0;
    for (int64_t i = 0; i < nbad; i++) {
        HIPCHECK(hipMemcpyAsync(dD + badq[(size_t)i] * k, h->w_sqfbD.as<float>() + i * k, (size_t)k * 4, hipMemcpyDeviceToDevice, h->st));
        HIPCHECK(hipMemcpyAsync(dI + badq[(size_t)i] * k, h->w_sqfbI.as<int64_t>() + i * k, (size_t)k * 8, hipMemcpyDeviceToDevice, h->st));
    }
}

// profile != 0: stage times on the stream, summed per name (as search_batch's marks)
struct SqfMarks {
    rsx_index* h; bool on; hipEvent_t ev[64]; const char* name[64]; int n = 0;
    explicit SqfMarks(rsx_index* hh) : h(hh), on(hh->profile > 0) {}
    void mark(const char* nm) { if (!on || n >= 64) return; (void)hipEventCreate(&ev[n]); (void)hipEventRecord(ev[n], h->st); name[n++] = nm; }
    void finish() {
        if (n == 0) return;
        (void)hipEventSynchronize(ev[n - 1]);
        for (int i = 1; i < n; i++) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[i - 1], ev[i]); h->timing[name[i]] += ms; }
        float tot = 0; (void)hipEventElapsedTime(&tot, ev[0], ev[n - 1]); h->timing["total"] += tot;
        for (int i = 0; i < n; i++) (void)hipEventDestroy(ev[i]);
        n = 0;
    }
};

// one internal batch of more than 32 device-resident queries through the staged int8 scan
void sqf_batch(rsx_index* h, int64_t nq, const void* dq, int dtype, int k, float* dD, int64_t* dI) {
    const SqfPlan P = sqf_plan(h, nq, k);
    const int64_t N = h->h_len[0], CH = 65536; const int ld = h->ld, KP = P.KP;
    SqfMarks tm(h);
    tm.mark("start");
    sqf_queries(h, dq, dtype, nq, P.nq_pad);
    h->w_sqplanes.ensure((size_t)P.nq_pad * 2 * P.ldp); h->w_sqs.ensure((size_t)P.nq_pad * 8 + 16);
    const int8_t* planes = h->w_sqplanes.as<int8_t>(); const float* qs = h->w_sqs.as<float>();
    unsigned int* rho_bits = reinterpret_cast<unsigned int*>(h->w_sqs.as<float>() + 2 * P.nq_pad);
    HIPCHECK(hipMemsetAsync(rho_bits, 0, sizeof(unsigned int), h->st));
    launch_sqflat_planes(h->w_q32.as<float>(), ld, nq, P.nq_pad, h->d, P.ldp, h->d_sq.as<float>(), P.wmax, h->w_sqplanes.as<int8_t>(), h->w_sqs.as<float>(), rho_bits, h->st);
    tm.mark("sq_factors");
    const uint8_t* codes = h->data.as<uint8_t>();
    const float* bias = h->metric == RSX_METRIC_L2 ? h->w_misc.as<float>() : nullptr;
    h->w_state.ensure((size_t)nq * KP * 8);
    uint64_t* state = h->w_state.as<uint64_t>();
    h->w_temp.ensure((size_t)P.nq_pad * CH * 4);
    launch_fill_u64(state, nq * KP, 0, h->st);
    FinalizeArgs fa = sqf_finalize_args(h, P, dD, dI, 0.0f);
    float rho = 0.0f;                              // read back behind the scan (below): the one host round trip of a batch before its finalize
    auto chunk_pass = [&](int64_t v0, int64_t vend) {
        const int64_t nv = std::min<int64_t>(CH, vend - v0);
        launch_sqflat_gemm(planes, qs, (int)P.nq_pad, P.ldp, codes, v0, nv, ld, bias, h->w_temp.as<float>(), CH, h->st);
        h->timing["sqflat_gemm_launches"] += 1;
        select_rows(h, h->w_temp.as<float>(), CH, nullptr, 0, nv, (uint32_t)v0, nq, KP, P.BUF, KP, state, true);
    };
    // threshold phase and stage boundaries: flat_staged's rules and knobs ("flat_pre_unit", "flat_pre_mult", "flat_stages")
    const int64_t U = h->flat_pre_unit > 0 ? std::min<int64_t>(CH, round_up(h->flat_pre_unit, 256)) : (KP <= 64 ? CH / 4 : CH / 2);
    const int64_t nchunks = (N + U - 1) / U;
    const int64_t n0 = std::min<int64_t>(nchunks, std::max<int64_t>(1, ((int64_t)KP * std::max(1, h->flat_pre_mult) + U - 1) / U));
    for (int64_t c = 0; c < n0; c++) chunk_pass(c * U, std::min<int64_t>(N, (c + 1) * U));
    int64_t done_rows = std::min<int64_t>(n0 * U, N);
    tm.mark("scan0");
    if (done_rows < N) {
        int S = h->flat_stages;
        if (S <= 0) S = KP <= 64 ? 2 : std::min(6, std::max(1, (int)lround(log((double)nchunks / (double)n0) / log(3.0))));
        const double r = pow((double)nchunks / (double)n0, 1.0 / S);
        const int cap = h->sqflat_cand_cap > 0 ? h->sqflat_cand_cap : (KP <= 64 ? 32768 : 131072);
        h->w_cand.ensure((size_t)nq * cap * 8);
        // every stage owns a set of per-query counters; the selection clamps an overflowed row to the buffer and k_finalize flags a query any
        // of whose stage rows overflowed: it joins the exact re-run, the batch is not scanned again
        const size_t cc_stride = (size_t)nq * CCS;
        h->w_candcnt.ensure(cc_stride * 8 * (size_t)S);
        HIPCHECK(hipMemsetAsync(h->w_candcnt.p, 0, cc_stride * 8 * (size_t)S, h->st));
        int stages_run = 0;
        for (int st_ = 0; st_ < S && done_rows < N; st_++) {
            const int64_t endc = st_ == S - 1 ? nchunks : std::min<int64_t>(nchunks, std::max<int64_t>(done_rows / U + 1, (int64_t)llround((double)n0 * pow(r, st_ + 1))));
            const int64_t end = std::min<int64_t>(N, endc * U);
            unsigned long long* cc = h->w_candcnt.as<unsigned long long>() + cc_stride * (size_t)st_;
            launch_sqflat_gemm_filter(planes, qs, (int)P.nq_pad, (int)nq, P.ldp, codes, done_rows, end - done_rows, ld, bias, state + (KP - 1), KP,
                                      h->w_cand.as<uint64_t>(), cc, cap, h->st);
            h->timing["sqflat_gemm_launches"] += 1;
            tm.mark("scan");
            sqf_merge_key_rows(h, h->w_cand.p, cc, cap, nq, state, KP, P.BUF);
            tm.mark("select");
            done_rows = end;
            stages_run = st_ + 1;
        }
        h->timing["sqflat_stages"] += stages_run;
        fa.cand_cnt = h->w_candcnt.as<unsigned long long>(); fa.cand_cap = cap; fa.cand_cnt_n = stages_run; fa.cand_cnt_stride = (int64_t)cc_stride;
        if (h->profile >= 2) {      // diagnostics: keys that passed the in-kernel filter
            std::vector<unsigned long long> cnts(cc_stride * (size_t)stages_run);
            HIPCHECK(hipMemcpyAsync(cnts.data(), h->w_candcnt.p, cnts.size() * 8, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipStreamSynchronize(h->st));
            double tot = 0;
            for (int s = 0; s < stages_run; s++) for (int64_t qi = 0; qi < nq; qi++) tot += (double)cnts[(size_t)s * cc_stride + (size_t)qi * CCS];
            h->timing["cand_keys"] += tot;
        }
    }
    HIPCHECK(hipMemcpyAsync(&rho, rho_bits, sizeof(float), hipMemcpyDeviceToHost, h->st));
    HIPCHECK(hipStreamSynchronize(h->st));
    fa.cert_q = sqf_finalize_args(h, P, dD, dI, rho).cert_q;
    launch_finalize(fa, h->st);
    tm.mark("finalize");
    tm.finish();
    sqf_rerun(h, nq, dq, dtype, k, dD, dI);
}

}  // namespace

void sqflat_search(rsx_index* h, int64_t nq, const void* q, int dtype, int k, float* D, int64_t* I) {
    if (nq < 0 || k <= 0) RSX_THROW(RSX_ERR_INVALID, "search: nq=%lld k=%d", (long long)nq, k);
    if (k > 4096) RSX_THROW(RSX_ERR_UNSUPPORTED, "search: k = %d exceeds this build's maximum of 4096 (the reference backends' default k)", k);
    if (!h->trained) RSX_THROW(RSX_ERR_NOT_TRAINED, "search before train");
    if (nq == 0) return;
    if (!q || !D || !I) RSX_THROW(RSX_ERR_INVALID, "search: null pointer");
    const bool q_dev = is_device_ptr(q), o_dev = is_device_ptr(D);
    if (o_dev != is_device_ptr(I)) RSX_THROW(RSX_ERR_INVALID, "search: D and I must both be host or both device pointers");
    const size_t esz = dtype == RSX_F16 ? 2 : 4;
    const int64_t qb = std::max(1, h->query_batch);
    for (int64_t q0 = 0; q0 < nq; q0 += qb) {
        const int64_t nb = std::min(qb, nq - q0);
        const char* qp = (const char*)q + (size_t)q0 * h->d * esz;
        if (nb <= 32 || h->ntotal == 0 || h->flat_cert == 0 || h->sel) {       // the one-list routes of the IVF-SQ kind
            search_impl(h, nb, qp, dtype, k, D + q0 * k, I + q0 * k);
            continue;
        }
        if (h->metric == RSX_METRIC_L2) l2_bias_rows(h);
        const void* dq = qp;
        if (!q_dev) {
            h->w_qin.ensure((size_t)nb * h->d * esz);
            HIPCHECK(hipMemcpyAsync(h->w_qin.p, qp, (size_t)nb * h->d * esz, hipMemcpyHostToDevice, h->st));
            dq = h->w_qin.p;
        }
        float* dD = D + q0 * k; int64_t* dI = I + q0 * k;
        if (!o_dev) {
            h->w_D.ensure((size_t)nb * k * 4); h->w_I.ensure((size_t)nb * k * 8);
            dD = h->w_D.as<float>(); dI = h->w_I.as<int64_t>();
        }
        sqf_batch(h, nb, dq, dtype, k, dD, dI);
        if (!o_dev) {
            HIPCHECK(hipMemcpyAsync(D + q0 * k, dD, (size_t)nb * k * 4, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipMemcpyAsync(I + q0 * k, dI, (size_t)nb * k * 8, hipMemcpyDeviceToHost, h->st));
        }
        HIPCHECK(hipStreamSynchronize(h->st));
    }
    HIPCHECK(hipGetLastError());
}
