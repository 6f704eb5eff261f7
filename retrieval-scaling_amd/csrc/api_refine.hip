// api_refine.hip — rsx_refine's host driver: exact re-ranking of candidate labels against a Flat handle's row store (k_refine.hip).
#include "rsx_stages.h"
#include "k_rescore.h"

// rsx_refine on a Flat handle of sequential ids: the labels ARE the storage rows.  One k_refine launch per internal batch; queries, labels
// and results of host callers are staged through the handle's workspace.  The out-of-range flag is one word of page-locked host memory the
// kernel writes across the bus; it is read after the call's closing synchronisation.
void refine_impl(rsx_index* h, int64_t nq, const void* q, int dtype, int kc, const int64_t* labels, int k, float* D, int64_t* I) {
    if (nq == 0) return;
    if (!q || !labels || !D || !I) RSX_THROW(RSX_ERR_INVALID, "refine: null pointer");
    const bool q_dev = is_device_ptr(q), l_dev = is_device_ptr(labels), o_dev = is_device_ptr(D);
    if (o_dev != is_device_ptr(I)) RSX_THROW(RSX_ERR_INVALID, "refine: D and I must both be host or both device pointers");
    const size_t esz = dtype == RSX_F16 ? 2 : 4;
    const int d = h->d, ld = h->ld;
    h->w_rflag.host_mapped = true;
    h->w_rflag.ensure(sizeof(int));
    *h->w_rflag.as<int>() = 0;          // (no kernel of this handle is in flight: every call ends with a synchronisation of its stream)
    StreamTimer t_all(h->profile > 0, h->st);
    t_all.start();
    const int64_t qb = std::max(1, h->query_batch);
    for (int64_t q0 = 0; q0 < nq; q0 += qb) {
        const int64_t nb = std::min(qb, nq - q0);
        const void* dq = (const char*)q + (size_t)q0 * d * esz;
        if (!q_dev) dq = stage_rows(h, h->w_qin, dq, nb, d, dtype);
        const int64_t* dl = labels + q0 * kc;
        if (!l_dev) {
            h->w_rlabels.ensure((size_t)nb * kc * 8);
            HIPCHECK(hipMemcpyAsync(h->w_rlabels.p, dl, (size_t)nb * kc * 8, hipMemcpyHostToDevice, h->st));
            dl = h->w_rlabels.as<int64_t>();
        }
        float* dD = D + q0 * k; int64_t* dI = I + q0 * k;
        if (!o_dev) {
            h->w_D.ensure((size_t)nb * k * 4); h->w_I.ensure((size_t)nb * k * 8);
            dD = h->w_D.as<float>(); dI = h->w_I.as<int64_t>();
        }
        h->w_q32.ensure((size_t)nb * ld * 4);
        launch_convert_to_f32(dq, dtype == RSX_F16, d, nb, d, h->w_q32.as<float>(), ld, h->st);
        RefineArgs ra{};
        ra.metric = h->metric; ra.nq = nb; ra.kc = kc; ra.k = k; ra.labels = dl;
        ra.Q32 = h->w_q32.as<float>(); ra.ldq = ld; ra.d = d;
        ra.X = h->data.p; ra.x_f16 = h->storage_f16; ra.ld = ld; ra.ntotal = h->ntotal;
        ra.D = dD; ra.I = dI; ra.flag = h->w_rflag.as<int>();
        launch_refine(ra, h->st);
        if (!o_dev) {
            HIPCHECK(hipMemcpyAsync(D + q0 * k, dD, (size_t)nb * k * 4, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipMemcpyAsync(I + q0 * k, dI, (size_t)nb * k * 8, hipMemcpyDeviceToHost, h->st));
        }
        if (!q_dev || !l_dev || !o_dev) HIPCHECK(hipStreamSynchronize(h->st));     // the staging buffers serve the next batch
    }
    t_all.stop();
    HIPCHECK(hipStreamSynchronize(h->st));
    HIPCHECK(hipGetLastError());
    if (h->profile > 0) h->timing["refine_ms"] += t_all.ms();
    h->timing["refine_calls"] += 1.0;
    h->timing["refine_candidates"] += (double)nq * kc;
    if (*h->w_rflag.as<int>() != 0)
        RSX_THROW(RSX_ERR_INVALID, "refine: a label is not below ntotal = %lld (such labels were skipped; the outputs are unspecified)", (long long)h->ntotal);
}
