// rsx_api.hip — the C ABI of include/rsx.h: argument checks, error codes (rsx_last_error), dispatch to the host functions of
// api_build.hip / api_search.hip / api_sharded.hip (rsx_host.h).  Every entry point but the selector objects' needs a GPU: there is no
// CPU search path.
#include <atomic>
#include "rsx_host.h"
#include "rsx_range.h"

thread_local std::string g_err;

// The selector and the nprobe override of one filtered search (rsx_search_sel / rsx_search_prepass_sel) on the handle and its shards,
// restored when the call ends, whether it succeeds or throws (FAISS: SearchParametersIVF.nprobe does not change index.nprobe).
struct SelScope {
    rsx_index* h; int nprobe0; bool np_set;
    SelScope(rsx_index* hh, const rsx_selector* sel, int nprobe_override) : h(hh), nprobe0(hh->nprobe), np_set(nprobe_override > 0) {
        h->sel = sel;
        for (auto* c : h->shards) c->sel = sel;
        if (nprobe_override > 0) { h->nprobe = nprobe_override; for (auto* c : h->shards) c->nprobe = nprobe_override; }
    }
    ~SelScope() {
        h->sel = nullptr;
        for (auto* c : h->shards) c->sel = nullptr;
        if (np_set) { h->nprobe = nprobe0; for (auto* c : h->shards) c->nprobe = nprobe0; }
    }
};

// faiss.IndexPQ handles (rsx_index::flat_pq) have no coarse quantiser, no selectors and no removal
static void refuse_flat_pq(const rsx_index* h, int code, const char* what) {
    if (h && h->flat_pq) RSX_THROW(code, "%s: not available on an IndexPQ handle (a flat product quantiser: one list, no coarse quantiser)", what);
}

extern "C" {
static int search_prepass_common(rsx_index_t* h, int64_t nq, const void* q, int dtype, int k, const rsx_selector* sel, int nprobe_override,
                                 float* D, int64_t* I, uint64_t** tau_dev, int64_t* ntau) {
    return guarded([&] {
        if (!h || !tau_dev || !ntau) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        if (dtype != RSX_F32 && dtype != RSX_F16) RSX_THROW(RSX_ERR_INVALID, "bad dtype %d", dtype);
        if (nprobe_override < 0) RSX_THROW(RSX_ERR_INVALID, "nprobe override must be positive or 0 (got %d)", nprobe_override);
        if (sel) refuse_flat_pq(h, RSX_ERR_UNSUPPORTED, "search with a selector (FAISS 1.8.0 IndexPQ::search takes no search parameters)");
        refuse_ivfsq(h, "search_prepass (the two-call search)");
        if (is_sharded(h)) RSX_THROW(RSX_ERR_UNSUPPORTED, "search_prepass: not available on a sharded handle (its shards share one process)");
        if (nq > h->query_batch) RSX_THROW(RSX_ERR_UNSUPPORTED, "search_prepass: nq = %lld exceeds query_batch = %d (one internal batch per two-call search)", (long long)nq, h->query_batch);
        if (!h->tc) h->tc.reset(new rsx_index::TwoCall());
        rsx_index::TwoCall& t = *h->tc;
        if (t.active) RSX_THROW(RSX_ERR_INVALID, "search_prepass: the previous two-call search has not been finished with rsx_search_scan");
        t.active = true; t.parked = false; t.go = false; t.done = false; t.status = 0; t.err.clear(); t.tau = nullptr; t.ntau = 0;
        t.th = std::thread([h, nq, q, dtype, k, sel, nprobe_override, D, I] {
            rsx_index::TwoCall& tt = *h->tc;
            { std::lock_guard<std::mutex> lk(tt.mu); tt.worker = std::this_thread::get_id(); }
            int st_ = RSX_OK; std::string msg;
            try { HIPCHECK(hipSetDevice(h->device)); SelScope sc(h, sel, nprobe_override); search_impl(h, nq, q, dtype, k, D, I); }
            catch (const RsxError& e) { st_ = e.code; msg = e.what(); }
            catch (const std::exception& e) { st_ = RSX_ERR_INVALID; msg = e.what(); }
            std::lock_guard<std::mutex> lk(tt.mu);
            tt.status = st_; tt.err = msg; tt.done = true;
            tt.cv.notify_all();
        });
        std::unique_lock<std::mutex> lk(t.mu);
        t.cv.wait(lk, [&] { return t.parked || t.done; });
        *tau_dev = t.parked ? t.tau : nullptr;       // null: this search has no threshold pre-pass (Flat, exact paths, one probe, ...)
        *ntau = t.parked ? t.ntau : 0;
    });
}
}

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

const char* rsx_last_error(void) { return g_err.c_str(); }
int rsx_version(void) { return 1010; }     // 1010: rsx_merge_from, rsx_copy_subset_to (api_merge.hip); 1009: rsx_sq_create (api_sqflat.hip); 1008: rsx_vt_create, rsx_vt_set, rsx_vt_apply, rsx_vt_destroy (api_vt.hip); 1007: rsx_make_direct_map, rsx_reconstruct_batch; 1001: filtered search (rsx_selector_*, rsx_search_sel, rsx_search_prepass_sel); 1002: rsx_remove_ids; 1003: rsx_pq_create; 1004: rsx_refine; 1005: rsx_ivfsq_create; 1006: rsx_range_search, rsx_range_result_get, rsx_range_result_destroy

int rsx_device_count(int* n) {
    return guarded([&] {
        if (!n) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        int c = 0;
        hipError_t e = hipGetDeviceCount(&c);
        if (e != hipSuccess || c <= 0) { (void)hipGetLastError(); *n = 0; RSX_THROW(RSX_ERR_HIP, "no HIP device available: librsx has no CPU path"); }
        *n = c;
    });
}

int rsx_flat_create(int d, int metric, int device, rsx_index_t** out) {
    return guarded([&] { if (!out) RSX_THROW(RSX_ERR_INVALID, "null out"); *out = create_common(KIND_FLAT, d, 1, 0, 8, metric, device); });
}
int rsx_ivfflat_create(int d, int nlist, int metric, int device, rsx_index_t** out) {
    return guarded([&] { if (!out) RSX_THROW(RSX_ERR_INVALID, "null out"); *out = create_common(KIND_IVFFLAT, d, nlist, 0, 8, metric, device); });
}
int rsx_ivfpq_create(int d, int nlist, int M, int nbits, int metric, int device, rsx_index_t** out) {
    return guarded([&] { if (!out) RSX_THROW(RSX_ERR_INVALID, "null out"); *out = create_common(KIND_IVFPQ, d, nlist, M, nbits, metric, device); });
}
int rsx_pq_create(int d, int M, int nbits, int metric, int device, rsx_index_t** out) {
    return guarded([&] { if (!out) RSX_THROW(RSX_ERR_INVALID, "null out"); *out = create_flat_pq(d, M, nbits, metric, device); });
}
int rsx_ivfsq_create(int d, int nlist, int qtype, int metric, int by_residual, int device, rsx_index_t** out) {
    return guarded([&] { if (!out) RSX_THROW(RSX_ERR_INVALID, "null out"); *out = create_ivfsq(d, nlist, qtype, metric, by_residual, device); });
}
int rsx_sq_create(int d, int qtype, int metric, int device, rsx_index_t** out) {
    return guarded([&] { if (!out) RSX_THROW(RSX_ERR_INVALID, "null out"); *out = create_flat_sq(d, qtype, metric, device); });
}
int rsx_sharded_create(int kind, int d, int nlist, int M, int nbits, int metric, int ndev, const int* devices, rsx_index_t** out) {
    return guarded([&] {
        if (!out) RSX_THROW(RSX_ERR_INVALID, "null out");
        if (kind == RSX_KIND_IVFSQ) RSX_THROW(RSX_ERR_UNSUPPORTED, "sharded_create: IndexIVFScalarQuantizer (kind 4) has no sharded form in this build");
        if (kind == RSX_KIND_PQ) RSX_THROW(RSX_ERR_UNSUPPORTED, "sharded_create: IndexPQ (kind 3) has no sharded form in this build");
        if (kind == RSX_KIND_SQ) RSX_THROW(RSX_ERR_UNSUPPORTED, "sharded_create: IndexScalarQuantizer (kind 5) has no sharded form in this build");
        if (kind != KIND_FLAT && kind != KIND_IVFFLAT && kind != KIND_IVFPQ) RSX_THROW(RSX_ERR_INVALID, "unknown index kind %d", kind);
        *out = sharded_create(kind, d, nlist, M, nbits, metric, ndev, devices);
    });
}
int rsx_load_sharded(const char* path, int ndev, const int* devices, rsx_index_t** out) {
    return guarded([&] {
        if (!path || !out) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        *out = sharded_load(path, ndev, devices);
    });
}
int rsx_destroy(rsx_index_t* h) {
    return guarded([&] {
        if (!h) return;
        if (h->tc && h->tc->active) {       // an unfinished two-call search: let it run to the end before the handle goes away
            { std::lock_guard<std::mutex> lk(h->tc->mu); h->tc->go = true; }
            h->tc->cv.notify_all();
            if (h->tc->th.joinable()) h->tc->th.join();
        }
        for (auto* c : h->shards) {
            (void)hipSetDevice(c->device);
            if (c->st) { (void)hipStreamSynchronize(c->st); (void)hipStreamDestroy(c->st); }
            delete c;
        }
        h->shards.clear();
        (void)hipSetDevice(h->device);
            if (h->st) { (void)hipStreamSynchronize(h->st); (void)hipStreamDestroy(h->st); }
        delete h;
    });
}

int rsx_train(rsx_index_t* h, int64_t n, const void* x, int dtype) {
    return guarded([&] {
        if (!h || (!x && n > 0)) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "train");
        if (dtype != RSX_F32 && dtype != RSX_F16) RSX_THROW(RSX_ERR_INVALID, "bad dtype %d", dtype);
        if (is_sharded(h)) {     // train once on the first shard, copy the parameters to the others
            HIPCHECK(hipSetDevice(h->shards[0]->device));
            train_impl(h->shards[0], n, x, dtype);
            sharded_sync_trained(h);
            return;
        }
        use_device(h);
        train_impl(h, n, x, dtype);
    });
}
int rsx_set_centroids(rsx_index_t* h, const float* c) {
    return guarded([&] {
        if (!h || !c) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "set_centroids");
        refuse_flat_pq(h, RSX_ERR_INVALID, "set_centroids");
        refuse_flat_sq(h, RSX_ERR_INVALID, "set_centroids");
        if (h->kind == KIND_FLAT) RSX_THROW(RSX_ERR_INVALID, "Flat has no centroids");
        if (h->ntotal) RSX_THROW(RSX_ERR_INVALID, "cannot replace centroids of a populated index");
        if (is_sharded(h)) {
            for (auto* s : h->shards) { HIPCHECK(hipSetDevice(s->device)); set_centroids(s, c); update_trained(s); }
            h->trained = h->shards[0]->trained;
            return;
        }
        use_device(h); set_centroids(h, c); update_trained(h);
    });
}
int rsx_set_codebooks(rsx_index_t* h, const float* c) {
    return guarded([&] {
        if (!h || !c) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "set_codebooks");
        if (h->kind != KIND_IVFPQ) RSX_THROW(RSX_ERR_INVALID, "only IVFPQ has codebooks");
        if (h->ntotal) RSX_THROW(RSX_ERR_INVALID, "cannot replace codebooks of a populated index");
        if (is_sharded(h)) {
            for (auto* s : h->shards) { HIPCHECK(hipSetDevice(s->device)); set_codebooks(s, c); update_trained(s); }
            h->trained = h->shards[0]->trained;
            return;
        }
        use_device(h); set_codebooks(h, c); update_trained(h);
    });
}
int rsx_set_sq_trained(rsx_index_t* h, const float* t) {
    return guarded([&] {
        if (!h || !t) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "set_sq_trained");
        if (h->kind != KIND_IVFSQ) RSX_THROW(RSX_ERR_INVALID, "only an IndexIVFScalarQuantizer handle (kind 4) has scalar-quantiser parameters");
        if (h->ntotal) RSX_THROW(RSX_ERR_INVALID, "cannot replace the scalar-quantiser parameters of a populated index");
        use_device(h); set_sq_trained(h, t); update_trained(h);
    });
}
int rsx_get_sq_trained(rsx_index_t* h, float* out) {
    return guarded([&] {
        if (!h || !out) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        if (h->kind != KIND_IVFSQ) RSX_THROW(RSX_ERR_INVALID, "only an IndexIVFScalarQuantizer handle (kind 4) has scalar-quantiser parameters");
        if (h->h_sq.empty()) RSX_THROW(RSX_ERR_NOT_TRAINED, "no scalar-quantiser parameters");
        memcpy(out, h->h_sq.data(), h->h_sq.size() * 4);
    });
}
int rsx_get_centroids(rsx_index_t* h, float* out) {
    return guarded([&] {
        if (!h || !out) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_flat_pq(h, RSX_ERR_INVALID, "get_centroids");
        refuse_flat_sq(h, RSX_ERR_INVALID, "get_centroids");
        if (is_sharded(h)) h = h->shards[0];
        if (h->h_centroids.empty()) RSX_THROW(RSX_ERR_NOT_TRAINED, "no centroids");
        memcpy(out, h->h_centroids.data(), h->h_centroids.size() * 4);
    });
}
int rsx_get_codebooks(rsx_index_t* h, float* out) {
    return guarded([&] {
        if (!h || !out) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        if (is_sharded(h)) h = h->shards[0];
        if (h->h_codebooks.empty()) RSX_THROW(RSX_ERR_NOT_TRAINED, "no codebooks");
        memcpy(out, h->h_codebooks.data(), h->h_codebooks.size() * 4);
    });
}

int rsx_add(rsx_index_t* h, int64_t n, const void* x, int dtype, const int64_t* ids) {
    return guarded([&] {
        if (!h || (!x && n > 0)) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "add");
        if (dtype != RSX_F32 && dtype != RSX_F16) RSX_THROW(RSX_ERR_INVALID, "bad dtype %d", dtype);
        if (!h->trained) RSX_THROW(RSX_ERR_NOT_TRAINED, "add before train");
        if (ids) refuse_flat_pq(h, RSX_ERR_UNSUPPORTED, "add with ids (FAISS's IndexFlatCodes has no add_with_ids)");
        if (ids) refuse_flat_sq(h, RSX_ERR_UNSUPPORTED, "add with ids (FAISS's IndexFlatCodes has no add_with_ids)");
        if (n <= 0) return;
        if (is_sharded(h)) { sharded_add(h, n, x, dtype, ids); if (ids) h->ids_given = true; return; }
        use_device(h);
        add_all(h, n, x, dtype, ids);
        if (ids) h->ids_given = true;
    });
}
int rsx_assign(rsx_index_t* h, int64_t n, const void* x, int dtype, int64_t* labels) {
    return guarded([&] {
        if (!h || (!x && n > 0) || (!labels && n > 0)) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        if (dtype != RSX_F32 && dtype != RSX_F16) RSX_THROW(RSX_ERR_INVALID, "bad dtype %d", dtype);
        if (h->kind == KIND_FLAT) RSX_THROW(RSX_ERR_INVALID, "Flat has no coarse quantiser");
        refuse_while_two_call(h, "assign");
        refuse_flat_pq(h, RSX_ERR_INVALID, "assign");
        refuse_flat_sq(h, RSX_ERR_INVALID, "assign");
        if (is_sharded(h)) h = h->shards[0];
        if (h->h_centroids.empty()) RSX_THROW(RSX_ERR_NOT_TRAINED, "assign before train");
        use_device(h);
        const int64_t B = 262144;
        size_t esz = dtype == RSX_F16 ? 2 : 4;
        int ct = (h->nlist + 127) / 128;
        bool out_dev = is_device_ptr(labels);
        std::vector<int32_t> a32; std::vector<int64_t> a64;
        for (int64_t i0 = 0; i0 < n; i0 += B) {
            int64_t nb = std::min(B, n - i0);
            const void* dx = stage_rows(h, h->w_x, (const char*)x + (size_t)i0 * h->d * esz, nb, h->d, dtype);
            h->w_partial.ensure((size_t)nb * 2 * ct * 8);
            h->w_assign.ensure((size_t)nb * 4);
            launch_gemm_exact_argmax(dx, dtype == RSX_F16, nb, h->d, h->d_centroids.as<float>(), h->nlist, h->d,
                                     h->w_partial.as<uint64_t>(), h->w_assign.as<int32_t>(), nullptr, h->st);
            a32.resize((size_t)nb); a64.resize((size_t)nb);
            HIPCHECK(hipMemcpyAsync(a32.data(), h->w_assign.p, (size_t)nb * 4, hipMemcpyDeviceToHost, h->st));
            HIPCHECK(hipStreamSynchronize(h->st));
            for (int64_t i = 0; i < nb; i++) a64[(size_t)i] = a32[(size_t)i];
            HIPCHECK(hipMemcpy(labels + i0, a64.data(), (size_t)nb * 8, out_dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
        }
    });
}
int rsx_reset(rsx_index_t* h) {
    return guarded([&] {
        if (!h) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "reset");
        if (is_sharded(h)) {
            for (auto* s : h->shards) {
                HIPCHECK(hipSetDevice(s->device));
                HIPCHECK(hipStreamSynchronize(s->st));
                std::fill(s->h_len.begin(), s->h_len.end(), 0);
                s->ntotal = 0; s->ndropped = 0;
                if (s->d_len.p) upload_dir(s);
            }
            h->ntotal = 0; h->sh_next_id = 0; h->ids_given = false;
            return;
        }
        use_device(h);
        HIPCHECK(hipStreamSynchronize(h->st));
        std::fill(h->h_len.begin(), h->h_len.end(), 0);
        h->ntotal = 0; h->ndropped = 0; h->ids_given = false;
        if (h->d_len.p) upload_dir(h);
    });
}
int rsx_reserve_lists(rsx_index_t* h, const int64_t* counts) {
    return guarded([&] {
        if (!h || !counts) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "reserve_lists");
        refuse_flat_pq(h, RSX_ERR_INVALID, "reserve_lists");
        refuse_flat_sq(h, RSX_ERR_INVALID, "reserve_lists");
        if (is_sharded(h)) { sharded_reserve(h, counts); return; }
        use_device(h);
        std::vector<int64_t> need(counts, counts + h->nlist);
        for (int l = 0; l < h->nlist; l++) need[(size_t)l] = std::max(need[(size_t)l], h->h_len[(size_t)l]);
        ensure_capacity(h, need, true);
    });
}
int rsx_add_list(rsx_index_t* h, int64_t list_no, int64_t n, const void* codes, int dtype, const int64_t* ids) {
    return guarded([&] {
        if (!h || (!codes && n > 0)) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "add_list");
        if (is_sharded(h)) {
            if (!h->trained) RSX_THROW(RSX_ERR_NOT_TRAINED, "add_list before train");
            if (list_no < 0 || list_no >= h->nlist) RSX_THROW(RSX_ERR_INVALID, "list %lld out of range", (long long)list_no);
            sharded_add_list(h, list_no, n, codes, dtype, ids);
            return;
        }
        use_device(h);
        add_list_impl(h, list_no, n, codes, dtype, ids);
    });
}
int rsx_get_list(rsx_index_t* h, int64_t list_no, int64_t* n_out, void* codes_out, int64_t* ids_out) {
    return guarded([&] {
        if (!h) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        if (is_sharded(h)) RSX_THROW(RSX_ERR_UNSUPPORTED, "get_list: not available on a sharded handle (the lists are split over the shards)");
        use_device(h);
        get_list_impl(h, list_no, n_out, codes_out, ids_out);
    });
}

int rsx_get_list_sizes(rsx_index_t* h, int64_t* sizes) {
    return guarded([&] {
        if (!h || !sizes) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        if (is_sharded(h)) {
            for (int l = 0; l < h->nlist; l++) { sizes[l] = 0; for (auto* s : h->shards) sizes[l] += s->h_len[(size_t)l]; }
            return;
        }
        for (int l = 0; l < h->nlist; l++) sizes[l] = h->h_len[(size_t)l];
    });
}

int rsx_set_nprobe(rsx_index_t* h, int nprobe) {
    return guarded([&] {
        if (!h) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "set_nprobe");
        refuse_flat_pq(h, RSX_ERR_INVALID, "set_nprobe");
        refuse_flat_sq(h, RSX_ERR_INVALID, "set_nprobe");
        if (nprobe <= 0) RSX_THROW(RSX_ERR_INVALID, "nprobe must be positive (got %d)", nprobe);
        // FAISS accepts any nprobe and probes min(nprobe, nlist) lists; the effective value is bounded at search time
        h->nprobe = nprobe;
        for (auto* s : h->shards) s->nprobe = nprobe;
    });
}

int rsx_search(rsx_index_t* h, int64_t nq, const void* q, int dtype, int k, float* D, int64_t* I) {
    return guarded([&] {
        if (!h) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "search");
        if (dtype != RSX_F32 && dtype != RSX_F16) RSX_THROW(RSX_ERR_INVALID, "bad dtype %d", dtype);
        if (is_sharded(h)) {
            if (!h->trained) RSX_THROW(RSX_ERR_NOT_TRAINED, "search before train");
            sharded_search(h, nq, q, dtype, k, D, I);
            return;
        }
        use_device(h);
        if (h->flat_sq) sqflat_search(h, nq, q, dtype, k, D, I); else search_impl(h, nq, q, dtype, k, D, I);
    });
}
int rsx_search_sel(rsx_index_t* h, int64_t nq, const void* q, int dtype, int k, const rsx_selector_t* sel, int nprobe_override,
                   float* D, int64_t* I) {
    return guarded([&] {
        if (!h) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "search");
        if (dtype != RSX_F32 && dtype != RSX_F16) RSX_THROW(RSX_ERR_INVALID, "bad dtype %d", dtype);
        if (nprobe_override < 0) RSX_THROW(RSX_ERR_INVALID, "nprobe override must be positive or 0 (got %d)", nprobe_override);
        if (sel) refuse_flat_pq(h, RSX_ERR_UNSUPPORTED, "search with a selector (FAISS 1.8.0 IndexPQ::search takes no search parameters)");
        if (sel) refuse_ivfsq(h, "search with a selector");
        SelScope sc(h, sel, (h->flat_pq || h->flat_sq) ? 0 : nprobe_override);
        if (is_sharded(h)) {
            if (!h->trained) RSX_THROW(RSX_ERR_NOT_TRAINED, "search before train");
            sharded_search(h, nq, q, dtype, k, D, I);
            return;
        }
        use_device(h);
        if (h->flat_sq) sqflat_search(h, nq, q, dtype, k, D, I); else search_impl(h, nq, q, dtype, k, D, I);
    });
}

int rsx_refine(rsx_index_t* h, int64_t nq, const void* q, int dtype, int kc, const int64_t* labels, int k, float* D, int64_t* I) {
    return guarded([&] {
        if (!h) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "refine");
        if (dtype != RSX_F32 && dtype != RSX_F16) RSX_THROW(RSX_ERR_INVALID, "bad dtype %d", dtype);
        if (public_kind(h) != RSX_KIND_FLAT) RSX_THROW(RSX_ERR_INVALID, "refine: the handle must be a Flat index (its kind is %d): the labels name stored rows", public_kind(h));
        if (is_sharded(h)) RSX_THROW(RSX_ERR_UNSUPPORTED, "refine: not available on a sharded handle (the rows are split over the shards)");
        if (h->custom_ids) RSX_THROW(RSX_ERR_UNSUPPORTED, "refine: not available on a Flat handle with explicit ids (labels are positions, as in FAISS's IndexRefineFlat)");
        if (nq < 0) RSX_THROW(RSX_ERR_INVALID, "refine: nq = %lld", (long long)nq);
        if (kc > 4096) RSX_THROW(RSX_ERR_UNSUPPORTED, "refine: kc = %d exceeds this build's maximum of 4096 candidates per query", kc);
        if (k < 1 || k > kc) RSX_THROW(RSX_ERR_INVALID, "refine: k = %d must lie in [1, kc = %d]", k, kc);
        use_device(h);
        refine_impl(h, nq, q, dtype, kc, labels, k, D, I);
    });
}

int rsx_make_direct_map(rsx_index_t* h, int type) {
    return guarded([&] {
        if (!h) RSX_THROW(RSX_ERR_INVALID, "make_direct_map: null pointer");
        refuse_while_two_call(h, "make_direct_map");
        if (is_sharded(h)) RSX_THROW(RSX_ERR_UNSUPPORTED, "make_direct_map: not available on a sharded handle (the rows are split over the shards)");
        use_device(h);
        make_direct_map_impl(h, type);
    });
}
int rsx_reconstruct_batch(rsx_index_t* h, int64_t n, const int64_t* keys, int fill_negative, float* out) {
    return guarded([&] {
        if (!h) RSX_THROW(RSX_ERR_INVALID, "reconstruct_batch: null pointer");
        refuse_while_two_call(h, "reconstruct_batch");
        if (is_sharded(h)) RSX_THROW(RSX_ERR_UNSUPPORTED, "reconstruct_batch: not available on a sharded handle (the rows are split over the shards)");
        if (n < 0) RSX_THROW(RSX_ERR_INVALID, "reconstruct_batch: n = %lld", (long long)n);
        if (n > 0 && (!keys || !out)) RSX_THROW(RSX_ERR_INVALID, "reconstruct_batch: null pointer with n = %lld", (long long)n);
        use_device(h);
        reconstruct_impl(h, n, keys, fill_negative, out);
    });
}

int rsx_range_search(rsx_index_t* h, int64_t nq, const void* q, int dtype, float radius, int nprobe_override, rsx_range_result_t** out) {
    return guarded([&] {
        if (!h || !out) RSX_THROW(RSX_ERR_INVALID, "range_search: null pointer");
        *out = nullptr;
        refuse_while_two_call(h, "range_search");
        if (dtype != RSX_F32 && dtype != RSX_F16) RSX_THROW(RSX_ERR_INVALID, "range_search: bad dtype %d", dtype);
        if (nprobe_override < 0) RSX_THROW(RSX_ERR_INVALID, "range_search: nprobe override must be positive or 0 (got %d)", nprobe_override);
        if (is_sharded(h)) RSX_THROW(RSX_ERR_UNSUPPORTED, "range_search: not available on a sharded handle in this build");
        refuse_ivfsq(h, "range_search");
        if (public_kind(h) != RSX_KIND_FLAT && public_kind(h) != RSX_KIND_IVFFLAT)
            RSX_THROW(RSX_ERR_UNSUPPORTED, "range_search: available on Flat and IVF-Flat handles only in this build (this handle's kind is %d)", public_kind(h));
        use_device(h);
        SelScope sc(h, nullptr, h->kind == KIND_IVFFLAT ? nprobe_override : 0);
        *out = range_impl(h, nq, q, dtype, radius);
    });
}
int rsx_range_result_get(const rsx_range_result_t* r, int64_t* nq, int64_t* total, int* on_device, const int64_t** lims, const float** D, const int64_t** I) {
    return guarded([&] {
        if (!r) RSX_THROW(RSX_ERR_INVALID, "range_result_get: null result");
        if (nq) *nq = r->nq;
        if (total) *total = r->total;
        if (on_device) *on_device = r->on_device;
        if (lims) *lims = r->on_device ? r->d_lims->as<int64_t>() : r->h_lims.data();
        if (D) *D = r->on_device ? (r->d_D ? r->d_D->as<float>() : nullptr) : r->h_D.data();
        if (I) *I = r->on_device ? (r->d_I ? r->d_I->as<int64_t>() : nullptr) : r->h_I.data();
    });
}
int rsx_range_result_destroy(rsx_range_result_t* r) {
    return guarded([&] {
        if (!r) return;
        int prev = -1;
        if (r->on_device && hipGetDevice(&prev) == hipSuccess && prev != r->device) (void)hipSetDevice(r->device); else prev = -1;
        delete r;
        if (prev >= 0) (void)hipSetDevice(prev);      // the caller's current device is left as it was
    });
}

int rsx_remove_ids(rsx_index_t* h, const rsx_selector_t* sel, int64_t* nremoved) {
    return guarded([&] {
        if (!h || !sel || !nremoved) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "remove_ids");
        refuse_flat_pq(h, RSX_ERR_UNSUPPORTED, "remove_ids");
        refuse_ivfsq(h, "remove_ids");
        *nremoved = 0;
        if (is_sharded(h)) { *nremoved = sharded_remove(h, sel); return; }
        use_device(h);
        *nremoved = remove_impl(h, sel);
    });
}

int rsx_merge_from(rsx_index_t* dst, rsx_index_t* src, int64_t add_id) {
    return guarded([&] { merge_from_impl(dst, src, add_id); });
}
int rsx_copy_subset_to(rsx_index_t* src, rsx_index_t* dst, int subset_type, int64_t a1, int64_t a2) {
    return guarded([&] { copy_subset_impl(src, dst, subset_type, a1, a2); });
}

static std::atomic<uint64_t> g_sel_serial{0};
int rsx_selector_create(int kind, const void* data, int64_t n, int64_t lo, int64_t hi, int invert, rsx_selector_t** out) {
    return guarded([&] {
        if (!out) RSX_THROW(RSX_ERR_INVALID, "null out");
        if (kind != RSX_SEL_RANGE && kind != RSX_SEL_BATCH && kind != RSX_SEL_BITMAP) RSX_THROW(RSX_ERR_INVALID, "unknown selector kind %d", kind);
        if (n < 0 || (kind != RSX_SEL_RANGE && n > 0 && !data)) RSX_THROW(RSX_ERR_INVALID, "selector: n = %lld with data %p", (long long)n, data);
        std::unique_ptr<rsx_selector> s(new rsx_selector());
        s->kind = kind; s->invert = invert != 0;
        if (kind == RSX_SEL_RANGE) { s->lo = lo; s->hi = hi; }
        else {
            const size_t bytes = (size_t)n * (kind == RSX_SEL_BATCH ? 8 : 1);
            std::vector<uint8_t> raw(bytes);
            if (bytes) {
                if (is_device_ptr(data)) HIPCHECK(hipMemcpy(raw.data(), data, bytes, hipMemcpyDeviceToHost));
                else memcpy(raw.data(), data, bytes);
            }
            if (kind == RSX_SEL_BITMAP) s->bitmap.swap(raw);
            else {
                s->ids.resize((size_t)n);
                if (bytes) memcpy(s->ids.data(), raw.data(), bytes);
                std::sort(s->ids.begin(), s->ids.end());
                s->ids.erase(std::unique(s->ids.begin(), s->ids.end()), s->ids.end());
            }
        }
        s->serial = ++g_sel_serial;
        *out = s.release();
    });
}
int rsx_selector_destroy(rsx_selector_t* sel) {
    return guarded([&] { delete sel; });
}
int rsx_selector_is_member(const rsx_selector_t* sel, int64_t n, const int64_t* ids, uint8_t* out) {
    return guarded([&] {
        if (!sel || n < 0 || (n > 0 && (!ids || !out))) RSX_THROW(RSX_ERR_INVALID, "selector is_member: bad arguments");
        for (int64_t i = 0; i < n; i++) out[i] = sel->contains(ids[i]) ? 1 : 0;
    });
}

int rsx_search_prepass(rsx_index_t* h, int64_t nq, const void* q, int dtype, int k, float* D, int64_t* I, uint64_t** tau_dev,
                       int64_t* ntau) {
    return search_prepass_common(h, nq, q, dtype, k, nullptr, 0, D, I, tau_dev, ntau);
}
int rsx_search_prepass_sel(rsx_index_t* h, int64_t nq, const void* q, int dtype, int k, const rsx_selector_t* sel, int nprobe_override,
                           float* D, int64_t* I, uint64_t** tau_dev, int64_t* ntau) {
    return search_prepass_common(h, nq, q, dtype, k, sel, nprobe_override, D, I, tau_dev, ntau);
}
int rsx_search_scan(rsx_index_t* h) {
    return guarded([&] {
        if (!h || !h->tc || !h->tc->active) RSX_THROW(RSX_ERR_INVALID, "search_scan without rsx_search_prepass");
        rsx_index::TwoCall& t = *h->tc;
        { std::lock_guard<std::mutex> lk(t.mu); t.go = true; }
        t.cv.notify_all();
        t.th.join();
        t.active = false;
        if (t.status != RSX_OK) throw RsxError(t.status, t.err);
    });
}

int rsx_merge_topk(int nshards, int64_t nq, int k, int metric, const float* D, const int64_t* I, float* Do, int64_t* Io,
                   int device) {
    return guarded([&] {
        if (nshards <= 0 || nq < 0 || k <= 0 || !D || !I || !Do || !Io) RSX_THROW(RSX_ERR_INVALID, "merge_topk: bad arguments");
        // one launch holds nshards x k <= 16384 keys; beyond that the merge runs in rounds over groups of blocks, which need k <= 8192 (ADVICE r5:
        // the pre-check used to refuse every k > 8192, also nshards = 1 with k = 16384, which one launch handles)
        if (k > 8192 && (int64_t)nshards * k > 16384) RSX_THROW(RSX_ERR_UNSUPPORTED, "merge_topk: %d shards x k = %d: more than 16384 keys per query need k <= 8192", nshards, k);
        if (nq == 0) return;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); RSX_THROW(RSX_ERR_HIP, "no HIP device available: librsx has no CPU path"); }
        HIPCHECK(hipSetDevice(device));
        bool dev = is_device_ptr(D);
        size_t nin = (size_t)nshards * nq * k, nout = (size_t)nq * k;
        if (dev) {
            if (!launch_merge_topk(nshards, nq, k, metric, D, I, Do, Io, nullptr)) RSX_THROW(RSX_ERR_OOM, "merge_topk: no memory for the round buffers");
            HIPCHECK(hipStreamSynchronize(nullptr));
        } else {
            DevBuf a, b, c, e;
            a.ensure(nin * 4); b.ensure(nin * 8); c.ensure(nout * 4); e.ensure(nout * 8);
            HIPCHECK(hipMemcpy(a.p, D, nin * 4, hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(b.p, I, nin * 8, hipMemcpyHostToDevice));
            if (!launch_merge_topk(nshards, nq, k, metric, a.as<float>(), b.as<int64_t>(), c.as<float>(), e.as<int64_t>(), nullptr))
                RSX_THROW(RSX_ERR_OOM, "merge_topk: no memory for the round buffers");
            HIPCHECK(hipMemcpy(Do, c.p, nout * 4, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(Io, e.p, nout * 8, hipMemcpyDeviceToHost));
        }
        HIPCHECK(hipGetLastError());
    });
}

int rsx_pack_topk(int64_t nq, int k, const float* D, const int64_t* I, int64_t id_offset, int64_t* packed, int device,
                  void* stream) {
    return guarded([&] {
        if (nq < 0 || k <= 0 || !D || !I || !packed) RSX_THROW(RSX_ERR_INVALID, "pack_topk: bad arguments");
        if (nq == 0) return;
        if (!is_device_ptr(D) || !is_device_ptr(I) || !is_device_ptr(packed)) RSX_THROW(RSX_ERR_INVALID, "pack_topk: device pointers only");
        HIPCHECK(hipSetDevice(device));
        launch_pack_topk(nq * k, D, I, id_offset, packed, (hipStream_t)stream);
        HIPCHECK(hipGetLastError());
    });
}

int rsx_merge_packed(int nshards, int64_t nq, int k, int metric, const int64_t* packed, float* Do, int64_t* Io, int device,
                     void* stream) {
    return guarded([&] {
        if (nshards <= 0 || nq < 0 || k <= 0 || !packed || !Do || !Io) RSX_THROW(RSX_ERR_INVALID, "merge_packed: bad arguments");
        if (k > 8192 && (int64_t)nshards * k > 16384) RSX_THROW(RSX_ERR_UNSUPPORTED, "merge_packed: %d shards x k = %d: more than 16384 keys per query need k <= 8192", nshards, k);
        if (nq == 0) return;
        if (!is_device_ptr(packed) || !is_device_ptr(Do) || !is_device_ptr(Io)) RSX_THROW(RSX_ERR_INVALID, "merge_packed: device pointers only");
        HIPCHECK(hipSetDevice(device));
        if (!launch_merge_packed(nshards, nq, k, metric, packed, Do, Io, (hipStream_t)stream)) RSX_THROW(RSX_ERR_OOM, "merge_packed: no memory for the round buffers");
        HIPCHECK(hipGetLastError());
    });
}

int rsx_get(rsx_index_t* h, const char* key, int64_t* out) {
    return guarded([&] {
        if (!h || !key || !out) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        std::string s(key);
        if (s == "nshards") { *out = (int64_t)h->shards.size(); return; }
        if (s == "direct_map_type") { *out = (!is_sharded(h) && h->dmap_type != 0 && h->dmap_gen == h->dir_gen) ? h->dmap_type : 0; return; }
        if (s == "explicit_ids") { *out = (h->ids_given || (h->kind == KIND_FLAT && h->custom_ids)) ? 1 : 0; return; }
        if (is_sharded(h)) {
            if (s == "ntotal") { *out = h->ntotal; return; }
            if (s == "nprobe") { *out = h->nprobe; return; }
            if (s == "is_trained") { *out = h->trained; return; }
            if (s == "hbm_bytes") { *out = 0; for (auto* c : h->shards) *out += (int64_t)(c->data.bytes + c->ids.bytes + c->norms.bytes); return; }
            if (s == "workspace_bytes") { *out = 0; for (auto* c : h->shards) *out += workspace_bytes(c); return; }
            if (s == "storage_dtype" && h->kind != KIND_IVFPQ) {     // fp32 as soon as ANY shard had to widen its rows
                *out = RSX_F16;
                for (auto* c : h->shards) if (!c->storage_f16) *out = RSX_F32;
                return;
            }
            h = h->shards[0];
        }
        if (s == "ntotal") *out = h->ntotal;
        else if (s == "nlist") *out = h->nlist;
        else if (s == "d") *out = h->d;
        else if (s == "is_trained") *out = h->trained;
        else if (s == "nprobe") *out = h->nprobe;
        else if (s == "M") *out = h->M;
        else if (s == "nbits") *out = h->nbits;
        else if (s == "kind") *out = public_kind(h);
        else if (s == "metric") *out = h->metric;
        else if (s == "storage_dtype") *out = (h->kind == KIND_IVFPQ || h->kind == KIND_IVFSQ) ? -1 : (h->storage_f16 ? RSX_F16 : RSX_F32);
        else if (s == "code_size") *out = (h->kind == KIND_IVFPQ) ? h->M : (h->kind == KIND_IVFSQ) ? h->d : (int64_t)h->d * (h->storage_f16 ? 2 : 4);
        else if (s == "qtype" && h->kind == KIND_IVFSQ) *out = h->sq_qtype;
        else if (s == "by_residual" && h->kind == KIND_IVFSQ) *out = h->by_residual ? 1 : 0;
        else if (s == "device") *out = h->device;
        else if (s == "max_k") *out = 4096;
        else if (s == "query_batch") *out = h->query_batch;
        else if (s == "pq_layout") *out = h->kind != KIND_IVFPQ ? 0 : h->CB == 0 ? 1 : h->CB == PQ_SLICED ? 2 : 0;
        else if (s == "hbm_bytes") *out = (int64_t)(h->data.bytes + h->ids.bytes + h->norms.bytes);
        else if (s == "workspace_bytes") *out = workspace_bytes(h);
        else RSX_THROW(RSX_ERR_INVALID, "unknown property '%s'", key);
    });
}
int rsx_set_param(rsx_index_t* h, const char* key, double value) {
    return guarded([&] {
        if (!h || !key) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "set_param");
        std::string s(key);
        if (is_sharded(h)) {     // knobs apply to every shard
            for (auto* c : h->shards) { int st_ = rsx_set_param(c, key, value); if (st_ != RSX_OK) throw RsxError(st_, g_err); }
            return;
        }
        if (s == "query_batch") h->query_batch = std::max(1, (int)value);
        else if (s == "scan_chunk") { refuse_ivfsq(h, "scan_chunk (the code-row scan has its own work items)"); h->scan_chunk = std::max(0, (int)value); }
        else if (s == "scan_kernel") h->scan_kernel = (int)value;
        else if (s == "pq_fast") h->pq_fast = (int)value;
        else if (s == "pq_fast_kp") h->pq_fast_kp = std::min(4096, std::max(0, (int)value));     // k_finalize sorts K' <= 4096 candidates in LDS
        else if (s == "pq_filter") h->pq_filter = (int)value;
        else if (s == "pq_prune") h->pq_prune = (int)value;
        else if (s == "pq_q8") h->pq_q8 = (int)value;
        else if (s == "pq_pace") h->pq_pace = std::max(0, (int)value);
        else if (s == "add_list_mod" || s == "add_list_rem") {
            if (h->kind == KIND_FLAT) RSX_THROW(RSX_ERR_UNSUPPORTED, "%s: IVF indexes only", key);
            refuse_flat_pq(h, RSX_ERR_INVALID, key);
            refuse_flat_sq(h, RSX_ERR_INVALID, key);
            if (h->ntotal + h->ndropped > 0) RSX_THROW(RSX_ERR_INVALID, "%s must be set before the first add", key);
            if (s == "add_list_mod") { if (value < 1) RSX_THROW(RSX_ERR_INVALID, "add_list_mod >= 1"); h->add_list_mod = (int)value; h->add_list_rem = 0; }
            else { if (value < 0 || value >= h->add_list_mod) RSX_THROW(RSX_ERR_INVALID, "0 <= add_list_rem < add_list_mod"); h->add_list_rem = (int)value; }
        }
        else if (s == "pq_layout") {
            if (h->kind != KIND_IVFPQ) RSX_THROW(RSX_ERR_UNSUPPORTED, "pq_layout: IVFPQ only");
            if (h->ntotal + h->ndropped > 0) RSX_THROW(RSX_ERR_INVALID, "pq_layout must be set before the first add");
            if ((int)value == 1 && !pq_rot_applies(h->M)) RSX_THROW(RSX_ERR_UNSUPPORTED, "pq_layout=1 (rotated) needs M in {16, 32, 64, 96, 128}");
            if ((int)value == 2 && !pq_sliced_applies(h->M)) RSX_THROW(RSX_ERR_UNSUPPORTED, "pq_layout=2 (sliced) needs M = 96");
            h->CB = (int)value == 1 ? 0 : (int)value == 2 ? PQ_SLICED : h->CB_granule;
        }
        else if (s == "ivf_filter") h->ivf_filter = (int)value;
        else if (s == "ivf_pre_lists") h->ivf_pre_lists = std::max(0, (int)value);
        else if (s == "ivf_pre_mult") h->ivf_pre_mult = std::max(1, (int)value);
        else if (s == "pq_pre_rows") h->pq_pre_rows = (int)value;
        else if (s == "pq_tau_anchor") h->pq_tau_anchor = (int)value;
        else if (s == "pq_flat_first") h->pq_flat_first = std::max(0, (int)value);
        else if (s == "pq_flat_growth") h->pq_flat_growth = std::max(0, (int)value);
        else if (s == "pq_flat_max_stages") h->pq_flat_max_stages = std::min(64, std::max(0, (int)value));
        else if (s == "pq_log_cap") h->pq_log_cap = std::max(0, (int)value);
        else if (s == "pq_pre_mult") h->pq_pre_mult = std::max(1, (int)value);
        else if (s == "pq_pre_max") h->pq_pre_max = std::min(32768, std::max(64, (int)value));
        else if (s == "pq_final_tab") h->pq_final_tab = (int)value;
        else if (s == "pq_gather") h->pq_gather = (int)value;
        else if (s == "pq_plain_codes") h->pq_plain_codes = (int)value;
        else if (s == "pq_prepass4") h->pq_prepass4 = (int)value;
        else if (s == "ivf_qtiles") h->ivf_qtiles = (int)value;
        else if (s == "pq_prepass_fused") h->pq_prepass_fused = (int)value;
        else if (s == "lut_tiled") h->lut_tiled = (int)value;
        else if (s == "pq_group_fused") h->pq_group_fused = (int)value;
        else if (s == "coarse_fast") h->coarse_fast = (int)value;
        else if (s == "pq_lut_early") h->pq_lut_early = (int)value;
        else if (s == "flat_filter") h->flat_filter = (int)value;
        else if (s == "flat_pre_mult") h->flat_pre_mult = std::max(1, (int)value);
        else if (s == "flat_pre_unit") h->flat_pre_unit = std::max(0, (int)value);
        else if (s == "ivf_overflow_max") h->ivf_overflow_max = std::max(0, (int)value);
        else if (s == "flat_stages") h->flat_stages = std::max(0, (int)value);
        else if (s == "flat_cert") h->flat_cert = (int)value;
        else if (s == "sqflat_cand_cap") {
            if (!h->flat_sq) RSX_THROW(RSX_ERR_UNSUPPORTED, "sqflat_cand_cap: IndexScalarQuantizer (kind 5) only");
            h->sqflat_cand_cap = std::max(0, (int)value);
        }
        else if (s == "range_cand_cap") h->range_cand_cap = std::max(0, (int)value);
        else if (s == "profile") { h->profile = (int)value; h->timing.clear(); }
        else if (s == "temp_budget_mb") h->temp_budget = (int64_t)value << 20;
        else RSX_THROW(RSX_ERR_INVALID, "unknown parameter '%s'", key);
    });
}
int rsx_get_timing(rsx_index_t* h, const char* key, double* ms) {
    return guarded([&] {
        if (!h || !key || !ms) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        if (is_sharded(h)) {     // stage times: the slowest shard; counters: the sum
            *ms = 0.0;
            const std::string ks(key);
            const bool sum = ks.find("queries") != std::string::npos || ks.find("launches") != std::string::npos || ks.find("vectors") != std::string::npos || ks == "removed";
            for (auto* c : h->shards) { auto it = c->timing.find(key); double v = it == c->timing.end() ? 0.0 : it->second; *ms = sum ? *ms + v : std::max(*ms, v); }
            return;
        }
        auto it = h->timing.find(key);
        *ms = (it == h->timing.end()) ? 0.0 : it->second;
    });
}

int rsx_save(rsx_index_t* h, const char* path) {
    return guarded([&] {
        if (!h || !path) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        refuse_while_two_call(h, "save");
        if (is_sharded(h)) { sharded_save(h, path); return; }
        use_device(h);
        save_impl(h, path);
    });
}
int rsx_load(const char* path, int device, rsx_index_t** out) {
    return guarded([&] {
        if (!path || !out) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        *out = load_impl(path, device);
    });
}

int rsx_synth_vectors(int device, int d, int ncentres, uint32_t seed_c, uint32_t seed_x, float sigma, int64_t i0,
                      int64_t n, void* out) {
    return guarded([&] {
        if (!out || d <= 0 || ncentres <= 0 || n < 0) RSX_THROW(RSX_ERR_INVALID, "synth_vectors: bad arguments");
        HIPCHECK(hipSetDevice(device));
        if (is_device_ptr(out)) {
            launch_synth_vectors(d, ncentres, seed_c, seed_x, sigma, i0, n, (__half*)out, nullptr);
            HIPCHECK(hipStreamSynchronize(nullptr));
        } else {
            DevBuf t; t.ensure((size_t)n * d * 2);
            launch_synth_vectors(d, ncentres, seed_c, seed_x, sigma, i0, n, t.as<__half>(), nullptr);
            HIPCHECK(hipMemcpy(out, t.p, (size_t)n * d * 2, hipMemcpyDeviceToHost));
        }
        HIPCHECK(hipGetLastError());
    });
}
int rsx_synth_queries(int device, int d, int ncentres, uint32_t seed_c, uint32_t seed_x, float sigma, int64_t nbase,
                      uint32_t seed_q, float sigma_q, int64_t r0, int64_t n, void* out) {
    return guarded([&] {
        if (!out || d <= 0 || ncentres <= 0 || n < 0 || nbase <= 0) RSX_THROW(RSX_ERR_INVALID, "synth_queries: bad arguments");
        HIPCHECK(hipSetDevice(device));
        if (is_device_ptr(out)) {
            launch_synth_queries(d, ncentres, seed_c, seed_x, sigma, nbase, seed_q, sigma_q, r0, n, (__half*)out, nullptr);
            HIPCHECK(hipStreamSynchronize(nullptr));
        } else {
            DevBuf t; t.ensure((size_t)n * d * 2);
            launch_synth_queries(d, ncentres, seed_c, seed_x, sigma, nbase, seed_q, sigma_q, r0, n, t.as<__half>(), nullptr);
            HIPCHECK(hipMemcpy(out, t.p, (size_t)n * d * 2, hipMemcpyDeviceToHost));
        }
        HIPCHECK(hipGetLastError());
    });
}

}  // extern "C"

