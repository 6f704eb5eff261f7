// api_reconstruct.hip — rsx_reconstruct_batch / rsx_make_direct_map's host driver: the direct map (stored id -> storage row) and the
// gather-and-decode launches (k_reconstruct.hip; rsx_reconstruct.h).
#include <chrono>
#include "rsx_host.h"
#include "rsx_reconstruct.h"

// The map is derived data: every mutation of the directory (upload_dir: add, add_list, remove_ids, reset, re-layout) releases it, so a
// mutation that needs the memory finds it free, and the next lookup builds it again.
void release_direct_map(rsx_index* h) {
    h->dmap.release();
    h->dmap_type = DM_NONE; h->dmap_n = 0; h->dmap_gen = ~0ull;
}

// A Flat handle of sequential ids, an IndexPQ and an IndexScalarQuantizer handle store vector i in row i: the key is the row, checked against ntotal.
static inline bool needs_direct_map(const rsx_index* h) { return !(h->flat_pq || h->flat_sq || (h->kind == KIND_FLAT && !h->custom_ids)); }

static void dm_alloc(rsx_index* h, size_t bytes, const char* form) {
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t headroom = (size_t)64 << 20;      // what the call's staging buffers and the runtime may still ask for
    if (free_b < bytes + headroom)
        RSX_THROW(RSX_ERR_OOM, "direct map (%s): %zu bytes for %lld vectors do not fit the %zu bytes free on device %d", form, bytes, (long long)h->ntotal, free_b, h->device);
    h->dmap.release();
    HIPCHECK(hipMalloc(&h->dmap.p, bytes));       // exact: 8 B (Array) / 16 B per slot (Hashtable), no growth margin
    h->dmap.bytes = bytes;
}
static int dm_read_flag(rsx_index* h) {
    int f = 0;
    HIPCHECK(hipMemcpyAsync(&f, h->dmap_ws.p, sizeof(int), hipMemcpyDeviceToHost, h->st));
    HIPCHECK(hipStreamSynchronize(h->st));
    HIPCHECK(hipGetLastError());
    return f;
}

// Build the map of the current directory generation unless it exists: Array when the preference allows it and every stored id lies in
// [0, ntotal) once (one scatter pass decides), else Hashtable.  A failure (RSX_ERR_OOM) leaves the handle without a map and usable.
static void ensure_direct_map(rsx_index* h) {
    if (!needs_direct_map(h) || h->ntotal == 0) return;
    if (h->dmap_type != DM_NONE && h->dmap_gen == h->dir_gen) return;
    release_direct_map(h);
    const auto t0 = std::chrono::steady_clock::now();
    h->dmap_ws.ensure(16);
    int* flag = h->dmap_ws.as<int>();
    const int64_t* ids = h->ids.as<int64_t>();
    const int64_t *base = h->d_base.as<int64_t>(), *len = h->d_len.as<int64_t>();
    try {
        if (h->dmap_pref == DM_ARRAY) {
            dm_alloc(h, (size_t)h->ntotal * 8, "Array");
            HIPCHECK(hipMemsetAsync(h->dmap.p, 0xFF, h->dmap.bytes, h->st));
            HIPCHECK(hipMemsetAsync(flag, 0, sizeof(int), h->st));
            launch_dm_array_build(ids, base, len, h->nlist, h->total_cap, h->dmap.as<unsigned long long>(), h->ntotal, flag, h->st);
            if (dm_read_flag(h) == 0) { h->dmap_type = DM_ARRAY; h->dmap_n = h->ntotal; }
            else h->dmap.release();       // an id out of range or stored twice: the hash table serves every id set
        }
        if (h->dmap_type == DM_NONE) {
            const uint64_t cap = dm_hash_capacity(h->ntotal);
            dm_alloc(h, (size_t)cap * 16, "Hashtable");
            launch_dm_fill(h->dmap.as<unsigned long long>(), (int64_t)cap * 2, DM_EMPTY, DM_NO_ROW, h->st);
            HIPCHECK(hipMemsetAsync(flag, 0, sizeof(int), h->st));
            launch_dm_hash_build(ids, base, len, h->nlist, h->total_cap, h->dmap.as<unsigned long long>(), cap - 1, flag, h->st);
            if (dm_read_flag(h) != 0) RSX_THROW(RSX_ERR_UNSUPPORTED, "direct map: the index stores the id INT64_MIN, which the hash table cannot hold");
            h->dmap_type = DM_HASH; h->dmap_n = (int64_t)cap;
        }
    } catch (...) {
        release_direct_map(h);
        throw;
    }
    h->dmap_gen = h->dir_gen;
    h->timing["direct_map_builds"] += 1.0;
    h->timing["direct_map_ms"] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void make_direct_map_impl(rsx_index* h, int type) {
    if (type != DM_NONE && type != DM_ARRAY && type != DM_HASH) RSX_THROW(RSX_ERR_INVALID, "make_direct_map: unknown map type %d (0 = NoMap, 1 = Array, 2 = Hashtable)", type);
    if (type == DM_NONE) { release_direct_map(h); return; }
    if (type != h->dmap_pref) release_direct_map(h);
    h->dmap_pref = type;
    ensure_direct_map(h);
}

void reconstruct_impl(rsx_index* h, int64_t n, const int64_t* keys, int fill_negative, float* out) {
    if (n == 0) return;
    ensure_direct_map(h);
    const bool k_dev = is_device_ptr(keys), o_dev = is_device_ptr(out);
    const int d = h->d;
    h->w_rflag.host_mapped = true;
    h->w_rflag.ensure(sizeof(int));
    *h->w_rflag.as<int>() = 0;          // (no kernel of this handle is in flight: every call ends with a synchronisation of its stream)
    h->dmap_ws.ensure(16);
    unsigned long long* miss_first = h->dmap_ws.as<unsigned long long>() + 1;
    HIPCHECK(hipMemsetAsync(miss_first, 0xFF, 8, h->st));

    ReconArgs a{};
    a.d = d; a.ld = h->ld; a.fill_negative = fill_negative != 0;
    a.ntotal = h->ntotal;
    if (!needs_direct_map(h) || h->ntotal == 0) a.mode = RC_DIRECT;     // (an empty index: every key misses at the bounds check)
    else { a.mode = h->dmap_type == DM_ARRAY ? RC_ARRAY : RC_HASH; a.map = h->dmap.as<unsigned long long>(); a.map_n = h->dmap_n; }
    a.data = h->data.p;
    a.list_base = h->d_base.as<int64_t>(); a.nlist = h->nlist;
    if (h->kind == KIND_IVFPQ) {
        a.fmt = RC_PQ; a.M = h->M; a.Mpad = h->Mpad; a.CB = h->CB; a.dsub = d / h->M;
        a.codebooks = h->d_codebooks.as<float>();
        a.centroids = h->flat_pq ? nullptr : h->d_centroids.as<float>();      // IndexPQ: the codebook entries alone (a -0 stays -0)
    } else if (h->kind == KIND_IVFSQ) {
        a.fmt = RC_SQ; a.trained = h->d_sq.as<float>();
        a.centroids = h->by_residual ? h->d_centroids.as<float>() : nullptr;
    } else a.fmt = h->storage_f16 ? RC_ROWS_F16 : RC_ROWS_F32;
    a.miss_flag = h->w_rflag.as<int>(); a.miss_first = miss_first;

    // host keys / outputs are staged through the workspace in chunks of at most 64 MiB of output
    int64_t chunk = std::min<int64_t>(n, (int64_t)1 << 30);
    if (!o_dev) chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, ((int64_t)64 << 20) / ((int64_t)d * 4)));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t nb = std::min(chunk, n - i0);
        a.n = nb; a.pos0 = i0;
        a.keys = keys + i0;
        if (!k_dev) {
            h->w_rkeys.ensure((size_t)nb * 8);
            HIPCHECK(hipMemcpyAsync(h->w_rkeys.p, keys + i0, (size_t)nb * 8, hipMemcpyHostToDevice, h->st));
            a.keys = h->w_rkeys.as<int64_t>();
        }
        a.out = out + i0 * d;
        if (!o_dev) { h->w_rout.ensure((size_t)nb * d * 4); a.out = h->w_rout.as<float>(); }
        launch_reconstruct(a, h->st);
        if (!o_dev) HIPCHECK(hipMemcpyAsync(out + i0 * d, a.out, (size_t)nb * d * 4, hipMemcpyDeviceToHost, h->st));
        if (!k_dev || !o_dev) HIPCHECK(hipStreamSynchronize(h->st));     // the staging buffers serve the next chunk
    }
    HIPCHECK(hipStreamSynchronize(h->st));
    HIPCHECK(hipGetLastError());
    h->timing["reconstruct_calls"] += 1.0;
    h->timing["reconstruct_keys"] += (double)n;
    if (*h->w_rflag.as<int>() != 0) {
        unsigned long long pos = 0; int64_t key = 0;
        HIPCHECK(hipMemcpy(&pos, miss_first, 8, hipMemcpyDeviceToHost));
        if (pos < (unsigned long long)n) {
            if (k_dev) HIPCHECK(hipMemcpy(&key, keys + pos, 8, hipMemcpyDeviceToHost)); else key = keys[pos];
        }
        RSX_THROW(RSX_ERR_INVALID, "reconstruct_batch: key %lld (position %llu of %lld) is not stored in the index (the outputs are unspecified)",
                  (long long)key, pos, (long long)n);
    }
}
