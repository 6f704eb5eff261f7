// api_remove.hip — rsx_remove_ids (FAISS 1.8.0 Index::remove_ids): host orchestration of the removal kernels (k_remove.hip) on the
// handle's stream, and the fan-out over the shards of a single-process multi-GPU handle.  Shared declarations: rsx_host.h.
#include <chrono>
#include "rsx_host.h"

// exact device allocation (DevBuf::ensure adds 1/8 of headroom: the Flat staging buffer has a hard bound)
static void alloc_exact(DevBuf& b, size_t n) {
    b.release();
    HIPCHECK(hipMalloc(&b.p, std::max<size_t>(n, 16)));
    b.bytes = std::max<size_t>(n, 16);
}

// the selector's slot mask over `nslots` storage slots, in a buffer of the removal's own (the search's cached mask, h->sel_mask,
// is left alone: upload_dir bumps dir_gen afterwards, which invalidates it)
static void build_mask(rsx_index* h, const rsx_selector* s, const int64_t* slot_ids, int64_t nslots, DevBuf& mask, DevBuf& sel_dev) {
    alloc_exact(mask, (size_t)std::max<int64_t>(1, sel_mask_words(nslots)) * 4);
    SelDevArgs a{};
    a.kind = s->kind; a.invert = s->invert; a.lo = s->lo; a.hi = s->hi;
    const size_t bytes = s->kind == RSX_SEL_BITMAP ? s->bitmap.size() : s->kind == RSX_SEL_BATCH ? s->ids.size() * 8 : 0;
    if (bytes) {
        const void* src = s->kind == RSX_SEL_BITMAP ? (const void*)s->bitmap.data() : (const void*)s->ids.data();
        alloc_exact(sel_dev, bytes);
        HIPCHECK(hipMemcpyAsync(sel_dev.p, src, bytes, hipMemcpyHostToDevice, h->st));
    }
    a.bitmap = s->kind == RSX_SEL_BITMAP ? sel_dev.as<uint8_t>() : nullptr; a.nbytes = (int64_t)s->bitmap.size();
    a.ids = s->kind == RSX_SEL_BATCH ? sel_dev.as<int64_t>() : nullptr; a.nids = (int64_t)s->ids.size();
    launch_sel_mask(a, slot_ids, nslots, mask.as<uint32_t>(), h->st);
}

// the index after a removal: lengths, directory (dir_gen: bound cache, selector mask cache), the stale row-major code copy
static void finish_removal(rsx_index* h, int64_t removed) {
    h->ntotal -= removed;
    h->codes_plain.release();
    h->plain_gen = ~0ull; h->plain_of = nullptr;
    upload_dir(h);
}

// IndexIVF::remove_ids: plan (one workgroup per list), one launch of moves, one launch clearing the vacated slots
static int64_t remove_ivf(rsx_index* h, const rsx_selector* s) {
    const int nlist = h->nlist;
    const bool pq = h->kind == KIND_IVFPQ;
    const bool l2 = h->metric == RSX_METRIC_L2 && !pq;
    DevBuf mask, sel_dev, plan, moves, runs;
    build_mask(h, s, h->ids.as<int64_t>(), h->total_cap, mask, sel_dev);
    alloc_exact(plan, (size_t)(3 * nlist + 1) * 8);
    int64_t* new_len = plan.as<int64_t>();
    int64_t* nmoves = new_len + nlist;
    int64_t* move_off = nmoves + nlist;
    launch_rm_ivf_plan_counts(mask.as<uint32_t>(), h->d_base.as<int64_t>(), h->d_len.as<int64_t>(), nlist, new_len, nmoves, move_off, h->st);
    std::vector<int64_t> nl((size_t)nlist);
    HIPCHECK(hipMemcpyAsync(nl.data(), new_len, (size_t)nlist * 8, hipMemcpyDeviceToHost, h->st));     // the removal's only read-back
    HIPCHECK(hipStreamSynchronize(h->st));
    HIPCHECK(hipGetLastError());
    int64_t removed = 0;
    for (int l = 0; l < nlist; l++) removed += h->h_len[(size_t)l] - nl[(size_t)l];
    if (removed == 0) return 0;
    // moves <= removed: sized by that bound, the kernels read the exact count (move_off[nlist]) on the device
    alloc_exact(moves, (size_t)removed * 8);
    uint32_t* msrc = moves.as<uint32_t>();
    uint32_t* mdst = msrc + removed;
    launch_rm_ivf_plan_moves(mask.as<uint32_t>(), h->d_base.as<int64_t>(), h->d_len.as<int64_t>(), new_len, nmoves, move_off, nlist, msrc, mdst,
                             h->st);
    const int64_t rb = (int64_t)h->row_bytes();
    launch_rm_ivf_move(msrc, mdst, move_off + nlist, removed, h->data.as<uint8_t>(), rb, pq, h->Mpad, h->CB, h->ids.as<int64_t>(),
                       l2 ? h->norms.as<float>() : nullptr, h->st);
    // vacated slots [new_len, len) of every list, in runs of at most 256 slots
    std::vector<int64_t> hr;
    for (int l = 0; l < nlist; l++)
        for (int64_t r0 = nl[(size_t)l]; r0 < h->h_len[(size_t)l]; r0 += 256)
            hr.insert(hr.end(), {h->h_base[(size_t)l] + r0, std::min<int64_t>(256, h->h_len[(size_t)l] - r0)});
    alloc_exact(runs, hr.size() * 8);
    HIPCHECK(hipMemcpyAsync(runs.p, hr.data(), hr.size() * 8, hipMemcpyHostToDevice, h->st));
    launch_rm_clear(runs.as<int64_t>(), (int64_t)hr.size() / 2, h->data.as<uint8_t>(), rb, pq, h->Mpad, h->CB, h->ids.as<int64_t>(),
                    l2 ? h->norms.as<float>() : nullptr, h->st);
    HIPCHECK(hipStreamSynchronize(h->st));      // (hr is a local)
    HIPCHECK(hipGetLastError());
    h->h_len = nl;
    finish_removal(h, removed);
    return removed;
}

// IndexFlatCodes::remove_ids (sequential ids: the selector sees positions, the survivors are renumbered 0 .. ntotal - 1) and
// IndexIDMap::remove_ids (explicit ids): stable compaction, staged chunk by chunk through at most max(256 MiB, payload / 16)
static int64_t remove_flat(rsx_index* h, const rsx_selector* s) {
    const int64_t n = h->h_len[0];
    const bool l2 = h->metric == RSX_METRIC_L2;
    int64_t* ids = h->custom_ids ? h->ids.as<int64_t>() : nullptr;
    float* norms = l2 ? h->norms.as<float>() : nullptr;
    DevBuf mask, sel_dev, scan;
    build_mask(h, s, ids, n, mask, sel_dev);
    const int64_t nw = (n + 31) / 32, nb = rm_flat_blocks(n);
    alloc_exact(scan, (size_t)round_up(nw * 4, 8) + (size_t)(2 * nb + 1) * 8);
    int64_t* blk_cnt = reinterpret_cast<int64_t*>(scan.as<uint8_t>() + round_up(nw * 4, 8));
    int64_t* blk_off = blk_cnt + nb;
    launch_rm_flat_scan(mask.as<uint32_t>(), n, scan.as<int32_t>(), blk_cnt, blk_off, h->st);
    int64_t kept = 0;
    HIPCHECK(hipMemcpyAsync(&kept, blk_off + nb, 8, hipMemcpyDeviceToHost, h->st));     // the removal's only read-back
    HIPCHECK(hipStreamSynchronize(h->st));
    HIPCHECK(hipGetLastError());
    const int64_t removed = n - kept;
    if (removed == 0) return 0;
    const int64_t rb = (int64_t)h->row_bytes(), per_row = rb + 8 + 4;
    const int64_t bound = std::max<int64_t>((int64_t)256 << 20, n * rb / 16);
    const int64_t fixed = (int64_t)(mask.bytes + sel_dev.bytes + scan.bytes);
    const int64_t unit = rm_flat_unit();
    int64_t chunk = std::max<int64_t>(unit, (bound - fixed) / per_row / unit * unit);
    chunk = std::min(chunk, round_up(n, unit));
    DevBuf stage;
    alloc_exact(stage, (size_t)(chunk * per_row));
    int64_t* st_ids = reinterpret_cast<int64_t*>(stage.as<uint8_t>() + chunk * rb);
    float* st_norms = reinterpret_cast<float*>(st_ids + chunk);
    for (int64_t lo = 0; lo < n; lo += chunk)
        launch_rm_flat_chunk(mask.as<uint32_t>(), scan.as<int32_t>(), blk_off, lo, std::min(n, lo + chunk), h->data.as<uint8_t>(), rb, ids, norms,
                             stage.as<uint8_t>(), st_ids, st_norms, h->st);
    // vacated rows [kept, n): zero rows and norms, ids -1
    HIPCHECK(hipMemsetAsync(h->data.as<uint8_t>() + kept * rb, 0, (size_t)(removed * rb), h->st));
    if (norms) HIPCHECK(hipMemsetAsync(norms + kept, 0, (size_t)removed * 4, h->st));
    if (ids) HIPCHECK(hipMemsetAsync(ids + kept, 0xFF, (size_t)removed * 8, h->st));
    HIPCHECK(hipStreamSynchronize(h->st));
    HIPCHECK(hipGetLastError());
    h->h_len[0] = kept;
    finish_removal(h, removed);
    return removed;
}

int64_t remove_impl(rsx_index* h, const rsx_selector* s) {
    if (h->add_list_mod > 1)
        RSX_THROW(RSX_ERR_UNSUPPORTED, "remove_ids: not available on a list shard (add_list_mod = %d): its sequential-id count cannot be kept "
                  "right from one rank", h->add_list_mod);
    if (h->ntotal == 0) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t removed = h->kind == KIND_FLAT ? remove_flat(h, s) : remove_ivf(h, s);
    h->timing["remove_calls"] += 1;
    h->timing["removed"] += (double)removed;
    h->timing["remove_ms"] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return removed;
}

// every shard removes in parallel; the logical index's next sequential id follows the single index's rule (FAISS: ntotal)
int64_t sharded_remove(rsx_index* h, const rsx_selector* s) {
    if (h->kind == KIND_FLAT && !h->custom_ids)
        RSX_THROW(RSX_ERR_UNSUPPORTED, "remove_ids: a sharded Flat index with sequential ids cannot renumber across its shards "
                  "(faiss.IndexShards has no remove_ids either)");
    for (auto* c : h->shards)
        if (c->add_list_mod > 1) RSX_THROW(RSX_ERR_UNSUPPORTED, "remove_ids: not available on a list shard (add_list_mod = %d)", c->add_list_mod);
    std::vector<int64_t> rem(h->shards.size(), 0);
    for_each_shard_parallel(h, [&](int r, rsx_index* c) { rem[(size_t)r] = remove_impl(c, s); });
    int64_t removed = 0;
    for (int64_t v : rem) removed += v;
    if (removed) { h->ntotal -= removed; h->sh_next_id = h->ntotal; }
    return removed;
}
