// api_merge.hip — rsx_merge_from (FAISS IndexIVF::merge_from / IndexFlatCodes::merge_from / IndexIDMap::merge_from) and
// rsx_copy_subset_to (IndexIVF::copy_subset_to): checks, plan, capacity, launches (k_merge.hip) and bookkeeping.  DESIGN.md 7k.
// Order of work, so that a refusal or a failed allocation leaves BOTH handles as they were: every check, the free-memory check and
// ensure_capacity(dst), the copy, the stream's synchronisation, and only then the lengths of either handle.
// Shared declarations: rsx_host.h.
#include <chrono>
#include "rsx_host.h"
#include "k_merge.h"

static const char* kind_name(const rsx_index* h) {
    static const char* names[] = {"IndexFlat", "IndexIVFFlat", "IndexIVFPQ", "IndexPQ", "IndexIVFScalarQuantizer", "IndexScalarQuantizer"};
    return names[public_kind(h)];
}
static bool same_floats(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

// everything that must hold before either handle is touched (FAISS's check_compatible_for_merge compares the sizes only: we also compare
// the trained parameters bit for bit)
static void check_pair(const rsx_index* dst, const rsx_index* src, const char* what) {
    if (!dst || !src) RSX_THROW(RSX_ERR_INVALID, "null pointer");
    if (dst == src) RSX_THROW(RSX_ERR_INVALID, "%s: source and destination are the same handle", what);
    if (is_sharded(dst) || is_sharded(src))
        RSX_THROW(RSX_ERR_UNSUPPORTED, "%s: not available on a sharded handle (merge or split the per-device indexes, then shard the result)", what);
    refuse_while_two_call(dst, what);
    refuse_while_two_call(src, what);
    if (dst->add_list_mod > 1 || src->add_list_mod > 1)
        RSX_THROW(RSX_ERR_UNSUPPORTED, "%s: not available on a list shard (add_list_mod = %d): its sequential-id count cannot be kept right from one rank",
                  what, std::max(dst->add_list_mod, src->add_list_mod));
    if (public_kind(dst) != public_kind(src))
        RSX_THROW(RSX_ERR_INVALID, "%s: the handles differ in kind (%s and %s)", what, kind_name(dst), kind_name(src));
#define MG_SAME(field, name)                                                                                                        \
    if (dst->field != src->field) RSX_THROW(RSX_ERR_INVALID, "%s: the handles differ in %s (%d and %d)", what, name, (int)dst->field, (int)src->field)
    MG_SAME(d, "d"); MG_SAME(metric, "metric"); MG_SAME(nlist, "nlist"); MG_SAME(M, "M"); MG_SAME(nbits, "nbits"); MG_SAME(sq_qtype, "qtype");
    MG_SAME(by_residual, "by_residual");
#undef MG_SAME
    if (!dst->trained || !src->trained) RSX_THROW(RSX_ERR_NOT_TRAINED, "%s: both handles must be trained", what);
    if (dst->device != src->device) RSX_THROW(RSX_ERR_INVALID, "%s: the handles live on different devices (%d and %d)", what, dst->device, src->device);
    if (!same_floats(dst->h_centroids, src->h_centroids)) RSX_THROW(RSX_ERR_INVALID, "%s: the handles' centroids differ (they must be bit-equal)", what);
    if (!same_floats(dst->h_codebooks, src->h_codebooks)) RSX_THROW(RSX_ERR_INVALID, "%s: the handles' codebooks differ (they must be bit-equal)", what);
    if (!same_floats(dst->h_sq, src->h_sq)) RSX_THROW(RSX_ERR_INVALID, "%s: the handles' scalar-quantiser parameters differ (they must be bit-equal)", what);
}

struct MergePlan {
    std::vector<int64_t> first, count;      // per list: position of the run's first entry in the source list (contiguous forms), entries
    bool sel = false;                       // subset types 0 / 1: the entries are sel_rows[off[l] .. off[l] + count[l])
    DevBuf sel_rows;
    int64_t total = 0;
};

// The append itself.  add_id is what the stored ids gain; adopt_ids: a Flat destination without rows takes over the source's explicit ids.
// Returns with the stream synchronised and dst's lengths, counters and derived state updated; src is not touched.
static void append_rows(rsx_index* dst, rsx_index* src, MergePlan& plan, int64_t add_id, const char* what) {
    const int nlist = dst->nlist;
    const bool rowkind = dst->kind == KIND_FLAT || dst->kind == KIND_IVFFLAT;
    const bool adopt_ids = dst->kind == KIND_FLAT && src->custom_ids && !dst->custom_ids;
    std::vector<int64_t> need(dst->h_len);
    bool grow = false;
    for (int l = 0; l < nlist; l++) {
        need[(size_t)l] += plan.count[(size_t)l];
        grow = grow || need[(size_t)l] > dst->h_cap[(size_t)l];
    }
    // fp32 rows on either side: dst ends as fp32 (what one index fed all the vectors would hold)
    const bool upgrade = rowkind && dst->storage_f16 && !src->storage_f16;
    const size_t drb_after = upgrade ? (size_t)dst->ld * 4 : dst->row_bytes();
    // room for what the steps below allocate: a re-layout holds dst old, dst new and src at once, the widening dst old and dst new
    {
        size_t want = 0;
        if (grow) {
            int64_t rows = 0;
            for (int l = 0; l < nlist; l++)
                rows += round_up(std::max(dst->h_cap[(size_t)l], dst->kind == KIND_IVFPQ ? 2 * need[(size_t)l] + 64 : need[(size_t)l] + need[(size_t)l] / 2), dst->row_align());
            want += (size_t)rows * (drb_after + 12);
        }
        if (upgrade && dst->data.p) want += (size_t)std::max<int64_t>(dst->total_cap, dst->row_align()) * dst->ld * 4;
        want += plan.count.size() * 64 + (size_t)(plan.total / rsx::MG_TILE + nlist + 1) * sizeof(MergeItem);
        size_t free_b = 0, total_b = 0;
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        if (want > free_b)
            RSX_THROW(RSX_ERR_OOM, "%s: needs about %zu MiB of device memory, %zu MiB are free (reserve_lists on the destination beforehand avoids the re-layout)",
                      what, want >> 20, free_b >> 20);
    }
    const bool old_custom = dst->custom_ids;
    if (upgrade) upgrade_storage_to_f32(dst);      // (values unchanged: a failure further down leaves an index that answers as before)
    try {
        if (adopt_ids) dst->custom_ids = true;     // ensure_capacity then allocates the ids
        ensure_capacity(dst, need, false);
    } catch (...) {
        dst->custom_ids = old_custom;
        throw;
    }
    if (grow) dst->timing["merge_relayouts"] += 1;
    std::vector<MergeItem> items;
    int64_t off = 0;
    for (int l = 0; l < nlist; l++) {
        const int64_t c = plan.count[(size_t)l];
        const int64_t d0 = dst->h_base[(size_t)l] + dst->h_len[(size_t)l];
        if (plan.sel) mg_push_items(items, off, d0, c, 1);
        else mg_push_items(items, src->h_base[(size_t)l] + plan.first[(size_t)l], d0, c, 0);
        off += c;
    }
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf ditems;
    ditems.ensure(std::max<size_t>(items.size(), 1) * sizeof(MergeItem));
    HIPCHECK(hipMemcpyAsync(ditems.p, items.data(), items.size() * sizeof(MergeItem), hipMemcpyHostToDevice, dst->st));
    const bool has_ids = dst->kind != KIND_FLAT || dst->custom_ids;
    const bool has_norms = dst->metric == RSX_METRIC_L2 && dst->kind != KIND_IVFPQ;
    if (dst->kind == KIND_IVFPQ) {
        launch_mg_pq(ditems.as<MergeItem>(), (int64_t)items.size(), plan.sel_rows.as<uint32_t>(), src->data.as<uint8_t>(), dst->data.as<uint8_t>(), dst->M,
                     dst->Mpad, src->CB, dst->CB, src->ids.as<int64_t>(), dst->ids.as<int64_t>(), add_id, dst->st);
    } else {
        const int widen = rowkind && src->storage_f16 && !dst->storage_f16;
        launch_mg_rows(ditems.as<MergeItem>(), (int64_t)items.size(), plan.sel_rows.as<uint32_t>(), src->data.as<uint8_t>(), dst->data.as<uint8_t>(),
                       (int64_t)src->row_bytes(), (int64_t)dst->row_bytes(), widen, has_ids ? src->ids.as<int64_t>() : nullptr,
                       has_ids ? dst->ids.as<int64_t>() : nullptr, add_id, has_norms ? src->norms.as<float>() : nullptr,
                       has_norms ? dst->norms.as<float>() : nullptr, dst->st);
    }
    HIPCHECK(hipGetLastError());
    // the certificates' maxima: the larger of both sides, on the host and in the device word the next add folds its rows into
    if (dst->kind != KIND_IVFPQ) {
        dst->max_norm2 = std::max(dst->max_norm2, src->max_norm2);
        dst->sq_bn2 = std::max(dst->sq_bn2, src->sq_bn2);
        unsigned int w[2]; memcpy(&w[0], &dst->max_norm2, 4); w[1] = dst->sq_bn2;
        const size_t nw = dst->kind == KIND_IVFSQ ? 2 : 1;
        if (rowkind && !dst->d_maxnorm.p) dst->d_maxnorm.ensure(sizeof(unsigned int));
        if (dst->d_maxnorm.p) HIPCHECK(hipMemcpyAsync(dst->d_maxnorm.p, w, nw * sizeof(unsigned int), hipMemcpyHostToDevice, dst->st));
    }
    HIPCHECK(hipStreamSynchronize(dst->st));      // (items and w are locals)
    HIPCHECK(hipGetLastError());
    dst->timing["merge_copy_ms"] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    dst->timing["merge_rows"] += (double)plan.total;
    if (rowkind) dst->storage_decided = dst->storage_decided || src->storage_decided;
    dst->h_len = need;
    dst->ntotal += plan.total;
    dst->codes_plain.release();
    dst->plain_gen = ~0ull; dst->plain_of = nullptr;
    upload_dir(dst);
}

void merge_from_impl(rsx_index* dst, rsx_index* src, int64_t add_id) {
    const char* what = "merge_from";
    check_pair(dst, src, what);
    const bool flat_codes = dst->flat_pq || dst->flat_sq || (dst->kind == KIND_FLAT && !dst->custom_ids && !src->custom_ids);
    if (flat_codes && add_id != 0) RSX_THROW(RSX_ERR_INVALID, "merge_from: cannot set ids in FlatCodes index (add_id must be 0, got %lld)", (long long)add_id);
    if (src->ntotal == 0) return;
    if (dst->kind == KIND_FLAT && dst->custom_ids != src->custom_ids && !(src->custom_ids && dst->ntotal == 0))
        RSX_THROW(RSX_ERR_INVALID, "merge_from: %s", dst->custom_ids ? "the destination carries explicit ids, the source sequential ones"
                                                                     : "the source carries explicit ids, the populated destination sequential ones");
    use_device(dst);
    HIPCHECK(hipStreamSynchronize(src->st));
    HIPCHECK(hipStreamSynchronize(dst->st));
    MergePlan plan;
    plan.first.assign((size_t)dst->nlist, 0);
    plan.count = src->h_len;
    plan.total = src->ntotal;
    // IndexPQ / IndexScalarQuantizer keep their sequential ids in the one list's id array: source row i becomes id ntotal + i
    const int64_t shift = (dst->flat_pq || dst->flat_sq) ? dst->ntotal : add_id;
    // what sequential adds into ONE index would have produced keeps the handle free of "explicit ids"
    const bool sequential = !dst->ids_given && !src->ids_given && (flat_codes || add_id == dst->ntotal);
    append_rows(dst, src, plan, shift, what);
    dst->ids_given = !sequential;
    // src ends empty (as rsx_reset leaves it): still trained, its capacity kept
    std::fill(src->h_len.begin(), src->h_len.end(), 0);
    src->ntotal = 0; src->ndropped = 0; src->ids_given = false;
    src->codes_plain.release();
    src->plain_gen = ~0ull; src->plain_of = nullptr;
    upload_dir(src);
}

void copy_subset_impl(rsx_index* src, rsx_index* dst, int type, int64_t a1, int64_t a2) {
    const char* what = "copy_subset_to";
    check_pair(dst, src, what);
    if (dst->kind == KIND_FLAT || dst->flat_pq || dst->flat_sq)
        RSX_THROW(RSX_ERR_UNSUPPORTED, "copy_subset_to: IVF indexes only (this is an %s)", kind_name(dst));
    if (type == rsx::MG_SUBSET_INVLIST_FRACTION || type == rsx::MG_SUBSET_INVLIST)
        RSX_THROW(RSX_ERR_UNSUPPORTED, "copy_subset_to: subset type %d (%s) is not implemented", type,
                  type == rsx::MG_SUBSET_INVLIST ? "SUBSET_TYPE_INVLIST" : "SUBSET_TYPE_INVLIST_FRACTION");
    if (type < 0 || type > 4) RSX_THROW(RSX_ERR_INVALID, "copy_subset_to: unknown subset type %d", type);
    const int64_t nt = src->ntotal;
    if (type == rsx::MG_SUBSET_ID_RANGE && a1 > a2) RSX_THROW(RSX_ERR_INVALID, "copy_subset_to: id range needs a1 <= a2 (got %lld, %lld)", (long long)a1, (long long)a2);
    if (type == rsx::MG_SUBSET_ID_MOD && (a1 <= 0 || a2 < 0 || a2 >= a1))
        RSX_THROW(RSX_ERR_INVALID, "copy_subset_to: id modulo needs a1 > 0 and 0 <= a2 < a1 (got %lld, %lld)", (long long)a1, (long long)a2);
    if (type == rsx::MG_SUBSET_ELEMENT_RANGE && (a1 < 0 || a2 < a1 || a2 > nt))
        RSX_THROW(RSX_ERR_INVALID, "copy_subset_to: element range needs 0 <= a1 <= a2 <= ntotal (got %lld, %lld; ntotal %lld)", (long long)a1, (long long)a2, (long long)nt);
    if (nt == 0) return;
    use_device(dst);
    HIPCHECK(hipStreamSynchronize(src->st));
    HIPCHECK(hipStreamSynchronize(dst->st));
    const int nlist = src->nlist;
    MergePlan plan;
    plan.first.assign((size_t)nlist, 0);
    plan.count.assign((size_t)nlist, 0);
    if (type == rsx::MG_SUBSET_ELEMENT_RANGE) {
        int64_t accu[3] = {0, 0, 0};
        for (int l = 0; l < nlist; l++) {
            int64_t i1, i2;
            mg_element_range(src->h_len[(size_t)l], nt, a1, a2, accu, i1, i2);
            const int64_t c = std::max<int64_t>(0, i2 - i1);      // (i1 > i2 happens in lists whose share of the range is below two entries: FAISS's loop then copies nothing)
            plan.first[(size_t)l] = i1; plan.count[(size_t)l] = c; plan.total += c;
        }
    } else {
        // the per-list counts are the operation's only read-back
        DevBuf cnt, off;
        cnt.ensure((size_t)nlist * 8);
        launch_mg_count(src->ids.as<int64_t>(), src->d_base.as<int64_t>(), src->d_len.as<int64_t>(), nlist, type, a1, a2, cnt.as<int64_t>(), dst->st);
        HIPCHECK(hipMemcpyAsync(plan.count.data(), cnt.p, (size_t)nlist * 8, hipMemcpyDeviceToHost, dst->st));
        HIPCHECK(hipStreamSynchronize(dst->st));
        HIPCHECK(hipGetLastError());
        std::vector<int64_t> offs((size_t)nlist);
        for (int l = 0; l < nlist; l++) { offs[(size_t)l] = plan.total; plan.total += plan.count[(size_t)l]; }
        if (plan.total > 0) {
            plan.sel = true;
            plan.sel_rows.ensure((size_t)plan.total * 4);
            off.ensure((size_t)nlist * 8);
            HIPCHECK(hipMemcpyAsync(off.p, offs.data(), (size_t)nlist * 8, hipMemcpyHostToDevice, dst->st));
            launch_mg_fill(src->ids.as<int64_t>(), src->d_base.as<int64_t>(), src->d_len.as<int64_t>(), nlist, type, a1, a2, off.as<int64_t>(),
                           plan.sel_rows.as<uint32_t>(), dst->st);
            HIPCHECK(hipStreamSynchronize(dst->st));      // (offs is a local)
            HIPCHECK(hipGetLastError());
        }
    }
    if (plan.total == 0) return;
    append_rows(dst, src, plan, 0, what);
    dst->ids_given = true;
}
