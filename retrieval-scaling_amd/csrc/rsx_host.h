// rsx_host.h — host side of librsx shared by the api_*.hip files: error plumbing, device / pinned buffers, the index object
// (struct rsx_index = the opaque rsx_index_t of include/rsx.h) and the prototypes of the host functions that cross files.
//   api_build.hip    HBM layout management, add / train, list import / export, persistence
//   api_search.hip   the search drivers (search_batch = one internal batch, search_impl = one rsx_search call)
//   api_stages.hip   the batch stages that search and range_search share (declarations in rsx_stages.h)
//   api_refine.hip   rsx_refine: exact re-ranking of candidate labels against a Flat row store (k_refine.hip)
//   api_range.hip    rsx_range_search: every neighbour within a radius, Flat and IVF-Flat (k_range.hip; declarations in rsx_range.h)
//   api_reconstruct.hip  rsx_reconstruct_batch / rsx_make_direct_map: stored vectors by id (k_reconstruct.hip; rsx_reconstruct.h)
//   api_vt.hip       rsx_vt_*: the linear vector transform handle and its entry points (k_vt.hip)
//   api_sharded.hip  the single-process multi-GPU handle
//   api_remove.hip   rsx_remove_ids: the removal plan and compaction (k_remove.hip) on a handle and on the shards of one
//   api_merge.hip    rsx_merge_from / rsx_copy_subset_to: joining and splitting indexes on one device (k_merge.hip; mapping in k_merge.h)
//   rsx_api.hip      the extern "C" entry points
// Host control plane only; all search arithmetic is in the k_*.hip kernels.  There is no CPU search path.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/rsx.h"
#include "rsx_internal.h"
#include "rsx_sel.h"

using namespace rsx;

// ---------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------
extern thread_local std::string g_err;      // rsx_api.hip

struct RsxError : std::runtime_error {
    int code;
    RsxError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
#define RSX_THROW(code, ...)                                  \
    do {                                                      \
        char _b[512]; snprintf(_b, sizeof(_b), __VA_ARGS__);  \
        throw RsxError(code, _b);                             \
    } while (0)
#define HIPCHECK(expr)                                                                              \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            int code = (_e == hipErrorOutOfMemory) ? RSX_ERR_OOM : RSX_ERR_HIP;                     \
            RSX_THROW(code, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                           \
    } while (0)

template <typename F>
static inline int guarded(F&& f) {
    try {
        f();
        return RSX_OK;
    } catch (const RsxError& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_err = "host allocation failed";
        return RSX_ERR_OOM;
    } catch (const std::exception& e) {
        g_err = e.what();
        return RSX_ERR_INVALID;
    }
}

// ---------------------------------------------------------------------------------------
// device buffers
// ---------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool host_mapped = false;     // page-locked HOST memory mapped into the device (the per-query flag words: kernels write them across the
                                  // bus, the host reads them after the stream's synchronisation — no copy command at the end of a batch)
    void ensure(size_t n) {
        if (n <= bytes) return;
        release();
        size_t want = n + n / 8;
        if (host_mapped) { HIPCHECK(hipHostMalloc(&p, want, hipHostMallocMapped)); bytes = want; return; }
        if (hipMalloc(&p, want) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            HIPCHECK(hipMalloc(&p, n));
            want = n;
        }
        bytes = want;
    }
    void release() {
        if (p) (void)(host_mapped ? hipHostFree(p) : hipFree(p));
        p = nullptr; bytes = 0;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// Page-locked host staging for the small transfers of the latency path (a single query in, k results and the
// certificate flags out): copies to and from pageable memory go through the runtime's own staging and block the host.
struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool ensure(size_t n) {          // false: no pinned memory to be had — the caller keeps the pageable path
        if (n <= bytes) return true;
        release();
        if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
        bytes = n;
        return true;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
    ~PinBuf() { release(); }
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
};

static inline bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

static inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
static inline int pow2ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }
static inline int64_t pow2ceil64(int64_t x) { int64_t p = 1; while (p < x) p <<= 1; return p; }

// ---------------------------------------------------------------------------------------
// deterministic host RNG shared with the training spec (splitmix64 Fisher-Yates)
// ---------------------------------------------------------------------------------------
static inline uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline void rand_perm(int64_t n, uint64_t seed, std::vector<int64_t>& perm) {
    perm.resize((size_t)n);
    uint64_t s = seed;
    for (int64_t i = 0; i < n; i++) perm[(size_t)i] = i;
    for (int64_t i = 0; i + 1 < n; i++) {
        int64_t j = i + (int64_t)(splitmix(s) % (uint64_t)(n - i));
        std::swap(perm[(size_t)i], perm[(size_t)j]);
    }
}

// ---------------------------------------------------------------------------------------
// the index object
// ---------------------------------------------------------------------------------------
// faiss.IDSelector* behind rsx_selector_t (include/rsx.h): immutable after rsx_selector_create.  serial identifies it in the slot-mask
// cache of a handle (rsx_index::sel_*): a new selector never reuses a live one's serial.
struct rsx_selector {
    int kind = 0, invert = 0;
    int64_t lo = 0, hi = 0;                 // RSX_SEL_RANGE
    std::vector<uint8_t> bitmap;            // RSX_SEL_BITMAP
    std::vector<int64_t> ids;               // RSX_SEL_BATCH: sorted, unique
    uint64_t serial = 0;
    bool contains(int64_t id) const {
        bool m;
        if (kind == RSX_SEL_RANGE) m = id >= lo && id < hi;
        else if (kind == RSX_SEL_BITMAP) m = id >= 0 && (id >> 3) < (int64_t)bitmap.size() && ((bitmap[(size_t)(id >> 3)] >> (id & 7)) & 1);
        else m = std::binary_search(ids.begin(), ids.end(), id);
        return m != (invert != 0);
    }
};

struct rsx_index {
    int kind = 0, d = 0, metric = 0, device = 0;
    int nlist = 1, M = 0, nbits = 8, Mpad = 0, CB = 16, dsub = 0;   // CB: code layout (rsx_internal.h), 0 = rotated
    int CB_granule = 16;
#ifndef PQ_LAYOUT_DEFAULT
#define PQ_LAYOUT_DEFAULT 2      // RSX_PQ_LAYOUT unset: 1 = rotated wherever it applies, 2 = additionally the sliced layout for M = 96
#endif
    int nprobe = 1;
    // RSX_KIND_PQ (faiss.IndexPQ, rsx_pq_create): stored as an IVF-PQ index of ONE list with a zero centroid (kind stays KIND_IVFPQ: code
    // layouts, encoder, table builders, finalize and the RSX1 writer are shared; residual = x - 0 = x, dis0 = <q, 0> = +0) that reports
    // kind 3, refuses what a flat index has not, and searches through the staged filtered scan (api_search.hip: pq_staged_scan)
    bool flat_pq = false;
    // KIND_IVFSQ (faiss.IndexIVFScalarQuantizer, QT_8bit; rsx_ivfsq_create): rows of ld code bytes in the IVF-Flat directory, ids
    // and (L2) norm terms of the DECODED vectors beside them; sq_trained = vmin[d] then vdiff[d]; max_norm2 is over the decoded vectors
    int sq_qtype = 0; bool by_residual = false;
    // RSX_KIND_SQ (faiss.IndexScalarQuantizer, rsx_sq_create): stored as an IVF-SQ index of ONE list with a zero centroid and
    // by_residual off (kind stays KIND_IVFSQ: training, encoder, list import / export, the RSX1 record, finalize and the exact re-run are
    // shared) that reports kind 5, refuses what a flat index has not, and sends batches of more than 32 queries through the int8 GEMM scan
    // (api_sqflat.hip)
    bool flat_sq = false;
    int sqflat_cand_cap = 0;                      // ... keys a query's candidate row holds per stage (0 = 32768 for K' <= 64, else 131072); read by this kind only
    DevBuf w_sqfbq, w_sqfbD, w_sqfbI;             // ... the flagged queries of a batch and their second search's results (sqf_rerun)
    DevBuf w_sqplanes, w_sqs;                    // ... per-batch int8 query planes and {1 / s, constant} per query (k_sqflat_planes; layout: rsx_sqflat.h)
    std::vector<float> h_sq; DevBuf d_sq;
    float sq_nvmin = 0.0f, sq_nvdiff = 0.0f;      // >= the L2 norms of vmin / vdiff (certificate terms, with the parameters)
    float sq_vdmax = 0.0f;                        // the largest vdiff_j
    unsigned int sq_bn2 = 0;                      // the largest sum_j (code_j - 128)^2 of a row ever stored (with max_norm2).  Like max_norm2 of the
                                                  // row kinds, both survive rsx_reset: maxima over everything EVER stored — conservative for the certificate
    DevBuf w_sqhi, w_sqlo, w_sqc;                 // per-batch query factors (k_sq_query_factors)
    bool trained = false;
    int64_t ntotal = 0;
    hipStream_t st = nullptr;
    PinBuf pin_q, pin_out, pin_flags;     // latency path: pinned staging of queries / results / certificate flags

    // trained parameters
    std::vector<float> h_centroids, h_codebooks;
    DevBuf d_centroids, d_codebooks;
    DevBuf cent16;            // fp16 copy of the centroids, [round_up(nlist, 128)][ld] zero padded: the fast coarse quantiser's operand (built on demand)
    uint64_t cent_gen = 0, cent16_gen = 0;   // set_centroids counts; the copy belongs to cent16_gen
    float cent_cmax = 0.0f; uint64_t cent_cmax_gen = ~0ull;   // >= the largest centroid norm, of centroid set cent_cmax_gen (api_search.hip: cent_cmax; the fast
                                                              // coarse quantiser's bound and the by_residual scalar quantiser's certificate term)
    int coarse_fast = 1;      // coarse quantiser: fp16 MFMA scores + exact re-score of the candidates (k_coarse_pick), 0 = the exact GEMM for all lists

    // storage.  PQ: slab layout bytes.  Flat/IVFFlat: rows of ld elements (fp16 or fp32).
    int ld = 0;               // row stride (elements) of flat rows: d rounded up to 64
    int storage_f16 = 1;
    bool storage_decided = false;
    bool custom_ids = false;  // Flat: ids array only when the caller supplied ids (sharded Flat handle: its adds carried ids; the shards
                              // always store the logical ids)
    bool ids_given = false;   // any kind: an rsx_add since the last reset carried ids (rsx_get "explicit_ids"; IndexRefineFlat refuses such a base)
    DevBuf data, ids, norms;
    DevBuf codes_plain;               // IVF-PQ, block layouts: row-major copy of the codes for large-K' finalizes, built on demand (api_search.hip)
    uint64_t plain_gen = ~0ull; const void* plain_of = nullptr;
    std::vector<int64_t> h_base, h_len, h_cap;
    DevBuf d_base, d_len;
    int64_t total_cap = 0;

    // knobs
    int query_batch = 1024;
    int scan_chunk = 0;
    int scan_kernel = 0;  // 0 = auto (list-major v2 when the layout allows), 1 = force the per-pair v1 kernel
    int pq_fast = 1;      // IVFPQ: 8-bit-table fast scan + certified exact re-rank (results identical to exact)
    int pq_fast_kp = 0;   // candidates kept by the fast scan (0 = auto); tests shrink it to force fallbacks
    int pq_filter = 1;    // fast scan: filter candidates inside the scan kernel (0 = full score buffer + select)
    int pq_pace = 128 | (4 << 12);   // rotated fast scan schedule (never changes a result): bit 7 = a query group that starts while a
                          // sibling group of its list tile is under way JOINS it at its position and wraps around (L2 reuse of the code
                          // lines), bits 8-11 = join offset in tile rows (0 = 2), bits 12-15 = the last n rows of a tile are handed to
                          // the waves dynamically (default 4; 0 = static columns), bit 4 = every chunk dynamic, bit 6 = no issue-
                          // priority rotation
    int pq_q8 = 1;        // eight queries per table gather (8-byte entries, ds_read_b64): rotated layout M = 64 (k_pq_scan_rot<..., 2>; 0 = the 4-query form);
                          // sliced layout (M = 96): 1 = k_pq_scan_sl8 for batches with >= 3 probing queries per list on lists of >= 4096 vectors on average,
                          // else the four-query single-pass k_pq_scan_sl4; 2 = always eight, 0 = always four
    int pq_prune = 0;     // rotated fast scan: skip (list, query group) items that cannot hold a survivor (exact bound; opt-in)
    int pq_lut_early = 1;     // pass 0 of the matrix-core table build as extra workgroups of the probe-pick launch (0 = its own launch)
    int pq_group_fused = 1;   // the (query, probe) pairs grouped by list by extra workgroups of the table launch (0 = its own four launches)
    uint32_t pg_epoch = 0;    // ... whose hand-over words carry this launch counter
    int lut_tiled = 2;    // fast scan tables (dsub 8): non-zero = tiled build sharing codebook slices across queries (inner product: on the matrix cores,
                          // k_pq_lut_mfma, two launches; L2: VALU tiles, k_pq_lut_tiled + k_pq_qparam), 0 = one workgroup per query
    int pq_prepass_fused = 1;   // filtered fast scan: threshold pre-pass in one launch (0 = grouping + scan + selection)
    int ivf_qtiles = 1;      // IVF-Flat LDS-DMA scans: 1 = choose 16 / 64 / 128 probing queries per group from the queries per list, 2 / 4 / 8 = force 32 / 64 / 128, 0 = always 16
    int pq_prepass4 = 1;     // rotated fast scan, full batches: threshold pre-pass with four queries per workgroup on the scan's table format (1 = small and large k, 2 = small k only, 0 = never)
    int pq_plain_codes = 1;  // block layouts, K' >= 256: finalize from a row-major copy of the codes (built on demand, M bytes per vector)
    int pq_gather = 1;       // rotated fast scan: candidate gather + selection in one launch (k_pq_gather_select) instead of compaction + merge
    int pq_final_tab = 1;    // rotated fast scan: finalize from the complete candidate row with the fp32 table in LDS (1 = when K' >= 512 or dsub > 8 and as the second chance, 2 = always, 0 = never)
    int pq_log_cap = 0;      // rotated fast scan: keys per survivor log (0 = from the pool budget); tests shrink it to force the overflow path
    int pq_pre_mult = 80, pq_pre_max = 16384;    // ... and for larger k: pq_pre_mult x k rows, at most pq_pre_max (<= 32768: 64 KiB of 16-bit sums in LDS; 16384 measured best overall on the headline index at k = 100 / 1000 / 2000, profiles/r04u_pre_sweep.jsonl; round 6, after the four-query histogram pre-pass: 80 x k — k = 100 2.95 -> 2.88 ms per batch, k = 50 / 200 / 1000 unchanged, profiles/r06_fixed_cost.md 5)
    int pq_flat_first = 0;       // IndexPQ staged scan: rows of the first stage (0 = 4 scan tiles, at least 64 k rows)
    int pq_flat_growth = 0;      // ... percent by which a stage outgrows the one before it (0 = 300: each stage three times the rows scanned so far)
    int pq_flat_max_stages = 0;  // ... most stages (0 = 12; the last stage takes whatever is left)
    int pq_pre_rows = 4096;  // filtered fast scan: vectors of each query's closest list the threshold pre-pass scores (0 = one scan tile)
    int pq_tau_anchor = 1;   // four-query threshold pre-pass: raise the threshold to (k-th best CANONICAL score of the sample's k best rows) - eps; 0 = a_k - 2 eps alone.  Read per batch
    int add_list_mod = 1, add_list_rem = 0;   // IVF add keeps only lists l with l % mod == rem (list-sharded multi-GPU index)
    int64_t ndropped = 0;                     // vectors seen by add but owned by other shards
    int flat_filter = 1;  // Flat: filtered GEMM launches after the threshold phase (0 = score buffer per chunk)
    int flat_pre_mult = 16;  // Flat: rows of the threshold phase per K' (through the score buffer), rounded up to units of flat_pre_unit rows
    int ivf_overflow_max = 0; // IVF-Flat filtered scan: overflowed candidate rows whose queries are re-run exactly on their own before the batch is rescanned (0 = max(2, nq / 128))
    int flat_pre_unit = 0;   // Flat: rows per unit of the threshold phase and the stage boundaries (0 = 16384 for K' <= 64, else 32768)
    int flat_stages = 0;     // Flat: filtered stages behind the threshold phase (0 = from K' and the row count; see search_batch)
    int ivf_filter = 1;   // IVF-Flat: candidates filtered inside the list scan (0 = full score rows + select)
    int ivf_pre_lists = 0;   // IVF-Flat threshold sample at large K': closest lists sampled (0 = 2)
    int ivf_pre_mult = 4;    // ... and rows of each per K'
    int range_cand_cap = 0;  // range search: keys a query's candidate row holds in the first scan (0 = 65536; rounded up to a power of two); queries with more are scanned again with rows sized from their counts
    int profile = 0;
    int64_t temp_budget = (int64_t)16 << 30;

    // workspace
    DevBuf w_q32, w_q16, w_coarse, w_keys1, w_probekeys, w_probelist, w_dis0, w_segstart, w_temp, w_lut, w_lutws, w_pgflags, w_state,
        w_D, w_I, w_qin, w_pairs, w_flag, w_x, w_partial, w_assign, w_dest, w_idsin, w_misc, w_lut8, w_qparam, w_uncertain, w_fbq, w_fbD, w_fbI, w_cand, w_candcnt, w_itemdesc, w_tau, w_excl, w_state2, w_addcnt, w_addstart, w_qitems, w_tiews, w_stagedir, w_rlabels, w_rflag,
        w_rg_cnt, w_rg_nmem, w_rg_lims, w_rg_kptr;      // range search: per-row candidate counts, member counts, the batch's lims, the rows' key pointers
    std::vector<int32_t> stage_host;      // IndexPQ staged scan: host image of w_stagedir (the stages' item tables), alive while the copy runs
    std::map<std::string, double> timing;

    // filtered search (rsx_search_sel): the selector of the call in flight (null = unfiltered) and its slot mask — bit s of
    // sel_mask = the vector in storage slot s is selected — cached per (selector, directory generation, storage)
    const rsx_selector* sel = nullptr;
    DevBuf sel_mask, sel_dev;               // sel_dev: the selector's bitmap / sorted ids while the mask is built
    uint64_t sel_mask_serial = 0, sel_mask_gen = 0;
    const void* sel_mask_of = nullptr;

    // direct map (rsx_reconstruct_batch): id -> storage row, derived from the list directory and the ids.  dmap holds
    // dmap_n int64 rows (Array) or dmap_n (id, row) slots (Hashtable, dmap_n a power of two); it belongs to directory generation
    // dmap_gen and is RELEASED by upload_dir / ensure_capacity, i.e. by every mutation (api_reconstruct.hip: release_direct_map)
    DevBuf dmap, dmap_ws, w_rkeys, w_rout;
    int dmap_type = 0;        // what dmap holds: 0 = nothing, 1 = Array, 2 = Hashtable (rsx_get "direct_map_type")
    int dmap_pref = 1;        // what the next build makes: 1 = Array where the ids allow it, else Hashtable; 2 = Hashtable
    int64_t dmap_n = 0;
    uint64_t dmap_gen = ~0ull;

    // Flat / IVF-Flat: largest |x|^2 ever added (certificate of the MFMA scan); device copy is the running atomic max
    float max_norm2 = 0.0f;
    DevBuf d_maxnorm;
    int flat_cert = 1;        // 1 = certify the fp16-MFMA scan and re-run uncertified queries exactly (0 = round-1 behaviour)

    // host-side bounds that only depend on the list lengths (top-nprobe sums of list / tile counts): computed once per
    // directory generation instead of a partial_sort over nlist two to four times per search batch
    uint64_t dir_gen = 0;
    std::map<std::tuple<int, int, int>, std::pair<uint64_t, std::pair<int64_t, int64_t>>> bound_cache;

    // two-call search (rsx_search_prepass / rsx_search_scan: the caller exchanges the per-query thresholds between the calls,
    // e.g. an all-reduce(MAX) across the ranks of a LIST-sharded index).  The search runs on a worker thread that parks right
    // after the threshold pre-pass (only the worker thread ever parks: TwoCall::worker); parked / go / done / tau are guarded by
    // TwoCall::mu, and every other entry point refuses the handle while `active` (refuse_while_two_call).
    struct TwoCall {
        std::thread th;
        std::thread::id worker;     // the thread running the parked search: the only one allowed to park
        std::mutex mu;
        std::condition_variable cv;
        bool active = false, parked = false, go = false, done = false;
        uint64_t* tau = nullptr; int64_t ntau = 0;
        int status = 0; std::string err;
    };
    std::unique_ptr<TwoCall> tc;

    // single-process multi-GPU handle (rsx_sharded_create): this object owns one child index per device and nothing else
    std::vector<rsx_index*> shards;
    DevBuf sh_D, sh_I, sh_q, sh_oD, sh_oI;      // parent-device gather / merge buffers
    int64_t sh_next_id = 0;                      // next sequential id of the logical index

    // rows a list's storage starts on and grows by: 64-vector slabs of PQ codes — 512 (a slice-major group of 16 blocks) in the sliced layout
    int row_align() const { return kind == KIND_IVFPQ ? (CB == PQ_SLICED ? 32 * PQ_SLICED_GB : 64) : (kind == KIND_FLAT ? 128 : 64); }
    size_t row_bytes() const { return kind == KIND_IVFPQ ? (size_t)Mpad : kind == KIND_IVFSQ ? (size_t)ld : (size_t)ld * (storage_f16 ? 2 : 4); }
};


// ---------------------------------------------------------------------------------------
// RSX1 file records (api_build.hip: save_impl / load_impl; api_sharded.hip re-shards a plain file while loading)
// ---------------------------------------------------------------------------------------
struct FileHeader {
    char magic[4];
    int32_t version, kind, d, metric, nlist, M, nbits, trained, storage_f16, custom_ids, nprobe;
    int64_t ntotal;
};
// version >= 2 appends: what a LIST shard (rsx_set_param "add_list_mod") needs to keep assigning the logical index's
// sequential ids after a reload — the vectors it saw but did not keep, and its (mod, rem)
struct FileHeaderV2 { int64_t ndropped; int32_t add_list_mod, add_list_rem; };

static inline void wr(FILE* f, const void* p, size_t n) {
    if (n && fwrite(p, 1, n, f) != n) RSX_THROW(RSX_ERR_IO, "short write");
}
static inline void rd(FILE* f, void* p, size_t n) {
    if (n && fread(p, 1, n, f) != n) RSX_THROW(RSX_ERR_IO, "short read (truncated index file)");
}

// ---------------------------------------------------------------------------------------
// host functions that cross files (definitions: see the file list above)
// ---------------------------------------------------------------------------------------
void use_device(rsx_index* h);
void refuse_while_two_call(const rsx_index* h, const char* what);
int64_t workspace_bytes(const rsx_index* h);
void upload_dir(rsx_index* h);
void ensure_capacity(rsx_index* h, const std::vector<int64_t>& need, bool exact);
const void* stage_rows(rsx_index* h, DevBuf& buf, const void* x, int64_t n, int d, int dtype);
void set_centroids(rsx_index* h, const float* c);
void set_codebooks(rsx_index* h, const float* c);
void set_sq_trained(rsx_index* h, const float* t);
void update_trained(rsx_index* h);
rsx_index* create_common(int kind, int d, int nlist, int M, int nbits, int metric, int device);
rsx_index* create_flat_pq(int d, int M, int nbits, int metric, int device);
rsx_index* create_ivfsq(int d, int nlist, int qtype, int metric, int by_residual, int device);
rsx_index* create_flat_sq(int d, int qtype, int metric, int device);
void sqflat_search(rsx_index* h, int64_t nq, const void* q, int dtype, int k, float* D, int64_t* I);      // api_sqflat.hip
void add_all(rsx_index* h, int64_t n, const void* x, int dtype, const int64_t* ids);
void train_impl(rsx_index* h, int64_t n, const void* x, int dtype);
void search_impl(rsx_index* h, int64_t nq, const void* q, int dtype, int k, float* D, int64_t* I);
void refine_impl(rsx_index* h, int64_t nq, const void* q, int dtype, int kc, const int64_t* labels, int k, float* D, int64_t* I);
void get_list_impl(rsx_index* h, int64_t l, int64_t* n_out, void* codes_out, int64_t* ids_out);
void add_list_impl(rsx_index* h, int64_t l, int64_t n, const void* codes, int dtype, const int64_t* ids);
void save_impl(rsx_index* h, const char* path);
rsx_index* load_impl(const char* path, int device);
rsx_index* sharded_create(int kind, int d, int nlist, int M, int nbits, int metric, int ndev, const int* devices);
void sharded_sync_trained(rsx_index* h);
void sharded_add(rsx_index* h, int64_t n, const void* x, int dtype, const int64_t* ids);
void sharded_search(rsx_index* h, int64_t nq, const void* q, int dtype, int k, float* D, int64_t* I);
void sharded_add_list(rsx_index* h, int64_t l, int64_t n, const void* codes, int dtype, const int64_t* ids);
void sharded_reserve(rsx_index* h, const int64_t* counts);
void sharded_save(rsx_index* h, const char* path);
void destroy_handle(rsx_index* h);
rsx_index* sharded_load(const char* path, int ndev, const int* devices);
int64_t remove_impl(rsx_index* h, const rsx_selector* s);
void release_direct_map(rsx_index* h);
void make_direct_map_impl(rsx_index* h, int type);
void reconstruct_impl(rsx_index* h, int64_t n, const int64_t* keys, int fill_negative, float* out);
int64_t sharded_remove(rsx_index* h, const rsx_selector* s);
void upgrade_storage_to_f32(rsx_index* h);
void merge_from_impl(rsx_index* dst, rsx_index* src, int64_t add_id);
void copy_subset_impl(rsx_index* src, rsx_index* dst, int subset_type, int64_t a1, int64_t a2);

// k_remove.hip: the removal kernels (mask: k_sel_mask, bit s = slot s is removed; slots of the moves are uint32: < 2^32 storage rows)
namespace rsx {
void launch_rm_ivf_plan_counts(const uint32_t* mask, const int64_t* base, const int64_t* len, int nlist, int64_t* new_len, int64_t* nmoves,
                               int64_t* move_off /* [nlist + 1] */, hipStream_t st);
void launch_rm_ivf_plan_moves(const uint32_t* mask, const int64_t* base, const int64_t* len, const int64_t* new_len, const int64_t* nmoves,
                              const int64_t* move_off, int nlist, uint32_t* move_src, uint32_t* move_dst, hipStream_t st);
void launch_rm_ivf_move(const uint32_t* move_src, const uint32_t* move_dst, const int64_t* nmoves_total, int64_t max_moves, uint8_t* data,
                        int64_t row_bytes, int pq, int Mpad, int CB, int64_t* ids, float* norms, hipStream_t st);
void launch_rm_clear(const int64_t* runs /* [nruns][first slot, count <= 256] */, int64_t nruns, uint8_t* data, int64_t row_bytes, int pq,
                     int Mpad, int CB, int64_t* ids, float* norms, hipStream_t st);
int64_t rm_flat_blocks(int64_t n);      // Flat: scan blocks of rm_flat_unit() slots
int64_t rm_flat_unit();
void launch_rm_flat_scan(const uint32_t* mask, int64_t n, int32_t* word_pre /* [ceil(n / 32)] */, int64_t* blk_cnt /* [blocks] */,
                         int64_t* blk_off /* [blocks + 1] */, hipStream_t st);
void launch_rm_flat_chunk(const uint32_t* mask, const int32_t* word_pre, const int64_t* blk_off, int64_t lo, int64_t hi, uint8_t* data,
                          int64_t row_bytes, int64_t* ids, float* norms, uint8_t* stage, int64_t* stage_ids, float* stage_norms, hipStream_t st);
}  // namespace rsx

static inline bool is_sharded(const rsx_index* h) { return !h->shards.empty(); }
// what this build does not offer on an IndexIVFScalarQuantizer handle: the message names the kind, the handle stays untouched
static inline void refuse_ivfsq(const rsx_index* h, const char* what) {
    if (h && h->flat_sq) RSX_THROW(RSX_ERR_UNSUPPORTED, "%s: not available on an IndexScalarQuantizer handle (kind 5) in this build", what);
    if (h && h->kind == KIND_IVFSQ) RSX_THROW(RSX_ERR_UNSUPPORTED, "%s: not available on an IndexIVFScalarQuantizer handle (kind 4) in this build", what);
}
// faiss.IndexScalarQuantizer handles (rsx_index::flat_sq) have no coarse quantiser: one list, a zero centroid
static inline void refuse_flat_sq(const rsx_index* h, int code, const char* what) {
    if (h && h->flat_sq) RSX_THROW(code, "%s: not available on an IndexScalarQuantizer handle (kind 5: a flat scalar quantiser, one list, no coarse quantiser)", what);
}
static inline int public_kind(const rsx_index* h) { return h->flat_pq ? 3 : h->flat_sq ? 5 : h->kind; }      // rsx_kind as callers and files see it

template <typename F>
static inline void for_each_shard_parallel(rsx_index* h, F&& f) {
    const size_t n = h->shards.size();
    std::vector<std::string> errs(n);
    std::vector<int> codes(n, 0);
    std::vector<std::thread> th;
    for (size_t r = 0; r < n; r++)
        th.emplace_back([&, r] {
            try { (void)hipSetDevice(h->shards[r]->device); f((int)r, h->shards[r]); }
            catch (const RsxError& e) { errs[r] = e.what(); codes[r] = e.code; }
            catch (const std::exception& e) { errs[r] = e.what(); codes[r] = RSX_ERR_INVALID; }
        });
    for (auto& t : th) t.join();
    for (size_t r = 0; r < n; r++)
        if (codes[r]) RSX_THROW(codes[r], "shard %zu (device %d): %s", r, h->shards[r]->device, errs[r].c_str());
}

