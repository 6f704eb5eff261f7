/*
 * rsx.h — C ABI of librsx.so, the MI355X (gfx950) dense-retrieval search engine.
 *
 * This is the drop-in boundary for the search path of RulinShao/retrieval-scaling.
 * In the reference every entry point below is a call into the third-party FAISS 1.8.0
 * SWIG module (the reference holds no search arithmetic of its own); the citation on each
 * function names the reference call site(s) it replaces (paths relative to the reference
 * repository root).
 *
 * Conventions
 *   - every function returns an int status: RSX_OK (0) or a negative rsx_status;
 *     rsx_last_error() returns a thread-local message for the last failure on this thread
 *     (FAISS raises C++ exceptions that SWIG turns into Python RuntimeError; the Python shim
 *     rsx.py raises RuntimeError(rsx_last_error()) in the same places).
 *   - plain pointers + sizes only; no torch / numpy types cross this boundary.
 *   - "x"/"q" pointers may be HOST or DEVICE (HBM) pointers; the library detects which with
 *     hipPointerGetAttributes.  Output D/I follow the same rule.  The caller owns inputs and
 *     outputs; the handle owns all device memory of the index; no pointer is retained
 *     past the call.
 *   - one in-flight call per handle; callable from any host thread (hipSetDevice per call).
 *   - vectors are row-major, C-contiguous [n, d]; dtype is RSX_F32 or RSX_F16.
 *   - search returns D float32 [nq,k], I int64 [nq,k]; unfilled slots I=-1 and
 *     D=-inf (inner product) / +inf (L2), exactly as faiss.Index.search does.
 */
#ifndef RSX_H
#define RSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsx_index rsx_index_t;

enum rsx_status {
    RSX_OK = 0,
    RSX_ERR_INVALID = -1,      /* bad argument (shape, dtype, k, null pointer) */
    RSX_ERR_NOT_TRAINED = -2,  /* add/search before train / set_centroids */
    RSX_ERR_HIP = -3,          /* HIP runtime failure (message has hipGetErrorString) */
    RSX_ERR_OOM = -4,          /* device or host allocation failed */
    RSX_ERR_IO = -5,           /* save/load failure */
    RSX_ERR_UNSUPPORTED = -6   /* valid FAISS request this build does not implement */
};

enum rsx_metric { RSX_METRIC_INNER_PRODUCT = 0, RSX_METRIC_L2 = 1 }; /* = faiss.METRIC_* */
enum rsx_dtype { RSX_F32 = 0, RSX_F16 = 1 };
enum rsx_kind { RSX_KIND_FLAT = 0, RSX_KIND_IVFFLAT = 1, RSX_KIND_IVFPQ = 2, RSX_KIND_PQ = 3, RSX_KIND_IVFSQ = 4, RSX_KIND_SQ = 5 };

/* Thread-local message of the last error raised on the calling thread ("" if none). */
const char* rsx_last_error(void);
/* ABI version (major*1000+minor). */
int rsx_version(void);
/* Number of visible HIP devices; fails with RSX_ERR_HIP when there is no usable GPU.
 * There is NO CPU fallback anywhere in this library. */
int rsx_device_count(int* n);

/* ---- construction ------------------------------------------------------------------ */

/* faiss.IndexFlatIP(d)                         — src/indicies/flat.py:42
 * (also the coarse quantiser object of ivf_flat.py:143 / ivf_pq.py:146, which this
 *  library folds into the IVF handles). Vectors are stored as fp16 when every added value
 *  is fp16-representable (the reference's embeddings are, src/embed.py:137-138), else fp32. */
int rsx_flat_create(int d, int metric, int device, rsx_index_t** out);

/* faiss.IndexIVFFlat(quantizer, d, nlist, METRIC_INNER_PRODUCT) — src/indicies/ivf_flat.py:144-148 */
int rsx_ivfflat_create(int d, int nlist, int metric, int device, rsx_index_t** out);

/* faiss.IndexIVFPQ(quantizer, d, nlist, M, nbits, METRIC_INNER_PRODUCT) — src/indicies/ivf_pq.py:147-153
 * by_residual = true (FAISS default). nbits must be 8.  The coarse quantiser is the reference's IndexFlatIP (ivf_pq.py:146) for
 * either metric.  RSX_METRIC_INNER_PRODUCT (what the reference passes) takes the certified 8-bit-table fast scans;
 * RSX_METRIC_L2 (round 6) ranks by the squared distance to the decoded vector c_l + r^ — a table per (query, list) pair, so it
 * is served by the exact scan (k_pq_scan_l2), every code layout, any k <= 4096 (tests/test_gpu_ivf.py::test_ivfpq_l2_metric_vs_oracle). */
int rsx_ivfpq_create(int d, int nlist, int M, int nbits, int metric, int device, rsx_index_t** out);

/* faiss.IndexPQ(d, M, nbits, METRIC_INNER_PRODUCT) — contriever/src/index.py:19,28-30,42,53,62 (the vendored Indexer behind
 * passage_retrieval.py --n_subquantizers; ric/conf/a100.yaml:67 index_type: PQ).  FAISS 1.8.0 IndexPQ: a flat product quantiser, no
 * coarse stage.  nbits must be 8, d % M == 0, d / M <= 160.  train = ProductQuantizer::train on the vectors themselves (the
 * library's subsample and seed); add = per-subspace nearest codeword, sequential ids (ids must be NULL: IndexFlatCodes has no
 * add_with_ids); search scores EVERY stored code with the query's table — inner product: the fp32 sum of the M table entries in
 * sub-quantiser order, best first; L2: squared distance to the decoded vector, ascending; equal scores by id ascending.
 * Both metrics take the staged filtered scan: every query scans every code against its 8-bit table in
 * stages over disjoint tile sets, the per-query threshold rising between stages, then the exact re-score and certificate of the
 * IVF-PQ fast scan; device memory beside the codes does not grow with ntotal.  Under L2 the table holds the NEGATED squared
 * sub-vector distances (the one list's centroid is zero, so the table is per query; the sum of its entries is bit for bit
 * -distance) and the fp32 tables of a batch are kept for the re-score (M KiB per query).  The layouts without a work-item scan
 * (granule; M not in {16, 32, 64, 96, 128}) take the exact scans; past 2 GiB of codes in the one list only the staged scan and the exact scans of the rotated / sliced layouts (and L2)
 * are served, any other routing of a search is refused (RSX_ERR_UNSUPPORTED).  rsx_get "kind" = RSX_KIND_PQ; list calls see ONE list (number 0) in insertion order.  Refused with a message:
 * selectors (RSX_ERR_UNSUPPORTED, as FAISS 1.8.0's IndexPQ::search refuses search parameters), rsx_remove_ids and sharded
 * handles of this kind (RSX_ERR_UNSUPPORTED), "add_list_mod", rsx_set_nprobe, rsx_assign, rsx_reserve_lists,
 * rsx_set_centroids / rsx_get_centroids (RSX_ERR_INVALID). */
int rsx_pq_create(int d, int M, int nbits, int metric, int device, rsx_index_t** out);

/* faiss.IndexIVFScalarQuantizer(quantizer, d, nlist, ScalarQuantizer.QT_8bit, metric, by_residual) — factory "IVF<nlist>,SQ8": one byte
 * per dimension, half of what IndexIVFFlat's fp16 rows take.  qtype must be 0 (QT_8bit: per-dimension range, RS_minmax
 * with argument 0); any other qtype is RSX_ERR_UNSUPPORTED (QT_fp16 rows are what rsx_ivfflat_create stores).  The coarse quantiser is
 * the inner-product one of the other IVF kinds for either metric; list membership is the argmax-IP list of x.  A stored vector is
 * x^ = the decoded code (by_residual = 0) or fl(c_l + the decoded residual) (by_residual = 1), and a search returns the canonical
 * Flat scores of the queries against x^ over the probed lists (fp64 accumulation, rounded once; squared L2 = distance to x^), ties by
 * id: a certified fp16-MFMA scan over the code bytes (k_sq_list_scan), exact re-score of the candidates from their decoded rows,
 * exact re-run of the queries the certificate cannot clear.  rsx_train trains the coarse quantiser, then the per-dimension minimum and
 * maximum - minimum over ALL training vectors (their residuals when by_residual) on the GPU; the handle is trained once centroids AND
 * parameters are present.  rsx_add_list / rsx_get_list carry uint8 [n, d] codes; rsx_get "kind" = RSX_KIND_IVFSQ, "code_size" = d,
 * plus "qtype" and "by_residual".  Refused with RSX_ERR_UNSUPPORTED and a message naming the kind: selectors, rsx_remove_ids, sharded
 * handles (rsx_sharded_create, rsx_load_sharded), the two-call search, "scan_chunk". */
int rsx_ivfsq_create(int d, int nlist, int qtype, int metric, int by_residual, int device, rsx_index_t** out);

/* faiss.IndexScalarQuantizer(d, ScalarQuantizer.QT_8bit, metric) - factory "SQ8": the flat sibling of rsx_ivfsq_create, an exhaustive
 * search over one code byte per dimension (half of what IndexFlat's fp16 rows take).  The reference has no call of it (its
 * flat backend is faiss.IndexFlatIP, src/indicies/flat.py:42); FAISS 1.8.0: IndexScalarQuantizer, an IndexFlatCodes.  qtype must be 0
 * (QT_8bit), any other is RSX_ERR_UNSUPPORTED.  rsx_train = the per-dimension minimum and maximum - minimum over ALL training vectors, on the
 * GPU; rsx_add encodes (sequential ids; ids must be NULL: IndexFlatCodes has no add_with_ids); a search returns the canonical Flat scores of
 * the queries against the DECODED vectors x^ (fp64 accumulation, rounded once; squared L2 = distance to x^), ties by id.  Batches of more
 * than 32 queries take a certified int8 matrix-core scan (k_sq_gemm: code - 128 against two int8 planes of the scaled query, exact i32
 * sums, staged filtered launches), exact re-score of the candidates from their decoded rows; the queries the certificate cannot clear are
 * searched again through the one-list route and, where that cannot clear them either, exactly; smaller batches take rsx_ivfsq_create's
 * one-list routes.  Every kernel over the one list addresses rows with 64 bits: more
 * than 2 GiB of codes are served.  rsx_get "kind" = RSX_KIND_SQ, "code_size" = d, "qtype"; list calls see ONE list (number 0) in insertion
 * order, uint8 [n, d]; rsx_set_sq_trained / rsx_get_sq_trained and rsx_reconstruct_batch (the key is the row) apply.  Refused with a
 * message naming the kind: selectors, rsx_remove_ids, rsx_range_search, the two-call search, sharded handles (RSX_ERR_UNSUPPORTED);
 * "add_list_mod", rsx_set_nprobe, rsx_assign, rsx_reserve_lists, rsx_set_centroids / rsx_get_centroids (RSX_ERR_INVALID).
 * rsx_set_param "sqflat_cand_cap" (this kind only): keys a query's candidate row holds per stage of the scan (0 = default).
 * rsx_get_timing: "sqflat_gemm_launches" (launches of the int8 scan), "sqflat_stages" (its filtered stages), "fallback_queries" (queries its
 * certificate could not clear), "sqflat_exact_queries" (of those, the ones that reached the exact scores). */
int rsx_sq_create(int d, int qtype, int metric, int device, rsx_index_t** out);

/* ONE handle over several GPUs of the node, single process — SURVEY.md 8(b)/(e).  The reference's offline driver makes one
 * index.search(all_queries, k) call (src/search.py:296) and its serving tier fans a query out to shard workers over HTTP and
 * re-sorts (api/serve_main_node.py:281-323); with this handle the same `Indexer(cfg).search` spans the node:
 *   kind: rsx_kind; nlist / M / nbits as for the single-device constructors (ignored where they do not apply);
 *   devices[ndev]: one shard per entry (an ordinal may repeat: several shards on one GPU).
 * train trains the first shard and copies the parameters; every add call is cut into ndev contiguous pieces (piece r ->
 * shard r) that keep the logical index's sequential ids, so the shards' lists are a partition of the single index's lists;
 * search runs every shard from its own host thread on its own device, copies the [nq, k] blocks to devices[0] and merges
 * them there by (score desc, id asc) — bit-identical to one index holding everything.  Every other entry point accepts the
 * handle (rsx_get "ntotal" sums the shards, knobs apply to all shards, "nshards" tells them apart) except the per-list
 * import / export calls.  rsx_save writes a manifest at `path` and one RSX1 file per shard beside it (path.shard<r>);
 * rsx_load_sharded reads them back onto the given devices (shard r -> devices[r % ndev]). */
int rsx_sharded_create(int kind, int d, int nlist, int M, int nbits, int metric, int ndev, const int* devices,
                       rsx_index_t** out);
int rsx_load_sharded(const char* path, int ndev, const int* devices, rsx_index_t** out);

/* Python garbage collection of the SWIG object (implicit in the reference). */
int rsx_destroy(rsx_index_t* h);

/* ---- training ---------------------------------------------------------------------- */

/* index.train(x)                               — src/indicies/ivf_flat.py:162,166; ivf_pq.py:166,170
 * Coarse k-means with an inner-product quantiser (assignment = argmax <x,c>, spherical
 * centroids, FAISS Level1Quantizer defaults: niter 10, <=256 points per centroid) and, for
 * IVFPQ, per-subspace k-means (256 codewords, niter 25) on residuals.
 * Assignment runs on the GPU; this also replaces the CUDA-only
 * index_cpu_to_gpu/GpuClonerOptions branch of ivf_flat.py:152-163. No-op for Flat. */
int rsx_train(rsx_index_t* h, int64_t n, const void* x, int dtype);

/* Import already-trained parameters (what faiss.read_index(<...>.trained) restores:
 * ivf_flat.py:170, ivf_pq.py:174).  centroids: [nlist, d] f32.  codebooks: [M, 256, d/M] f32. */
int rsx_set_centroids(rsx_index_t* h, const float* centroids);
int rsx_set_codebooks(rsx_index_t* h, const float* codebooks);
int rsx_get_centroids(rsx_index_t* h, float* centroids_out);
int rsx_get_codebooks(rsx_index_t* h, float* codebooks_out);
/* IVFSQ: the scalar quantiser's parameters, [2 d] f32 = vmin[d] then vdiff[d] (faiss ScalarQuantizer::trained). */
int rsx_set_sq_trained(rsx_index_t* h, const float* trained);
int rsx_get_sq_trained(rsx_index_t* h, float* trained_out);

/* ---- population -------------------------------------------------------------------- */

/* index.add(x)                                 — flat.py:58; ivf_flat.py:180; ivf_pq.py:185
 * ids == NULL assigns sequential ids ntotal .. ntotal+n-1 (the only form the reference uses).
 * IVF: list = argmax-IP centroid; IVFPQ: residual = x - centroid, code = per-subspace nearest
 * (L2) codeword, first minimum on ties; in-list order = insertion order. */
int rsx_add(rsx_index_t* h, int64_t n, const void* x, int dtype, const int64_t* ids);

/* index.quantizer.assign(x) (FAISS Index::assign on the coarse quantiser): list number of each vector,
 * argmax <x, centroid> (first maximum) — the same exact fp32 kernel `add` uses.  labels: int64 [n].
 * Lets a caller count list sizes first and rsx_reserve_lists exactly (needed when the index cannot hold
 * two copies of itself in HBM, e.g. 100M x 768 fp16 IVF-Flat = 153.6 GB). */
int rsx_assign(rsx_index_t* h, int64_t n, const void* x, int dtype, int64_t* labels);

/* index.reset(): drop every stored vector, keep the trained parameters and the HBM reservation. */
int rsx_reset(rsx_index_t* h);

/* Optional: pre-size every inverted list (counts[nlist]) so add never re-lays-out HBM. */
int rsx_reserve_lists(rsx_index_t* h, const int64_t* counts);

/* Bulk import of one inverted list (FAISS on-disk reader; InvertedLists::add_entries).
 * IVFPQ: codes [n, M] u8.  IVFFlat: codes = raw vectors [n, d] in `dtype`. */
int rsx_add_list(rsx_index_t* h, int64_t list_no, int64_t n, const void* codes, int dtype,
                 const int64_t* ids);

/* Export one inverted list (inspection / parity tests / writer).  Pass NULL to skip an output.
 * n_out: list length.  codes_out: IVFPQ [n,M] u8; IVFFlat/Flat [n,d] f32 (list_no ignored
 * for Flat).  ids_out: [n]. */
int rsx_get_list(rsx_index_t* h, int64_t list_no, int64_t* n_out, void* codes_out,
                 int64_t* ids_out);

/* len(list l) for every inverted list: sizes int64 [nlist] (Flat: one entry = ntotal).  Host pointer.  Used for the
 * list-length histogram SURVEY.md 8(d) asks the bench to report (FAISS: index.invlists.list_size(l)). */
int rsx_get_list_sizes(rsx_index_t* h, int64_t* sizes);

/* ---- search ------------------------------------------------------------------------ */

/* index.nprobe = probe                         — ivf_flat.py:73,149; ivf_pq.py:77,154 */
int rsx_set_nprobe(rsx_index_t* h, int nprobe);

/* index.search(x, k) -> (D, I)   THE HOT PATH  — flat.py:139; ivf_flat.py:225; ivf_pq.py:230
 * q: [nq, d] dtype; D: float32 [nq, k]; I: int64 [nq, k].
 * Result order: score descending (IP) / distance ascending (L2); equal scores by id ascending. */
int rsx_search(rsx_index_t* h, int64_t nq, const void* q, int dtype, int k, float* D, int64_t* I);

/* The same search in TWO calls, for callers that improve the per-query thresholds between the threshold pre-pass and the scan —
 * the LIST-sharded multi-GPU form (rsx_set_param "add_list_mod"): a rank that does not own a query's closest lists derives
 * a weak threshold from its own lists; after an all-reduce(MAX) of the threshold keys every rank filters as hard as the single
 * index would (the reference has no counterpart: its shards are independent indexes, src/search.py:282-303).
 *   rsx_search_prepass: starts rsx_search(h, nq, q, dtype, k, D, I) and returns once the thresholds are final on the device:
 *       *tau_dev = device pointer to nq uint64 keys (high word = order-preserving score bits: compare as unsigned; 0 = no
 *       threshold), valid until rsx_search_scan; *tau_dev = NULL, *ntau = 0 when this search has no pre-pass (Flat, exact
 *       modes, nprobe 1).  Any key may be RAISED to another valid lower bound of the query's k-th best score; nq must not
 *       exceed "query_batch".
 *   rsx_search_scan: runs the rest; D / I (given to the first call) are complete when it returns its status. */
int rsx_search_prepass(rsx_index_t* h, int64_t nq, const void* q, int dtype, int k, float* D, int64_t* I, uint64_t** tau_dev,
                       int64_t* ntau);
int rsx_search_scan(rsx_index_t* h);

/* Multi-shard merge of per-shard top-k       — src/search.py:362-367 (post_hoc_merge_topk),
 *                                               api/serve_main_node.py:150-163 (rerank_elements)
 * D,I: [nshards, nq, k].  Output [nq, k]: best first; ties keep the earlier shard first, then the
 * original within-shard order (Python's stable sorted(..., reverse=True)).  ids < 0 are padding.
 * Pointers may be host or device (all four on the same side).  Any shard count for k <= 8192: up to 16384 keys per
 * query merge in one launch, more (the reference backends' default k = 4096, src/indicies/flat.py:138, on 8 ranks) in
 * rounds over groups of consecutive shards with the same result. */
int rsx_merge_topk(int nshards, int64_t nq, int k, int metric, const float* D, const int64_t* I,
                   float* D_out, int64_t* I_out, int device);

/* The same merge for the in-node multi-GPU exchange (replaces the HTTP fan-in of api/serve_main_node.py:281-323):
 * rsx_pack_topk turns one rank's (D, I) [nq, k] into its packed [2, nq, k] int64 block (plane 0 = the score's
 * bits in the low word, plane 1 = ids + id_offset, padding ids < 0 kept) — ONE buffer per rank, so ONE
 * all-gather; rsx_merge_packed merges the gathered [nshards, 2, nq, k] buffer with rsx_merge_topk's rule.
 * Device pointers; both calls run on `stream` (a hipStream_t, NULL = the default stream) and do NOT
 * synchronise, so they can sit between the search and the collective on the caller's stream. */
int rsx_pack_topk(int64_t nq, int k, const float* D, const int64_t* I, int64_t id_offset, int64_t* packed,
                  int device, void* stream);
int rsx_merge_packed(int nshards, int64_t nq, int k, int metric, const int64_t* packed, float* D_out,
                     int64_t* I_out, int device, void* stream);

/* ---- introspection / knobs --------------------------------------------------------- */

/* Integer properties: "ntotal", "nlist", "d", "is_trained", "nprobe", "M", "nbits", "kind",
 * "metric", "storage_dtype", "code_size", "qtype" / "by_residual" (IVFSQ), "device", "max_k", "pq_layout" (IVFPQ: 1 = rotated code layout), "direct_map_type" (rsx_direct_map_type the handle holds now), "nshards"
 * (0 = single-device handle), "hbm_bytes", "explicit_ids" (1 = a Flat handle that stores caller ids, or any handle one of whose
 * rsx_add calls since the last rsx_reset carried ids).
 * (index.ntotal / index.is_trained — ivf_flat.py:171; ivf_pq.py:175) */
int rsx_get(rsx_index_t* h, const char* key, int64_t* out);

/* Tuning knobs that do not change results: "query_batch" (max queries per internal pass),
 * "scan_chunk" (vectors per scan work item, 0 = auto), "scan_kernel" (IVFPQ: 0 = auto, 1 = per-pair
 * v1 kernel, 2 = exact list-major kernel; non-zero disables the fast scan), "pq_fast" (IVFPQ: 1 = 8-bit-table
 * fast scan with certified exact re-rank [default], 0 = exact scan only; IndexPQ: 1 = the staged scan for inner product and L2,
 * 0 = the exact scan of its metric), "pq_fast_kp" (candidates kept by the
 * fast scan, 0 = auto), "pq_filter" (fast scan: 1 = candidates filtered inside the scan kernel [default], 0 = full
 * score buffer), "pq_pre_rows" (filtered fast scan: vectors of each query's closest list scored by the threshold
 * pre-pass, default 2048, 0 = one scan tile), "pq_tau_anchor" (filtered fast scan, four-query pre-pass: 1 = the threshold is anchored on the
 * exact scores of the sample's k best rows [default], 0 = the approximate k-th best minus 2 eps alone; read per search), "ivf_filter" (IVF-Flat: candidates filtered inside the list scan: 1 = when
 * the score rows of the batch would exceed ~2 GB [default], 2 = always, 0 = never = full score rows), "pq_prepass_fused" (filtered fast scan: 1 = threshold pre-pass in one launch [default], 0 = grouping +
 * scan + selection launches), "lut_tiled" (IVFPQ fast scan, dsub = 8: non-zero = 8-bit tables built by
 * tiles that share codebook slices among queries [default 2; inner product: on the matrix cores, IndexPQ L2: VALU tiles], 0 = one workgroup per query), "flat_filter" (Flat: 1 = one filtered GEMM launch after the first chunk [default], 0 = score buffer
 * per chunk), "pq_flat_first" / "pq_flat_growth" / "pq_flat_max_stages" (IndexPQ staged scan: rows of the first stage, 0 =
 * default; percent by which each stage outgrows the one before, 0 = default 300; most stages, 0 = default 12), "range_cand_cap" (rsx_range_search: keys a query's candidate row holds in the first scan, 0 = default 65536), "profile" (1 = record stage timings with HIP
 * events on the library's stream; 2 = additionally count the vectors each search scanned). */
/* Build-time knob (IVF indexes, before the first add): "add_list_mod" = N, "add_list_rem" = r make this handle a LIST
 * shard of an N-way multi-GPU index: rsx_add assigns every vector of the stream (sequential ids keep counting all
 * of them) but stores only those whose inverted list l has l % N == r.  N handles fed the same stream, searched with
 * the same queries and merged (rsx_merge_topk / rsx_merge_packed) return the single index's result; unlike vector
 * shards, every rank then scans whole lists for 1/N of the (query, probe) pairs. */
int rsx_set_param(rsx_index_t* h, const char* key, double value);

/* HIP-event timings (ms) of the stages of the last rsx_search on this handle when
 * "profile"=1: "coarse", "select_probe", "lut", "scan", "select", "finalize", "total",
 * "scan_launches", "fast_queries", "fallback_queries" (certificate failures re-run exactly), "pq_flat_stages" (IndexPQ: stages
 * of the staged filtered scan, summed over the internal batches) and (profile 2) "scanned_vectors", "cand_keys", "cand_keys_max".  Used by bench.py for the roofline object. */
int rsx_get_timing(rsx_index_t* h, const char* key, double* ms);

/* ---- filtered search (FAISS SearchParameters with an IDSelector) ------------------- */

/* faiss.IDSelector* (FAISS 1.8.0 impl/IDSelector.h): the ids a search may return.  Pure host object: needs no GPU.
 *   RSX_SEL_RANGE  faiss.IDSelectorRange(lo, hi)      ids in [lo, hi)                              (data, n ignored)
 *   RSX_SEL_BATCH  faiss.IDSelectorBatch(n, data)     the n int64 ids at data; duplicates allowed   (lo, hi ignored)
 *   RSX_SEL_BITMAP faiss.IDSelectorBitmap(n, data)    n bytes at data: id i is selected when 0 <= i < 8 n and
 *                                                     bit (i & 7), least significant first, of byte i >> 3 is set
 *   invert != 0    faiss.IDSelectorNot(sel)           the complement of the above
 * data is a HOST or DEVICE pointer; it is copied, nothing is retained.  The reference has no filtered search: its
 * datastore subsampling (src/search.py:493-500) and decontamination (src/search.py:519-523) drop documents after it. */
enum rsx_selector_kind { RSX_SEL_RANGE = 0, RSX_SEL_BATCH = 1, RSX_SEL_BITMAP = 2 };
typedef struct rsx_selector rsx_selector_t;
int rsx_selector_create(int kind, const void* data, int64_t n, int64_t lo, int64_t hi, int invert, rsx_selector_t** out);
int rsx_selector_destroy(rsx_selector_t* sel);
/* sel.is_member(id) for n ids (host pointers): out[i] = 0 / 1.  Host code, no GPU. */
int rsx_selector_is_member(const rsx_selector_t* sel, int64_t n, const int64_t* ids, uint8_t* out);

/* index.search(x, k, params=faiss.SearchParameters(sel=sel))           (Flat)
 * index.search(x, k, params=faiss.SearchParametersIVF(sel=sel, nprobe=p)) (IVF-Flat / IVF-PQ)
 * Returns exactly what rsx_search returns on an index holding only the selected vectors (same trained parameters, ids
 * and insertion order); slots that cannot be filled get I = -1 and D = -inf (IP) / +inf (L2).  sel may be NULL (no
 * selection).  nprobe_override > 0 replaces the handle's nprobe for this call only (IVF; ignored by Flat); 0 keeps it.
 * A filtered search takes the routes whose scans write complete score rows, the unselected rows masked out of them (DESIGN.md
 * section 7b); the slot mask of a selector is built once per (selector, index state) and cached on the handle: rsx_get_timing
 * "sel_mask_builds", "sel_mask_ms", "filtered_queries".
 * Sharded handles apply the selector, over the logical index's ids, to every shard. */
int rsx_search_sel(rsx_index_t* h, int64_t nq, const void* q, int dtype, int k, const rsx_selector_t* sel,
                   int nprobe_override, float* D, int64_t* I);
/* rsx_search_prepass with a selector and an nprobe override (rsx_search_scan finishes it).  The filtered search has no
 * threshold pre-pass: *tau_dev = NULL, *ntau = 0 whenever sel is not NULL. */
int rsx_search_prepass_sel(rsx_index_t* h, int64_t nq, const void* q, int dtype, int k, const rsx_selector_t* sel,
                           int nprobe_override, float* D, int64_t* I, uint64_t** tau_dev, int64_t* ntau);

/* ---- exact re-ranking (FAISS IndexRefineFlat) -------------------------------------- */

/* IndexFlat::compute_distance_subset followed by IndexRefine::search's re-order: re-score the kc candidate labels of every query
 * exactly against the rows a Flat handle stores and keep the best k.  The reference holds the same idea as dead code
 * (get_knn_scores re-scores retrieved ids from the raw embeddings, src/indicies/ivf_pq.py:119-123); rsx.IndexRefineFlat puts it
 * behind a compressed index: search the base for k * k_factor candidates, refine, keep k.
 *   flat     a Flat handle of sequential ids: a label is the position of a stored row (fp16 or widened fp32 storage alike);
 *   q        [nq, d] dtype;  labels  int64 [nq, kc];  D float32 [nq, k];  I int64 [nq, k];  1 <= k <= kc <= 4096.
 * Score: fp64 accumulation of the exact products, rounded once to fp32 (what rsx_search on the Flat handle returns for that row);
 * inner product: the score, best first; L2: the squared distance, ascending; equal scores by label ascending.  Labels < 0 (the
 * padding of a base search) are skipped; a label that occurs twice is scored twice and may be returned twice, next to itself (as
 * FAISS's compute_distance_subset + reorder_2_heaps would); slots that cannot be filled get I = -1 and D = -inf (IP) / +inf (L2).
 * A label >= ntotal is never dereferenced: it is skipped, the call returns RSX_ERR_INVALID once its work has finished, and D / I are
 * unspecified.  q, labels and D / I follow rsx_search's host / device rule, each on its own (D and I on the same side).  One
 * kernel launch per "query_batch" queries (k_refine: one workgroup per query) on the handle's stream; the call may directly follow an
 * rsx_search on another handle of the same device that produced `labels` (rsx_search returns with its results complete).
 * Refused with the handle untouched: a handle that is not Flat (RSX_ERR_INVALID), a Flat handle with explicit ids or a sharded one,
 * kc > 4096 (RSX_ERR_UNSUPPORTED), k < 1 or k > kc (RSX_ERR_INVALID).  rsx_get_timing: "refine_calls", "refine_candidates" (nq * kc,
 * summed) and, with "profile" = 1, "refine_ms" (HIP events around the call's launches). */
int rsx_refine(rsx_index_t* flat, int64_t nq, const void* q, int dtype, int kc, const int64_t* labels, int k, float* D, int64_t* I);

/* ---- stored vectors by id (FAISS Index::reconstruct*) ------------------------------- */

/* DirectMap::Type of FAISS 1.8.0 (invlists/DirectMap.h): the map from a stored id to its storage row. */
enum rsx_direct_map_type { RSX_DM_NOMAP = 0, RSX_DM_ARRAY = 1, RSX_DM_HASHTABLE = 2 };

/* IndexIVF::make_direct_map(new_maintain_direct_map) / IndexIVF::set_direct_map_type(type) -> DirectMap::set_type: build the map
 * at once (type 1 or 2) or release it (type 0).
 *   RSX_DM_ARRAY      int64 map[ntotal], 8 B per vector: taken when every stored id lies in [0, ntotal) once (sequential ids in any
 *                     list order, a permutation given through rsx_add's ids); otherwise the build falls back to the hash table
 *                     (FAISS throws instead);
 *   RSX_DM_HASHTABLE  open addressing over (id, row) slots of 16 B, capacity the power of two >= 2 ntotal: 32 - 64 B per vector.
 * The type asked for is kept for later builds; rsx_get "direct_map_type" tells what the handle holds now (0 = nothing).
 * DIFFERENCE FROM FAISS: IndexIVF::reconstruct throws before make_direct_map; here the first rsx_reconstruct_batch builds the map
 * (Array where the ids allow it), so this call is an optimisation of WHEN, never a requirement.  The map is derived data, counted in
 * rsx_get "workspace_bytes": rsx_add, rsx_add_list, rsx_remove_ids, rsx_reset, rsx_reserve_lists and every re-layout RELEASE it
 * (FAISS maintains it across add), the next lookup builds it again.  The build checks hipMemGetInfo first: without
 * room it fails with RSX_ERR_OOM and the handle stays usable.  An id stored more than once resolves to its copy in the LOWEST
 * storage row: the first in (list number, in-list offset) order.  A Flat handle of sequential ids and an IndexPQ handle need no
 * map (the key is the row): the call succeeds and "direct_map_type" stays 0.  rsx_get_timing: "direct_map_builds",
 * "direct_map_ms" (host wall time).  Refused: sharded handles (RSX_ERR_UNSUPPORTED), an unknown type (RSX_ERR_INVALID). */
int rsx_make_direct_map(rsx_index_t* h, int type);

/* Index::reconstruct_batch(n, keys, recons) — and with it Index::reconstruct (n = 1), Index::reconstruct_n (keys i0 .. i0 + n - 1) and
 * the gather of Index::search_and_reconstruct (keys = the labels of a search, fill_negative = 1).  The reference serves the same need
 * from host RAM: get_embs(indices) / get_knn_scores(query_emb, indices) index a resident self.embs array
 * (src/indicies/ivf_flat.py:109-123, ivf_pq.py:112-123, flat.py:90); here the vectors come from what the index keeps in HBM.
 *   keys int64 [n]: ids, the labels rsx_search returns, in any order, repeats allowed;  out float32 [n, d];  keys and out are HOST or
 *   DEVICE pointers, each on its own.  out[i] is the vector the index STORES for keys[i] — what an exact search scores against:
 *     Flat, IVF-Flat   the stored row (fp16 rows widened, which is exact; fp32 rows as they are);
 *     IVF-PQ           x^_j = fl32(c_list[j] + codebook[m][code_m][t]), j = m dsub + t (IndexIVFPQ::reconstruct_from_offset): the
 *                      DECODED vector, not the one that was added;
 *     IndexPQ          the codebook entries alone, nothing added (ProductQuantizer::decode); a key is the position of the vector;
 *     IVF-SQ           the decoded code, with by_residual the list's centroid added and the sum rounded once (rsx_ivfsq_create's x^).
 *   fill_negative != 0: a key < 0 (the padding label of a search) gives a row whose every bit is set (FAISS: memset(-1); reads as NaN).
 * A key that is not stored (and a key < 0 without fill_negative) is never dereferenced: the call returns RSX_ERR_INVALID once its work
 * has finished, the message names the first such key, out is unspecified and the handle stays usable (DirectMap::get throws as well).
 * n = 0 succeeds and touches nothing.  One k_reconstruct launch (one wave per key) per 64 MiB of host output, or per call for device
 * output, on the handle's stream; the call may directly follow the rsx_search that produced the keys.  The id -> row map is built by
 * the first call that needs it (rsx_make_direct_map).  rsx_get_timing: "reconstruct_calls", "reconstruct_keys".
 * Refused with the handle untouched: sharded handles (RSX_ERR_UNSUPPORTED), n < 0, a null pointer with n > 0 (RSX_ERR_INVALID). */
int rsx_reconstruct_batch(rsx_index_t* h, int64_t n, const int64_t* keys, int fill_negative, float* out);

/* ---- vector transforms (FAISS VectorTransform / LinearTransform) --------------------- */

/* faiss.LinearTransform and its subclasses (RandomRotationMatrix, PCAMatrix, OPQMatrix) as the library sees them: a matrix A
 * float32 [d_out, d_in] row-major and an optional bias b [d_out] on one device, applied on the GPU (k_vt_apply).
 * The reference has no transform; FAISS applies it on the CPU in front of an index (IndexPreTransform; factory "OPQ96,..." / "PCA256,..."). */
typedef struct rsx_vt rsx_vt_t;

int rsx_vt_create(int device, int d_in, int d_out, rsx_vt_t** out);
/* A [d_out, d_in] and b [d_out] or NULL (no bias): HOST float32 arrays, copied; replaces what an earlier call set.  Uploads A, its
 * transposed copy (the reverse transform's operand) and b. */
int rsx_vt_set(rsx_vt_t* vt, const float* A, const float* b_or_null);
/* reverse = 0, LinearTransform::apply:  x [n, d_in] (dtype RSX_F32 or RSX_F16) -> y float32 [n, d_out],
 *     y_j = fl32(s_j + b_j),  s_j = fmaf(x[t], A[j][t], s) for t = 0 .. d_in - 1 from +0  (fp16 widened exactly; no bias: y_j = s_j);
 * reverse != 0, LinearTransform::transform_transpose (the inverse of an orthonormal A; the caller checks that):  x [n, d_out] ->
 * y float32 [n, d_in],  y_t = fmaf(fl32(x[j] - b_j), A[j][t], s) for j = 0 .. d_out - 1 from +0.
 * Both are one sequential fp32 chain per output, bit for bit reproducible (f32-input MFMA).  x and y are HOST or DEVICE pointers, each
 * on its own; a host operand is staged through at most 64 MiB of device memory per chunk.  Runs on the handle's own stream and
 * returns when the work is complete; device inputs must be complete when the call is made.  n = 0 succeeds and touches nothing.
 * RSX_ERR_NOT_TRAINED before rsx_vt_set; RSX_ERR_INVALID: n < 0, a bad dtype, a null pointer with n > 0. */
int rsx_vt_apply(rsx_vt_t* vt, int64_t n, const void* x, int dtype, float* y, int reverse);
/* NULL is accepted */
int rsx_vt_destroy(rsx_vt_t* vt);

/* ---- range search (FAISS Index::range_search) -------------------------------------- */

/* faiss RangeSearchResult: the library-owned answer of one rsx_range_search, whose size is known only after the scan.  It lives in
 * DEVICE memory (on the handle's device) when the queries were a device pointer, else in host memory; it stays valid until
 * rsx_range_result_destroy and does not depend on the handle. */
typedef struct rsx_range_result rsx_range_result_t;

/* Index::range_search(n, x, radius, result) of IndexFlat / IndexFlatIP / IndexFlatL2 and IndexIVFFlat (sequential and explicit ids):
 * every stored vector within the radius of every query.  The reference has no call of it (its thresholds are applied after a top-k
 * search, src/search.py:519-527); FAISS's GPU indexes do not offer it.  DESIGN.md section 7g.
 *   membership  inner product: score > radius;  L2: squared distance < radius — strict, in fp32, on the canonical exact value (fp64
 *               accumulation of the exact products, rounded once: what rsx_search returns for that row).  IVF-Flat compares the rows
 *               of the query's nprobe probed lists, the probes rsx_search would take; nprobe_override > 0 replaces the handle's nprobe
 *               for this call (ignored by Flat), 0 keeps it.  A query with a NaN or infinite component owns nothing.
 *   order       inside a query best first, equal values by id ascending (FAISS leaves the order open).
 *   exactness   every result is exact — there is no uncertified outcome: the scans' fixed per-query threshold admits every member
 *               (the proven bound of the fp16 scans plus rounding margins), an exact re-score decides.  A query with more candidates
 *               than a first-pass row holds ("range_cand_cap" keys, default 65536, rounded up to a power of two) is scanned again
 *               with a row sized from its count, in groups that fit "temp_budget_mb"; a row that cannot fit ends the call with
 *               RSX_ERR_OOM and leaves the handle usable.
 * nq = 0 gives lims = [0]; an empty index all-zero lims.  RSX_ERR_INVALID: a non-finite radius, an open two-call search.
 * RSX_ERR_UNSUPPORTED, the handle untouched: IVF-PQ, IndexPQ and IndexIVFScalarQuantizer handles, sharded handles, an IVF-Flat
 * handle whose rows had to be widened to fp32 (no filtered list scan).  rsx_get_timing: "range_candidates", "range_results",
 * "range_overflow_queries" (summed over the calls) and, with "profile" > 0, "range_ms" / "range_backend_ms" (HIP events). */
int rsx_range_search(rsx_index_t* h, int64_t nq, const void* q, int dtype, float radius, int nprobe_override, rsx_range_result_t** out);
/* The fields of a RangeSearchResult (any out pointer may be NULL): nq; total = lims[nq]; on_device (1: lims / D / I are device pointers);
 * lims int64 [nq + 1] with lims[0] = 0 (FAISS: size_t) — query i owns D[lims[i] .. lims[i + 1]) float32 (RangeSearchResult::distances)
 * and I[..] int64 (RangeSearchResult::labels).  D and I are NULL when total = 0. */
int rsx_range_result_get(const rsx_range_result_t* r, int64_t* nq, int64_t* total, int* on_device, const int64_t** lims, const float** D,
                         const int64_t** I);
/* delete of a RangeSearchResult; NULL is accepted */
int rsx_range_result_destroy(rsx_range_result_t* r);

/* ---- removal (FAISS Index::remove_ids) --------------------------------------------- */

/* index.remove_ids(sel) -> number of vectors removed (*nremoved), FAISS 1.8.0 semantics:
 *   IVF-Flat / IVF-PQ  IndexIVF::remove_ids -> DirectMap::remove_ids (NoMap): per list, each removed entry j takes the
 *                      list's last entry (j = 0, l = len; while j < l: if sel(ids[j]) entry[j] = entry[--l] else j++) —
 *                      the in-list order get_list and write_index see is the one FAISS leaves;
 *   Flat               IndexFlatCodes::remove_ids: sel tests the POSITION, the kept rows are compacted in order and the ids
 *                      renumbered 0 .. ntotal - 1;  Flat with explicit ids (IndexIDMap::remove_ids): sel tests the stored
 *                      id, rows and ids are compacted in order.
 * Later adds without ids number from the new ntotal, as in FAISS; on an IVF index those ids can equal surviving ones (FAISS
 * behaves the same way).  Trained parameters, list capacities and the storage dtype do not change; the vacated slots are
 * reset to zero bytes.  Removing nothing returns 0 and leaves the index untouched.  Runs on the GPU: slot mask (k_sel_mask),
 * per-list plan and one in-place move pass (IVF) or a stable compaction staged through at most max(256 MiB, payload / 16)
 * of device memory (Flat); rsx_get_timing "remove_calls", "removed", "remove_ms" (host wall time).
 * The reference drops documents after every search instead — subsampling (src/search.py:493-500) and decontamination /
 * short chunks (src/search.py:519-527): removing them once keeps all n_docs slots for the remaining documents.
 * Sharded handles (rsx_sharded_create / rsx_load_sharded) remove on every shard in parallel: IVF kinds, and Flat when its
 * adds carried ids.  Refused (RSX_ERR_UNSUPPORTED): a sharded Flat handle of sequential ids (faiss.IndexShards has no
 * remove_ids), a list shard ("add_list_mod" > 1).  Refused (RSX_ERR_INVALID): NULL arguments, an open two-call search. */
int rsx_remove_ids(rsx_index_t* h, const rsx_selector_t* sel, int64_t* nremoved);

/* ---- joining and splitting indexes (ABI 1010) --------------------------- */
/* InvertedLists::subset_type_t of FAISS 1.8.0 (invlists/InvertedLists.h). */
enum rsx_subset_type {
    RSX_SUBSET_TYPE_ID_RANGE = 0,          /* a1 <= id < a2 */
    RSX_SUBSET_TYPE_ID_MOD = 1,            /* id % a1 == a2 */
    RSX_SUBSET_TYPE_ELEMENT_RANGE = 2,     /* elements a1 .. a2 - 1 of ntotal, split evenly over the lists */
    RSX_SUBSET_TYPE_INVLIST_FRACTION = 3,  /* refused */
    RSX_SUBSET_TYPE_INVLIST = 4            /* refused */
};

/* dst.merge_from(src, add_id) — replaces FAISS 1.8.0's IndexIVF::merge_from (IVF-Flat, IVF-PQ in every code layout and any pair of
 * layouts, IVF-SQ), IndexFlatCodes::merge_from (Flat with sequential ids, IndexPQ, IndexScalarQuantizer: add_id must be 0, else
 * "cannot set ids in FlatCodes index"; src's vector i becomes id ntotal + i) and IndexIDMap::merge_from (Flat with explicit ids: both
 * sides carry explicit ids, or dst is empty and adopts src's id mode).  Every list of src is appended behind dst's in src's order,
 * ids stored as id + add_id, dst.ntotal grows by src.ntotal and src ends EMPTY (as after rsx_reset: trained, capacity kept).  The
 * result is what one index that was fed everything holds: lists, ids and search results bit for bit.  Runs on the device (k_merge.hip);
 * nothing passes through the host.  Flat / IVF-Flat: fp32 rows on either side leave dst with fp32 rows (fp16 rows are widened inside
 * the copy).  The certificate maxima take the larger of both sides; L2 norm terms are copied.  The direct map and the row-major code
 * copy of both handles are released.  rsx_get "explicit_ids" of dst stays 0 only when neither side had explicit ids and add_id equals
 * dst's ntotal before the call (what sequential adds would have stored).
 * Checked BEFORE anything is touched — a refused call leaves both handles as they were: dst != src; the same kind, d, metric, nlist,
 * M, nbits, qtype, by_residual; both trained; centroids, codebooks and scalar-quantiser parameters BIT-EQUAL (FAISS compares the
 * sizes only); both unsharded, on one device, outside an open two-call search, no list shard ("add_list_mod" > 1).
 * Memory: when a list of dst overflows, dst is laid out again and dst old, dst new and src exist at once; rsx_reserve_lists on dst
 * beforehand avoids that.  hipMemGetInfo is checked first (RSX_ERR_OOM, both handles untouched).
 * rsx_get_timing (dst): "merge_relayouts", "merge_rows", "merge_copy_ms" (host wall time of the copy). */
int rsx_merge_from(rsx_index_t* dst, rsx_index_t* src, int64_t add_id);

/* src.copy_subset_to(dst, subset_type, a1, a2) — replaces FAISS 1.8.0's IndexIVF::copy_subset_to (InvertedLists::copy_subset_to): IVF
 * kinds only.  src is unchanged; dst gains the selected entries of every list behind its own, in list order, ids unchanged; dst.ntotal
 * grows by their number.  Types 0 and 1 test the stored id; type 2 is FAISS's running split over the lists in order, so consecutive
 * (a1, a2) ranges partition every list.  Types 3 and 4 are refused (RSX_ERR_UNSUPPORTED, the message names the type); so are a1 > a2
 * (type 0), a1 <= 0 or a2 outside [0, a1) (type 1), a range outside [0, ntotal] (type 2) (RSX_ERR_INVALID).  The compatibility rules
 * of rsx_merge_from apply.  The per-list counts of types 0 / 1 are the call's only read-back. */
int rsx_copy_subset_to(rsx_index_t* src, rsx_index_t* dst, int subset_type, int64_t a1, int64_t a2);

/* ---- persistence ------------------------------------------------------------------- */

/* faiss.write_index(index, path) / faiss.read_index(path)
 *   — flat.py:39,63,69; ivf_flat.py:71,167,170,185; ivf_pq.py:75,171,174,190
 * Native container (magic "RSX1"); the FAISS .faiss reader lives in the Python host layer. */
int rsx_save(rsx_index_t* h, const char* path);
int rsx_load(const char* path, int device, rsx_index_t** out);

/* ---- synthetic data (bench / tests) ------------------------------------------------ */

/* Deterministic Gaussian-mixture generator, bit-identical to oracle/orc_synth (integer hash +
 * Irwin-Hall normal approximation, no transcendental functions):
 *   centre(j)[t]   = 1.0 * z(seed_c, j, t)
 *   vector(i)[t]   = fp16( centre(h(seed_x,i) % ncentres)[t] + sigma * z(seed_x, i, t) )
 * writes rows [i0, i0+n) as fp16 into `out` (host or device pointer, [n, d] fp16). */
int rsx_synth_vectors(int device, int d, int ncentres, uint32_t seed_c, uint32_t seed_x,
                      float sigma, int64_t i0, int64_t n, void* out_f16);
/* queries: q(r) = fp16( vector(h(seed_q, r) % nbase) + sigma_q * z(seed_q, r, t) ) */
int rsx_synth_queries(int device, int d, int ncentres, uint32_t seed_c, uint32_t seed_x,
                      float sigma, int64_t nbase, uint32_t seed_q, float sigma_q, int64_t r0,
                      int64_t n, void* out_f16);

#ifdef __cplusplus
}
#endif
#endif /* RSX_H */
