// k_range.hip — the kernels of range search (rsx_range_search) around the existing fixed-threshold scans:
//   k_range_tau      per query |q| and the scan threshold that admits every member of the result
//   k_range_rescore  exact re-score of every candidate (k_rescore.h's arithmetic) and the membership test, in place
//   k_range_sort     every candidate row in descending key order: members first, best first; rows of any length (bitonic network, LDS tiles
//                    of 4096 keys, the strides beyond a tile through global memory)
//   k_range_lims     exclusive scan of the member counts
//   k_range_emit / k_range_ties   D and I at lims[q]; runs of equal scores reordered by id where ids are not the scan's indices
//   k_range_compact / k_range_gather_rows   what the second pass of overflowed queries needs
#include "rsx_range.h"
#include "k_rescore.h"

namespace rsx {

// ---------------------------------------------------------------------------------------
// The threshold.  The scans rank a stored vector x by r = <q, x> (inner product) or r = <q, x> - |x|^2 / 2 (L2: |q - x|^2 = |q|^2 - 2 r) and
// compute r~ with |r~ - r| <= eps = rel |q| xmax + cert_abs (|q| + xmax) (api_stages.hip: scan_cert_bound; k_finalize forms the same
// expression, and so does this kernel, in fp32 with qn >= |q|).  Membership is decided on the canonical value c = fl32(v), v the fp64 sum:
//   inner product:  c > radius.  Rounding to nearest is monotone and radius is an fp32 number, so c > radius implies v > radius; v differs
//                   from the real <q, x> by the fp64 accumulation, at most d 2^-53 |q| |x|.  On top of that one fp32 rounding of the score
//                   (2^-24 |q| xmax) is given away, so that nothing rests on the monotonicity argument alone:
//                       r >= radius - 2^-23 |q| xmax       for every member
//   L2:             c < radius, hence v < radius likewise, and the real distance D < radius (1 + 2^-22) with the same allowances (radius > 0;
//                   no member otherwise); r = (|q|^2 - D) / 2:
//                       r > (|q|^2 - radius - 2^-22 |radius|) / 2
// A member therefore has r~ >= t = (that bound) - eps.  t is formed in fp64 from the fp32 eps (relative error 2^-52 per operation, covered by
// 2^-40 of the magnitudes involved), rounded DOWN to fp32, and emitted as the key just below (t, any index): key > tau admits every index
// at score t.  A query with a non-finite |q|^2 (a NaN or infinite component) gets the largest key: nothing passes, it owns nothing.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_range_tau(RangeTauArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.nq) return;
    const float* qv = a.Q32 + q * a.ldq;
    double q2 = 0.0;
    for (int t = lane; t < a.d; t += 64) q2 += (double)qv[t] * (double)qv[t];
    q2 = wave_sum_f64(q2);
    if (lane != 0) return;
    uint64_t key = ~0ull;
    if (q2 < (double)__builtin_inff()) {        // false for NaN
        const float qn = (float)sqrt(q2) * 1.0000002f;
        const float rel = a.cert_rel + ((a.cert_qflag && *a.cert_qflag) ? a.cert_rel_qlossy : 0.0f);
        const float eps = rel * qn * a.cert_xmax + a.cert_abs * (qn + a.cert_xmax);
        const double rad = (double)a.radius, qx = (double)qn * (double)a.cert_xmax;
        double t;
        if (a.metric == 0) t = rad - 1.1920928955078125e-7 * qx;
        else t = 0.5 * (q2 - rad - 2.384185791015625e-7 * fabs(rad));
        t -= (double)eps;
        t -= 9.094947017729282e-13 * (fabs(t) + q2 + fabs(rad) + qx + (double)eps);
        float tf = (float)t;
        if ((double)tf > t) tf = nextafterf(tf, -__builtin_inff());
        tf = tf + 0.0f;
        key = tf == tf ? (((uint64_t)f2ord(tf)) << 32) - 1ull : 0ull;       // (t = NaN cannot happen for a finite radius; 0 would admit everything)
    }
    a.tau[q] = key;
    a.cand_cnt[q * CCS] = 0ull;
}
void launch_range_tau(const RangeTauArgs& a, hipStream_t st) {
    if (a.nq <= 0) return;
    hipLaunchKernelGGL(k_range_tau, dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, st, a);
}

__device__ inline int range_pow2ceil(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// storage row of the candidate with index idx of query q (k_finalize's resolve)
__device__ inline int64_t range_row_of(int kind, uint32_t idx, int64_t q, const int32_t* probe_list, const int64_t* seg_start, int nprobe,
                                       const int64_t* list_base) {
    if (kind == KIND_FLAT) return (int64_t)idx;
    const int64_t* ss = seg_start + q * (nprobe + 1);
    int lo = 0, hi = nprobe;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ss[mid] <= (int64_t)idx) lo = mid; else hi = mid; }
    return list_base[probe_list[q * nprobe + lo]] + ((int64_t)idx - ss[lo]);
}

// ---------------------------------------------------------------------------------------
// Exact re-score and membership.  Workgroup (chunk, row): 256 candidates of one row; their storage rows are re-scored by rescore_rows (one
// wave per candidate, four in flight per wave: random reads of 2 d bytes), then a candidate whose canonical score passes the strict test
// keeps the key (exact order word, index) and every other slot of the chunk becomes 0.  The chunk grid covers the row up to the power of two
// the sort pads it to.
// ---------------------------------------------------------------------------------------
#define RANGE_RC 256
__global__ __launch_bounds__(256) void k_range_rescore(RangeRowsArgs a) {
    __shared__ int64_t srow[RANGE_RC];
    __shared__ uint32_t sord[RANGE_RC];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t r = blockIdx.y;
    const int n = a.rcnt[r];
    if (n <= 0) return;
    const int n2 = range_pow2ceil(n);            // <= cap: n <= cap and cap is a power of two
    const int c0 = (int)blockIdx.x * RANGE_RC;
    if (c0 >= n2) return;
    const int64_t q = a.qsel ? a.qsel[r] : r;
    uint64_t* row = a.cand + r * (int64_t)a.cap;
    const int c = c0 + tid;
    const uint64_t key = c < n ? row[c] : 0ull;
    const uint32_t idx = key_idx(key);
    srow[tid] = key ? range_row_of(a.kind, idx, q, a.probe_list, a.seg_start, a.nprobe, a.list_base) : -1;
    sord[tid] = 0u;
    __syncthreads();
    const int c_hi = n - c0 < RANGE_RC ? (n - c0 > 0 ? n - c0 : 0) : RANGE_RC;
    rescore_rows(a.X, a.x_f16, a.ld, a.d, a.metric, a.Q32 + q * a.ldq, a.ldq, INT64_MAX, srow, sord, 0, c_hi, lane, wv, 4);
    // strict, in fp32: score > radius; L2: the order word holds 0 - distance, and distance < radius <=> -distance > -radius
    const uint32_t o = sord[tid];
    const float thr = a.metric == 0 ? a.radius : 0.0f - a.radius;
    const bool member = o != 0u && ord2f(o) > thr;
    if (c < n2) row[c] = member ? (((uint64_t)o << 32) | (uint64_t)(0xFFFFFFFFu - idx)) : 0ull;
    const uint64_t mask = __ballot(member);
    if (lane == 0 && mask) atomicAdd(&a.nmem[q], (int32_t)__popcll(mask));
}
void launch_range_rescore(const RangeRowsArgs& a, hipStream_t st) {
    if (a.nrows <= 0 || a.max_cnt <= 0) return;
    int n2 = 1; while (n2 < a.max_cnt) n2 <<= 1;
    hipLaunchKernelGGL(k_range_rescore, dim3((unsigned)((n2 + RANGE_RC - 1) / RANGE_RC), (unsigned)a.nrows), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------
// Ordering.  One workgroup per row sorts the row's first n2 = pow2ceil(rcnt) keys in descending order with a bitonic network: keys are
// unique (the index is part of them) apart from the zeros, which sink.  A tile of 4096 keys (32 KiB) is worked in LDS; the compare-exchange
// steps whose stride reaches beyond a tile go through global memory (the row is L2-resident work of this workgroup alone; a workgroup
// barrier orders its own global writes and reads).
// ---------------------------------------------------------------------------------------
#define RANGE_TILE 4096
__device__ __forceinline__ void range_cmpx_lds(uint64_t* t, int i, int j, bool desc) {
    const uint64_t x = t[i], y = t[j];
    if ((x < y) == desc && x != y) { t[i] = y; t[j] = x; }
}
__global__ __launch_bounds__(1024) void k_range_sort(RangeRowsArgs a) {
    __shared__ uint64_t tile[RANGE_TILE];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t r = blockIdx.x;
    const int n = a.rcnt[r];
    if (n <= 1) return;
    const int n2 = range_pow2ceil(n);
    uint64_t* keys = a.cand + r * (int64_t)a.cap;
    const int T = n2 < RANGE_TILE ? n2 : RANGE_TILE;
    // every tile sorted on its own; tile tb is descending where (tb & T) == 0 once n2 > T (the network's direction rule at size T)
    for (int tb = 0; tb < n2; tb += T) {
        for (int i = tid; i < T; i += nt) tile[i] = keys[tb + i];
        __syncthreads();
        for (int size = 2; size <= T; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (T >> 1); t += nt) {
                    const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                    range_cmpx_lds(tile, i, i + stride, ((tb + i) & size) == 0);
                }
                __syncthreads();
            }
        for (int i = tid; i < T; i += nt) keys[tb + i] = tile[i];
        __syncthreads();
    }
    for (int size = 2 * RANGE_TILE; size <= n2 && size > 0; size <<= 1) {
        for (int stride = size >> 1; stride >= RANGE_TILE; stride >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += nt) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride;
                const bool desc = (i & size) == 0;
                const uint64_t x = keys[i], y = keys[j];
                if ((x < y) == desc && x != y) { keys[i] = y; keys[j] = x; }
            }
            __syncthreads();
        }
        for (int tb = 0; tb < n2; tb += RANGE_TILE) {
            for (int i = tid; i < RANGE_TILE; i += nt) tile[i] = keys[tb + i];
            __syncthreads();
            for (int stride = RANGE_TILE >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (RANGE_TILE >> 1); t += nt) {
                    const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                    range_cmpx_lds(tile, i, i + stride, ((tb + i) & size) == 0);
                }
                __syncthreads();
            }
            for (int i = tid; i < RANGE_TILE; i += nt) keys[tb + i] = tile[i];
            __syncthreads();
        }
    }
}
void launch_range_sort(const RangeRowsArgs& a, hipStream_t st) {
    if (a.nrows <= 0 || a.max_cnt <= 1) return;
    hipLaunchKernelGGL(k_range_sort, dim3((unsigned)a.nrows), dim3(1024), 0, st, a);
}

// ---------------------------------------------------------------------------------------
// lims: one workgroup; thread t owns `per` consecutive queries, the threads' sums are scanned in LDS.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_range_lims(const int32_t* nmem, int64_t nq, int64_t base, int64_t* lims) {
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (nq + 1023) / 1024, lo = tid * per, hi = lo + per < nq ? lo + per : nq;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; i++) s += nmem[i];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = base + part[tid] - s;      // exclusive
    if (tid == 0) lims[0] = base;
    for (int64_t i = lo; i < hi; i++) { run += nmem[i]; lims[i + 1] = run; }
}
void launch_range_lims(const int32_t* nmem, int64_t nq, int64_t base, int64_t* lims, hipStream_t st) {
    hipLaunchKernelGGL(k_range_lims, dim3(1), dim3(1024), 0, st, nmem, nq, base, lims);
}

__global__ __launch_bounds__(256) void k_range_compact(RangeRowsArgs a, const int64_t* koff, uint64_t* dst) {
    const int64_t r = blockIdx.y;
    const int n = a.nmem[a.qsel ? a.qsel[r] : r];
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j < n && j < a.cap) dst[koff[r] + j] = a.cand[r * (int64_t)a.cap + j];
}
void launch_range_compact(const RangeRowsArgs& a, const int64_t* koff, uint64_t* dst, hipStream_t st) {
    if (a.nrows <= 0 || a.max_cnt <= 0) return;
    hipLaunchKernelGGL(k_range_compact, dim3((unsigned)((a.max_cnt + 255) / 256), (unsigned)a.nrows), dim3(256), 0, st, a, koff, dst);
}

// ---------------------------------------------------------------------------------------
// Emission.  Slot j of query q's sorted keys -> D / I at lims[q] - lims[0] + j.  Where the ids are not the keys' indices (explicit ids, IVF
// columns) equal scores are so far ordered by index: the key slot is overwritten with the id, and k_range_ties puts every run of equal
// scores into id order (a slot's place in its run = the ids of the run below its own; runs are short unless the data holds many exact ties).
// Equal scores have equal bits: rescore_rows adds +0 to every score, so -0 never reaches an order word or D.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_range_emit(RangeEmitArgs a) {
    const int64_t q = blockIdx.y;
    const int n = a.nmem[q];
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= n) return;
    uint64_t* keys = a.kptr[q];
    const uint64_t key = keys[j];
    const int64_t o = a.lims[q] - a.lims[0] + j;
    const float s = key_score(key);
    a.D[o] = a.metric == 0 ? s : 0.0f - s;
    const int64_t row = range_row_of(a.kind, key_idx(key), q, a.probe_list, a.seg_start, a.nprobe, a.list_base);
    const int64_t id = a.ids ? a.ids[row] : row;
    a.I[o] = id;
    if (a.ids) keys[j] = (uint64_t)id;
}
__global__ __launch_bounds__(256) void k_range_ties(RangeEmitArgs a) {
    const int64_t q = blockIdx.y;
    const int n = a.nmem[q];
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= n) return;
    const uint32_t* Db = reinterpret_cast<const uint32_t*>(a.D) + (a.lims[q] - a.lims[0]);
    const uint32_t s = Db[j];
    if (!((j > 0 && Db[j - 1] == s) || (j + 1 < n && Db[j + 1] == s))) return;
    int lo = j, hi = j + 1;
    while (lo > 0 && Db[lo - 1] == s) lo--;
    while (hi < n && Db[hi] == s) hi++;
    const int64_t* idv = reinterpret_cast<const int64_t*>(a.kptr[q]);
    const int64_t id = idv[j];
    int rank = 0;
    for (int k = lo; k < hi; k++) { const int64_t ik = idv[k]; rank += (ik < id || (ik == id && k < j)) ? 1 : 0; }
    a.I[a.lims[q] - a.lims[0] + lo + rank] = id;
}
void launch_range_emit(const RangeEmitArgs& a, hipStream_t st) {
    if (a.nq <= 0 || a.max_cnt <= 0) return;
    hipLaunchKernelGGL(k_range_emit, dim3((unsigned)((a.max_cnt + 255) / 256), (unsigned)a.nq), dim3(256), 0, st, a);
}
void launch_range_ties(const RangeEmitArgs& a, hipStream_t st) {
    if (a.nq <= 0 || a.max_cnt <= 0 || !a.ids) return;
    hipLaunchKernelGGL(k_range_ties, dim3((unsigned)((a.max_cnt + 255) / 256), (unsigned)a.nq), dim3(256), 0, st, a);
}

__global__ __launch_bounds__(256) void k_range_gather_rows(const uint32_t* src, uint32_t* dst, int64_t row_words, const int32_t* sel, int64_t n) {
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const uint32_t* s = src + (int64_t)sel[i] * row_words;
    uint32_t* d = dst + i * row_words;
    for (int64_t w = threadIdx.x; w < row_words; w += 256) d[w] = s[w];
}
void launch_range_gather_rows(const void* src, void* dst, int64_t row_bytes, const int32_t* sel, int64_t n, hipStream_t st) {
    if (n <= 0 || row_bytes <= 0) return;
    hipLaunchKernelGGL(k_range_gather_rows, dim3((unsigned)n), dim3(256), 0, st, (const uint32_t*)src, (uint32_t*)dst, row_bytes / 4, sel, n);
}

}  // namespace rsx
