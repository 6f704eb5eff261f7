// api_vt.hip — rsx_vt_*: the linear vector transform handle (faiss.LinearTransform and its subclasses).  The handle owns the
// matrix A [d_out, d_in], its transposed copy (the reverse transform's operand), the bias and two staging buffers for host callers; the
// arithmetic is k_vt_apply (k_vt.hip).  Stream discipline as for an index handle: one non-blocking stream per handle, the caller's data
// complete before the call, the call's work complete when it returns.
#include "rsx_host.h"

struct rsx_vt {
    int device = 0, d_in = 0, d_out = 0;
    bool is_set = false, have_bias = false;
    hipStream_t st = nullptr;
    DevBuf dA, dAt, db, w_x, w_y;
};

namespace {
constexpr int64_t VT_STAGE_BYTES = (int64_t)64 << 20;      // a host operand is staged through at most this much device memory per chunk

void check_devices() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        RSX_THROW(RSX_ERR_HIP, "no HIP device available: librsx has no CPU path");
    }
}
}  // namespace

extern "C" {

int rsx_vt_create(int device, int d_in, int d_out, rsx_vt_t** out) {
    return guarded([&] {
        if (!out) RSX_THROW(RSX_ERR_INVALID, "null out");
        if (d_in <= 0 || d_out <= 0) RSX_THROW(RSX_ERR_INVALID, "vt_create: d_in and d_out must be positive (got %d, %d)", d_in, d_out);
        check_devices();
        int ndev = 0;
        HIPCHECK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) RSX_THROW(RSX_ERR_INVALID, "device %d out of range (have %d)", device, ndev);
        std::unique_ptr<rsx_vt> v(new rsx_vt());
        v->device = device; v->d_in = d_in; v->d_out = d_out;
        HIPCHECK(hipSetDevice(device));
        HIPCHECK(hipStreamCreateWithFlags(&v->st, hipStreamNonBlocking));
        *out = v.release();
    });
}

int rsx_vt_set(rsx_vt_t* v, const float* A, const float* b) {
    return guarded([&] {
        if (!v || !A) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        HIPCHECK(hipSetDevice(v->device));
        const size_t na = (size_t)v->d_in * v->d_out;
        v->dA.ensure(na * 4);
        v->dAt.ensure(na * 4);
        HIPCHECK(hipMemcpyAsync(v->dA.p, A, na * 4, hipMemcpyHostToDevice, v->st));
        launch_vt_transpose(v->dA.as<float>(), v->d_out, v->d_in, v->dAt.as<float>(), v->st);
        v->have_bias = b != nullptr;
        if (b) {
            v->db.ensure((size_t)v->d_out * 4);
            HIPCHECK(hipMemcpyAsync(v->db.p, b, (size_t)v->d_out * 4, hipMemcpyHostToDevice, v->st));
        }
        HIPCHECK(hipStreamSynchronize(v->st));
        HIPCHECK(hipGetLastError());
        v->is_set = true;
    });
}

int rsx_vt_apply(rsx_vt_t* v, int64_t n, const void* x, int dtype, float* y, int reverse) {
    return guarded([&] {
        if (!v) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        if (n < 0) RSX_THROW(RSX_ERR_INVALID, "vt_apply: n must not be negative (got %lld)", (long long)n);
        if (dtype != RSX_F32 && dtype != RSX_F16) RSX_THROW(RSX_ERR_INVALID, "bad dtype %d", dtype);
        if (!v->is_set) RSX_THROW(RSX_ERR_NOT_TRAINED, "vt_apply: the transform has no matrix yet (rsx_vt_set)");
        if (n == 0) return;
        if (!x || !y) RSX_THROW(RSX_ERR_INVALID, "null pointer");
        HIPCHECK(hipSetDevice(v->device));
        // forward: X [n, d_in] · Aᵀ + b -> [n, d_out];  reverse: fp32(Y - b) [n, d_out] · A -> [n, d_in], through the transposed copy
        const int dk = reverse ? v->d_out : v->d_in, nc = reverse ? v->d_in : v->d_out;
        const float* C = reverse ? v->dAt.as<float>() : v->dA.as<float>();
        const float* bias = v->have_bias ? v->db.as<float>() : nullptr;
        const float* bsub = reverse ? bias : nullptr;
        const float* badd = reverse ? nullptr : bias;
        const bool x_dev = is_device_ptr(x), y_dev = is_device_ptr(y);
        const size_t esz = dtype == RSX_F16 ? 2 : 4;
        int64_t chunk = n;
        if (!x_dev || !y_dev) chunk = std::min<int64_t>(n, std::max<int64_t>(128, VT_STAGE_BYTES / ((int64_t)std::max(dk, nc) * 4) / 128 * 128));
        for (int64_t i0 = 0; i0 < n; i0 += chunk) {
            const int64_t nb = std::min(chunk, n - i0);
            const void* xp = (const char*)x + (size_t)i0 * dk * esz;
            if (!x_dev) {
                v->w_x.ensure((size_t)nb * dk * esz);
                HIPCHECK(hipMemcpyAsync(v->w_x.p, xp, (size_t)nb * dk * esz, hipMemcpyHostToDevice, v->st));
                xp = v->w_x.p;
            }
            float* yp = y + i0 * nc;
            if (!y_dev) { v->w_y.ensure((size_t)nb * nc * 4); yp = v->w_y.as<float>(); }
            launch_vt_apply(xp, dtype == RSX_F16, nb, dk, bsub, C, nc, badd, yp, v->st);
            if (!y_dev) HIPCHECK(hipMemcpyAsync(y + i0 * nc, yp, (size_t)nb * nc * 4, hipMemcpyDeviceToHost, v->st));
            if (!x_dev || !y_dev) HIPCHECK(hipStreamSynchronize(v->st));      // the staging buffers serve the next chunk
        }
        HIPCHECK(hipStreamSynchronize(v->st));
        HIPCHECK(hipGetLastError());
    });
}

int rsx_vt_destroy(rsx_vt_t* v) {
    return guarded([&] {
        if (!v) return;
        (void)hipSetDevice(v->device);
        if (v->st) { (void)hipStreamSynchronize(v->st); (void)hipStreamDestroy(v->st); }
        delete v;
    });
}

}  // extern "C"
