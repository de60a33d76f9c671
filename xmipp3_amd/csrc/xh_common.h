// xh_common.h -- shared internals of libxmipp_hip.so (gfx950 only).
#ifndef XH_COMMON_H
#define XH_COMMON_H
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>
#include "../../include/xmipp_hip.h"

void xh_set_error(const char *fmt, ...);

#define XH_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            xh_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                         __LINE__);                                                       \
            return XH_ERR_HIP;                                                            \
        }                                                                                 \
    } while (0)

#define XH_CHECK(cond, code, ...)       \
    do {                                \
        if (!(cond)) {                  \
            xh_set_error(__VA_ARGS__);  \
            return code;                \
        }                               \
    } while (0)

#define XH_TRY(call)              \
    do {                          \
        int r_ = (call);          \
        if (r_ != XH_OK) return r_; \
    } while (0)

#define XH_LAUNCH_CHECK() XH_HIP(hipGetLastError())

// a kernel of 256-thread workgroups on the context's stream
#define XH_LAUNCH256(ctx, kern, grid, ...)                                                       \
    do {                                                                                         \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (ctx)->stream, __VA_ARGS__);          \
        XH_LAUNCH_CHECK();                                                                       \
    } while (0)

struct xh_ctx {
    int device;
    hipStream_t stream;
    bool own_stream;
    int num_cus;
};

// A device allocation with one owner (a handle member or a local of an entry point): move-only, freed by its
// destructor, counted in xh_device_bytes_held.  A local freed at scope exit on an error path needs no prior
// synchronisation: hipFree synchronises the device before it releases the memory.
struct XhBuf;
void xh_buf_free(XhBuf &b);   // early release; the buffer is empty afterwards
struct XhBuf {
    void *p = nullptr;
    size_t bytes = 0;
    XhBuf() = default;
    XhBuf(const XhBuf &) = delete;
    XhBuf &operator=(const XhBuf &) = delete;
    XhBuf(XhBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    XhBuf &operator=(XhBuf &&o) noexcept
    {
        if (this != &o) {
            xh_buf_free(*this);
            p = o.p;
            bytes = o.bytes;
            o.p = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~XhBuf() { xh_buf_free(*this); }
};
// frees b, then allocates `bytes` (none for 0)
int xh_buf_alloc(xh_ctx *ctx, XhBuf &b, size_t bytes);
// xh_buf_alloc, then a synchronous copy of `bytes` from the host
int xh_buf_upload(xh_ctx *ctx, XhBuf &b, const void *src, size_t bytes);
// grow-only scratch: reallocates (after synchronising the stream) only when it holds fewer than `bytes`;
// *grown tells whether it did
int xh_buf_reserve(xh_ctx *ctx, XhBuf &b, size_t bytes, bool *grown = nullptr);

// Page-locked host memory with one owner, XhBuf's twin: move-only, allocated through the context, freed by its destructor. A handle's
// destructor body synchronises the stream; its members, this one among them, go after the body, so no copy is still using the memory.
struct XhPinned {
    void *p = nullptr;
    XhPinned() = default;
    XhPinned(const XhPinned &) = delete;
    XhPinned &operator=(const XhPinned &) = delete;
    XhPinned(XhPinned &&o) noexcept : p(o.p) { o.p = nullptr; }
    XhPinned &operator=(XhPinned &&o) noexcept
    {
        std::swap(p, o.p);      // o's destructor frees what this held
        return *this;
    }
    ~XhPinned() { if (p) (void)hipHostFree(p); }
    double *f64() const { return (double *)p; }
};
// frees b, then allocates `bytes` of page-locked memory
int xh_pinned_alloc(xh_ctx *ctx, XhPinned &b, size_t bytes);

// A HIP event with one owner, the third of the family: move-only, destroyed by its destructor, which like XhPinned's runs after the body of
// the handle's destructor has synchronised the stream. A handle holds one, an array or a vector of them; a failed create leaks none.
struct XhEvent {
    hipEvent_t e = nullptr;
    XhEvent() = default;
    XhEvent(const XhEvent &) = delete;
    XhEvent &operator=(const XhEvent &) = delete;
    XhEvent(XhEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
    XhEvent &operator=(XhEvent &&o) noexcept
    {
        std::swap(e, o.e);      // o's destructor destroys what this held
        return *this;
    }
    ~XhEvent() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};
// destroys what ev held, then creates an event; timed false: hipEventDisableTiming, an event that only orders
static inline int xh_event_create(XhEvent &ev, bool timed = true)
{
    ev = XhEvent();
    XH_HIP(hipEventCreateWithFlags(&ev.e, timed ? hipEventDefault : hipEventDisableTiming));
    return XH_OK;
}

// a grow-only device buffer that lives with a 2-D transform plan (frame-after-frame callers: dose filter, binning)
int xh_fft2d_user_scratch(xh_fft2d *f, size_t bytes, void **p);
int xh_fft2d_rows_of_real_pairs(xh_fft2d *f, const float *d_frame, const float *d_dark, const float *d_gain, int Y, float *d_work, int *n1, int *n2);
int xh_fft2d_rows_of_real_pairs_kept(xh_fft2d *f, const float *d_frame, const float *d_dark, const float *d_gain, int Y, int nc, float *d_C, int *done);

// the Fourier projector's internals shared with xh_ca2: Euler_angles2matrix -> A [9], and n projections from device Euler matrices
// (eul_stride doubles apart on the device) as doubles that stay on the device, d_out [n][D][D]; projection p is multiplied by the CTF image [D][D/2+1] at
// d_ctf + p * ctf_stride (d_ctf null: none). Asynchronous on the context's stream.
void xh_fp_euler(double rot, double tilt, double psi, double *A);
int xh_fp_project_f64(xh_fp *fp, const double *d_eul, int32_t eul_stride, int32_t n, const double *d_ctf, size_t ctf_stride, double *d_out);

// lockstep Powell (host/powell_batch.h, xh_powell.hip). pre (nullable) decides a cost on the host: it returns 1 and sets *cost, and
// that evaluation never reaches f
typedef int32_t (*xh_lockstep_pre_fn)(int32_t problem, const double *x, double *cost, void *user);
int xh_powell_lockstep(int32_t nprob, const int32_t *n, int32_t nmax, double *p, const double *steps, double ftol, int32_t capacity,
                       xh_batch_cost_fn f, xh_lockstep_pre_fn pre, void *user, double *fret, int32_t *iter, int64_t *evals);

static inline int xh_ilog2(int n)
{
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}
static inline bool xh_is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// FFT_IDX2DIGFREQ (xmippCore xmipp_fft.h; in-tree copy cuda_gpu_reconstruct_fourier.cpp:381-385): the digital frequency, in
// [-0.5, 0.5], of index idx of a transform of `size` points
__device__ __forceinline__ double d_digfreq(int idx, int size) { return size <= 1 ? 0.0 : (double)(idx <= (size >> 1) ? idx : idx - size) / (double)size; }

#endif
