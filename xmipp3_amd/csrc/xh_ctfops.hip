// xh_ctfops.hip -- the CTF pre-steps that sit in front of the matching / reconstruction loop:
//
//   xh_ctfop_phase_flip   actualPhaseFlip, reconstruction/ctf_phase_flip.cpp:88-117 (xmipp_ctf_phase_flip): transform,
//                         negate every coefficient where the undamped CTF is negative, transform back
//   xh_ctfop_wiener2d     Wiener2D::wienerFilter + applyWienerFilter, data/wiener2d.cpp:29-141 (xmipp_ctf_correct_wiener2d):
//                         pad about the Xmipp origin, transform, multiply by CTF / (CTF^2 + wc), transform back, crop
//
// The reference works on the half spectrum of a real transform (FFTW r2c / c2r). Here the image rides as the real part of a
// complex transform (xh_fft2d: whole micrographs fit, any size its line plans take) and the real filter is applied to the
// full spectrum so that the result is what the half-spectrum form gives: coefficient (i, j) with j beyond nx/2 is the
// conjugate of (-i, -j), which the reference multiplies by the filter value at ((ny - i) % ny, nx - j) -- evaluated at those
// indices here, because FFT_IDX2DIGFREQ maps the Nyquist index to +0.5 on either side. The CTF itself is evaluated in double
// precision with the reference's formulas (data/ctf.h:452-500,541-570,1002-1029); the transforms run in fp32 (reference:
// double), which is the tolerance the tests state (1e-5 of the image's largest value).
#include <cmath>
#include <cstring>

#include "xh_common.h"
#include "xh_ctf.h"

namespace {
typedef float2 xc_cf;

// the index pair whose filter value the half-spectrum form applies to coefficient (i, j)
__device__ __forceinline__ void d_half_index(int &i, int &j, int ny, int nx)
{
    if (j > nx / 2) { j = nx - j; i = (ny - i) % ny; }
}

__global__ void __launch_bounds__(256) k_ctf_embed(const float *__restrict__ img, int ydim, int xdim, xc_cf *__restrict__ out, int pY, int pX, int oy, int ox)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)pY * pX) return;
    const int i = (int)(t / pX), j = (int)(t - (size_t)i * pX);
    const int si = i - oy, sj = j - ox;
    const bool in = si >= 0 && si < ydim && sj >= 0 && sj < xdim;
    out[t] = xc_cf{in ? img[(size_t)si * xdim + sj] : 0.f, 0.f};
}

__global__ void __launch_bounds__(256) k_ctf_extract(const xc_cf *__restrict__ in, int pY, int pX, int oy, int ox, float *__restrict__ img, int ydim, int xdim)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)ydim * xdim) return;
    const int i = (int)(t / xdim), j = (int)(t - (size_t)i * xdim);
    img[t] = in[(size_t)(i + oy) * pX + (j + ox)].x;
}

__global__ void __launch_bounds__(256) k_ctf_flip(xc_cf *__restrict__ F, int ny, int nx, CtfSide s, double iTm)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)ny * nx) return;
    int i = (int)(t / nx), j = (int)(t - (size_t)i * nx);
    d_half_index(i, j, ny, nx);
    if (d_ctf_at(s, d_digfreq(j, nx) * iTm, d_digfreq(i, ny) * iTm, false) < 0) { xc_cf v = F[t]; F[t] = xc_cf{-v.x, -v.y}; }
}

// ctfIm (wiener2d.cpp:55-69) over the whole padded array, and the sum of its squares for Grigorieff's default constant
__global__ void __launch_bounds__(256) k_ctf_wiener_ctf(double *__restrict__ ctfIm, int pY, int pX, CtfSide s, double iTs, int damping, int phaseFlipped,
                                                        double *__restrict__ sumSq)
{
    __shared__ double red[256];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    double sq = 0;
    if (t < (size_t)pY * pX) {
        const int i = (int)(t / pX), j = (int)(t - (size_t)i * pX);
        double v = d_ctf_at(s, d_digfreq(j, pX) * iTs, d_digfreq(i, pY) * iTs, damping != 0);
        if (phaseFlipped) v = fabs(v);
        ctfIm[t] = v;
        sq = v * v;
    }
    red[threadIdx.x] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) atomicAdd(sumSq, red[0]);
}

// F(i, j) *= ctf / (ctf^2 + wc) at the half-spectrum index of (i, j); wc < 0: 0.1 * mean(ctf^2) (wiener2d.cpp:78-98)
__global__ void __launch_bounds__(256) k_ctf_wiener_apply(xc_cf *__restrict__ F, const double *__restrict__ ctfIm, int pY, int pX, double wcIn,
                                                          const double *__restrict__ sumSq)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)pY * pX) return;
    int i = (int)(t / pX), j = (int)(t - (size_t)i * pX);
    d_half_index(i, j, pY, pX);
    const double wc = wcIn < 0. ? 0.1 * (*sumSq / ((double)pY * (double)pX)) : wcIn;
    const double c = ctfIm[(size_t)i * pX + j];
    const double m = c / (c * c + wc);
    const xc_cf v = F[t];
    F[t] = xc_cf{(float)(v.x * m), (float)(v.y * m)};
}
}  // namespace

struct xh_ctfop {
    xh_ctx *ctx;
    int ydim, xdim, pY, pX;
    xh_fft2d *fft = nullptr;
    XhBuf work, ctfIm, sum;
    ~xh_ctfop()
    {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        xh_fft2d_destroy(fft);
    }
};

extern "C" {

int xh_ctfop_create(xh_ctx *ctx, int32_t ydim, int32_t xdim, double pad, xh_ctfop **out)
{
    XH_CHECK(ctx && out && ydim >= 2 && xdim >= 2, XH_ERR_ARG, "xh_ctfop_create: bad argument");
    XH_HIP(hipSetDevice(ctx->device));
    if (!(pad >= 1.)) pad = 1.;                 // XMIPP_MAX(1., pad), ctf_correct_wiener2d.cpp:34
    std::unique_ptr<xh_ctfop> h(new xh_ctfop);
    h->ctx = ctx; h->ydim = ydim; h->xdim = xdim;
    h->pY = (int)(ydim * pad); h->pX = (int)(xdim * pad);        // wiener2d.cpp:31-33
    XH_TRY(xh_fft2d_create(ctx, h->pY, h->pX, &h->fft));
    XH_TRY(xh_buf_alloc(ctx, h->work, sizeof(xc_cf) * (size_t)h->pY * h->pX));
    XH_TRY(xh_buf_alloc(ctx, h->sum, sizeof(double)));
    *out = h.release();
    return XH_OK;
}

int xh_ctfop_destroy(xh_ctfop *h)
{
    delete h;
    return XH_OK;
}

int xh_ctfop_phase_flip(xh_ctfop *h, float *d_img, const xh_ctf_params *ctf, double sampling_rate)
{
    XH_CHECK(h && d_img && ctf && sampling_rate > 0, XH_ERR_ARG, "xh_ctfop_phase_flip: bad argument");
    XH_CHECK(h->pY == h->ydim && h->pX == h->xdim, XH_ERR_STATE, "xh_ctfop_phase_flip: the handle was created with padding; phase flipping works on the image as it is");
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const size_t tot = (size_t)h->ydim * h->xdim;
    const unsigned nb = (unsigned)((tot + 255) / 256);
    xc_cf *w = (xc_cf *)h->work.p;
    hipLaunchKernelGGL(k_ctf_embed, dim3(nb), dim3(256), 0, ctx->stream, (const float *)d_img, h->ydim, h->xdim, w, h->ydim, h->xdim, 0, 0);
    XH_LAUNCH_CHECK();
    XH_TRY(xh_fft2d_exec(h->fft, (float *)w, 0));
    hipLaunchKernelGGL(k_ctf_flip, dim3(nb), dim3(256), 0, ctx->stream, w, h->ydim, h->xdim, side_info(*ctf, true), 1.0 / sampling_rate);
    XH_LAUNCH_CHECK();
    XH_TRY(xh_fft2d_exec(h->fft, (float *)w, 1));
    hipLaunchKernelGGL(k_ctf_extract, dim3(nb), dim3(256), 0, ctx->stream, (const xc_cf *)w, h->ydim, h->xdim, 0, 0, d_img, h->ydim, h->xdim);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

int xh_ctfop_wiener2d(xh_ctfop *h, float *d_imgs, int32_t n, const xh_ctf_params *ctfs, double sampling_rate, int32_t phase_flipped,
                      int32_t is_isotropic, double wiener_constant, int32_t correct_envelope)
{
    XH_CHECK(h && d_imgs && ctfs && n >= 0 && sampling_rate > 0, XH_ERR_ARG, "xh_ctfop_wiener2d: bad argument");
    (void)is_isotropic;      // the reference averages DeltafU/V after produceSideInfo has consumed them (wiener2d.cpp:36-50): no effect
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const size_t ptot = (size_t)h->pY * h->pX, itot = (size_t)h->ydim * h->xdim;
    XH_TRY(xh_buf_reserve(ctx, h->ctfIm, sizeof(double) * ptot));
    const unsigned nbp = (unsigned)((ptot + 255) / 256), nbi = (unsigned)((itot + 255) / 256);
    // selfWindow about the Xmipp origin (wiener2d.cpp:111-119): the image keeps its logical coordinates
    const int oy = h->pY / 2 - h->ydim / 2, ox = h->pX / 2 - h->xdim / 2;
    xc_cf *w = (xc_cf *)h->work.p;
    for (int k = 0; k < n; ++k) {
        float *img = d_imgs + (size_t)k * itot;
        const CtfSide s = side_info(ctfs[k], true);
        XH_HIP(hipMemsetAsync(h->sum.p, 0, sizeof(double), ctx->stream));
        hipLaunchKernelGGL(k_ctf_wiener_ctf, dim3(nbp), dim3(256), 0, ctx->stream, (double *)h->ctfIm.p, h->pY, h->pX, s, 1.0 / sampling_rate,
                           correct_envelope, phase_flipped, (double *)h->sum.p);
        hipLaunchKernelGGL(k_ctf_embed, dim3(nbp), dim3(256), 0, ctx->stream, (const float *)img, h->ydim, h->xdim, w, h->pY, h->pX, oy, ox);
        XH_LAUNCH_CHECK();
        XH_TRY(xh_fft2d_exec(h->fft, (float *)w, 0));
        hipLaunchKernelGGL(k_ctf_wiener_apply, dim3(nbp), dim3(256), 0, ctx->stream, w, (const double *)h->ctfIm.p, h->pY, h->pX, wiener_constant,
                           (const double *)h->sum.p);
        XH_LAUNCH_CHECK();
        XH_TRY(xh_fft2d_exec(h->fft, (float *)w, 1));
        hipLaunchKernelGGL(k_ctf_extract, dim3(nbi), dim3(256), 0, ctx->stream, (const xc_cf *)w, h->pY, h->pX, oy, ox, img, h->ydim, h->xdim);
        XH_LAUNCH_CHECK();
    }
    return XH_OK;
}

}  // extern "C"
