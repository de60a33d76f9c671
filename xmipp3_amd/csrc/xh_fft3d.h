// xh_fft3d.h -- fp64 3-D real transforms of any size (line FFTs of xh_plan.h) in FFTW layout: real [Z][Y][X] <-> half spectrum
// [Z][Y][X/2+1]. Both directions are un-normalised, as FFTW's and cuFFT's plans are; a caller that wants the 1/N of an inverse passes it
// as `scale`, which multiplies each result once, the same single rounding as a separate pass over the output.
// Used by xh_fsc.hip (forward), xh_vds.hip (both, a plan per call) and, through the handle part of xh_volume.h, by the whole-volume
// programs listed there.
#ifndef XH_FFT3D_H
#define XH_FFT3D_H
#include "xh_common.h"
#include "xh_plan.h"

namespace {

// x lines: real input [nlines][X] (times scale) -> half spectrum [nlines][xh], forward, un-normalised
__global__ void __launch_bounds__(256)
k_fft3d_rows_r2c(const double *__restrict__ in, xh_cd *__restrict__ out, XhPlan<double> plan, size_t nlines, int X, int xh, int lpb, double scale)
{
    extern __shared__ __align__(16) unsigned char fft3d_smem[];
    xh_cd *s = reinterpret_cast<xh_cd *>(fft3d_smem);
    const int M = 1 << plan.logM;
    const int tid = threadIdx.x, nth = blockDim.x;
    const size_t line0 = (size_t)blockIdx.x * lpb;
    const int nl = (int)min((size_t)lpb, nlines - line0);
    for (int i = tid; i < lpb * X; i += nth) {
        const int l = i / X, e = i - l * X;
        const double v = l < nl ? in[(line0 + l) * X + e] * scale : 0.0;
        s[l * M + xh_plan_pos(plan, e)] = xh_cd{v, 0.0};
    }
    __syncthreads();
    xh_plan_exec<double, false>(s, plan, lpb, tid, nth);
    for (int i = tid; i < nl * xh; i += nth) {
        const int l = i / xh, e = i - l * xh;
        out[(line0 + l) * xh + e] = s[l * M + e];
    }
}

// x lines: half spectrum [nlines][xh] -> real [nlines][X] times scale, inverse, un-normalised. The line is completed by Hermitian
// symmetry (element e >= xh is conj(F[X - e])) and the real part kept: the imaginary parts of the DC and Nyquist terms drop out,
// as in FFTW's c2r.
__global__ void __launch_bounds__(256)
k_fft3d_rows_c2r(const xh_cd *__restrict__ in, double *__restrict__ out, XhPlan<double> plan, size_t nlines, int X, int xh, int lpb, double scale)
{
    extern __shared__ __align__(16) unsigned char fft3d_smem[];
    xh_cd *s = reinterpret_cast<xh_cd *>(fft3d_smem);
    const int M = 1 << plan.logM;
    const int tid = threadIdx.x, nth = blockDim.x;
    const size_t line0 = (size_t)blockIdx.x * lpb;
    const int nl = (int)min((size_t)lpb, nlines - line0);
    for (int i = tid; i < lpb * X; i += nth) {
        const int l = i / X, e = i - l * X;
        xh_cd v = xh_cd{0.0, 0.0};
        if (l < nl) {
            if (e < xh) v = in[(line0 + l) * xh + e];
            else { v = in[(line0 + l) * xh + (X - e)]; v.y = -v.y; }
        }
        s[l * M + xh_plan_pos(plan, e)] = v;
    }
    __syncthreads();
    xh_plan_exec<double, true>(s, plan, lpb, tid, nth);
    for (int i = tid; i < nl * X; i += nth) {
        const int l = i / X, e = i - l * X;
        out[(line0 + l) * X + e] = s[l * M + e].x * scale;
    }
}

// y and z lines of nb half spectra that lie one after the other, in place
template <bool INV>
int fft3d_yz(xh_ctx *ctx, xh_cd *F, int Z, int Y, int xh, const XhPlan<double> &py, const XhPlan<double> &pz, int nb = 1)
{
    if (Y > 1) {   // y lines: (b,k,j) -> offset (b*Z + k)*Y*xh + j, element stride xh
        const int lpb = xh_plan_lpb(py, 64 * 1024, 8);
        const size_t smem = ((size_t)lpb * sizeof(xh_cd)) << py.logM, nlines = (size_t)nb * Z * xh;
        hipLaunchKernelGGL((xh_k_fft_lines<double, INV>), dim3((unsigned)((nlines + lpb - 1) / lpb)), dim3(256), smem, ctx->stream, F, py,
                           nlines, (size_t)xh, (size_t)Y * xh, (size_t)1, (size_t)xh, lpb);
        XH_LAUNCH_CHECK();
    }
    if (Z > 1) {   // z lines: (b,i,j) -> offset b*Z*Y*xh + i*xh + j, element stride Y*xh
        const int lpb = xh_plan_lpb(pz, 64 * 1024, 8);
        const size_t smem = ((size_t)lpb * sizeof(xh_cd)) << pz.logM, nlines = (size_t)nb * Y * xh;
        hipLaunchKernelGGL((xh_k_fft_lines<double, INV>), dim3((unsigned)((nlines + lpb - 1) / lpb)), dim3(256), smem, ctx->stream, F, pz,
                           nlines, (size_t)Y * xh, (size_t)Z * Y * xh, (size_t)1, (size_t)Y * xh, lpb);
        XH_LAUNCH_CHECK();
    }
    return XH_OK;
}

// the plans of one volume size. The tables belong to the struct, so it lives with the handle (or the call) that transforms
struct XhFft3d {
    xh_ctx *ctx = nullptr;
    int Z = 0, Y = 0, X = 0, xh = 0;
    XhPlanBufs<double> px, py, pz;

    // forward: d_in [Z][Y][X] (each value times scale) -> F [Z][Y][X/2+1]
    int r2c(const double *d_in, xh_cd *F, double scale = 1.0) const
    {
        const int lpb = xh_plan_lpb(px.plan, 64 * 1024, 8);
        const size_t smem = ((size_t)lpb * sizeof(xh_cd)) << px.plan.logM, nlines = (size_t)Z * Y;
        hipLaunchKernelGGL(k_fft3d_rows_r2c, dim3((unsigned)((nlines + lpb - 1) / lpb)), dim3(256), smem, ctx->stream, d_in, F, px.plan, nlines, X, xh, lpb,
                           scale);
        XH_LAUNCH_CHECK();
        return fft3d_yz<false>(ctx, F, Z, Y, xh, py.plan, pz.plan);
    }

    // inverse: F [Z][Y][X/2+1] (overwritten) -> d_out [Z][Y][X], each value times scale
    int c2r(xh_cd *F, double *d_out, double scale) const
    {
        XH_TRY(fft3d_yz<true>(ctx, F, Z, Y, xh, py.plan, pz.plan));
        const int lpb = xh_plan_lpb(px.plan, 64 * 1024, 8);
        const size_t smem = ((size_t)lpb * sizeof(xh_cd)) << px.plan.logM, nlines = (size_t)Z * Y;
        hipLaunchKernelGGL(k_fft3d_rows_c2r, dim3((unsigned)((nlines + lpb - 1) / lpb)), dim3(256), smem, ctx->stream, F, d_out, px.plan, nlines, X, xh, lpb,
                           scale);
        XH_LAUNCH_CHECK();
        return XH_OK;
    }
};

int xh_fft3d_create(xh_ctx *ctx, int Z, int Y, int X, XhFft3d &f)
{
    f.ctx = ctx; f.Z = Z; f.Y = Y; f.X = X; f.xh = X / 2 + 1;
    XH_TRY(xh_plan_create<double>(ctx, X, f.px));
    XH_TRY(xh_plan_create<double>(ctx, Y, f.py));
    return xh_plan_create<double>(ctx, Z, f.pz);
}

}  // namespace

#endif
