// xh_estimators.h -- the estimator kernels and plans that the one-reference estimators (xh_estimators.hip) and the many-reference
// alignment (xh_align_sig.hip) share. The per-element arithmetic of the kernels that read a reference lives in the device helpers
// below, so that both paths compute every value with the same operations in the same order.
#ifndef XMIPP3_AMD_XH_ESTIMATORS_H
#define XMIPP3_AMD_XH_ESTIMATORS_H
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "xh_common.h"
#include "xh_bspline.h"
#include "xh_plan.h"
#include "xh_reduce.h"

namespace {
typedef float2 es_cf;

// first extremum in element order: std::max_element / std::min_element return the first of equals, the search around the centre
// replaces its candidate on a strict comparison only
template <bool LOWEST>
__global__ void __launch_bounds__(256) k_es_extrema(const float *__restrict__ data, size_t elems, int ydim, int xdim, int around, int maxDist, int empty,
                                                    float *__restrict__ pos, float *__restrict__ val)
{
    __shared__ float sv[256];
    __shared__ long long si[256];
    const float *d = data + (size_t)blockIdx.x * elems;
    const float start = LOWEST ? 3.402823466e+38f : -3.402823466e+38f;
    float best = start;
    long long bi = -1;
    if (!around) {
        for (size_t i = threadIdx.x; i < elems; i += 256) {
            const float v = d[i];
            // element 0 always becomes the candidate (max_element starts from it), later ones only when strictly better
            if (bi < 0 || (LOWEST ? v < best : v > best)) { best = v; bi = (long long)i; }
        }
    } else if (!empty) {
        const int xHalf = xdim / 2, yHalf = ydim / 2;
        const int x0 = max(0, xHalf - maxDist), x1 = min(xdim - 1, xHalf + maxDist), y0 = max(0, yHalf - maxDist), y1 = min(ydim - 1, yHalf + maxDist);
        const int w = x1 - x0 + 1, h = y1 - y0 + 1;
        for (int t = threadIdx.x; t < w * h; t += 256) {
            const int y = y0 + t / w, x = x0 + t % w;
            const int ly = y - yHalf, lx = x - xHalf;
            if (ly * ly + lx * lx > maxDist * maxDist) continue;
            const float v = d[(size_t)y * xdim + x];
            if (LOWEST ? v < best : v > best) { best = v; bi = (long long)y * xdim + x; }
        }
    }
    sv[threadIdx.x] = best; si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const float v = sv[threadIdx.x + o];
            const long long k = si[threadIdx.x + o];
            const bool mine = si[threadIdx.x] >= 0;
            if (k >= 0 && (!mine || (LOWEST ? v < sv[threadIdx.x] : v > sv[threadIdx.x]) || (v == sv[threadIdx.x] && k < si[threadIdx.x]))) { sv[threadIdx.x] = v; si[threadIdx.x] = k; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (pos) pos[blockIdx.x] = (float)si[0];
        if (val) val[blockIdx.x] = si[0] >= 0 ? sv[0] : start;
    }
}

// element (x, y) of the centred correlation of the shift estimator: ref conj(other) (-1)^(x+y), double precision
__device__ __forceinline__ xh_cd es_correlate64_at(xh_cd r, xh_cd o, int x, int y)
{
    xh_cd v = xh_cd{r.x * o.x + r.y * o.y, r.y * o.x - r.x * o.y};
    if ((x + y) & 1) { v.x = -v.x; v.y = -v.y; }
    return v;
}

// applyGeometry(LINEAR, out, in, A, IS_INV, DONT_WRAP) of xmippCore's 2-D branch, outside value 0: out(x, y) = in at A (x, y, 1) in
// logical (Xmipp origin) coordinates, bilinear, pixels that map outside the image stay 0. Pixel (i, j) of one image V1 through A [9].
__device__ __forceinline__ float es_geometry_at(const float *__restrict__ V1, const double *__restrict__ A, int i, int j, int ydim, int xdim)
{
    const int cen_y = ydim / 2, cen_x = xdim / 2;
    const double eps = 1e-6;                                   // XMIPP_EQUAL_ACCURACY
    const double minxp = -cen_x, minyp = -cen_y, maxxp = xdim - cen_x - 1, maxyp = ydim - cen_y - 1;
    const double x = j - cen_x, y = i - cen_y;
    const double xp = x * A[0] + y * A[1] + A[2], yp = x * A[3] + y * A[4] + A[5];
    double val = 0.0;
    if (!(xp < minxp - eps || xp > maxxp + eps || yp < minyp - eps || yp > maxyp + eps)) {
        double wx = xp + cen_x;
        const int m1 = (int)wx;
        wx = wx - m1;
        const int m2 = m1 + 1;
        double wy = yp + cen_y;
        const int n1 = (int)wy;
        wy = wy - n1;
        const int n2 = n1 + 1;
        const double wx_1 = 1 - wx, wy_1 = 1 - wy;
        double aux2 = wy_1 * wx_1;
        double tmp = aux2 * (double)V1[(size_t)n1 * xdim + m1];
        if (wx != 0 && m2 < xdim) tmp += (wy_1 - aux2) * (double)V1[(size_t)n1 * xdim + m2];
        if (wy != 0 && n2 < ydim) {
            aux2 = wy * wx_1;
            tmp += aux2 * (double)V1[(size_t)n2 * xdim + m1];
            if (wx != 0 && m2 < xdim) tmp += (wy - aux2) * (double)V1[(size_t)n2 * xdim + m2];
        }
        val = tmp;
    }
    return (float)val;
}

// correlationIndex(ref, other) of xmippCore without a mask (population statistics: its N / (N - 1) is an integer division), one block
// of 256 threads per image; the value is valid in thread 0
__device__ __forceinline__ float es_corr_index_block(const float *__restrict__ ref, const float *__restrict__ y, size_t N)
{
    __shared__ double red[5][256];
    double mx = 0, my = 0, sx = 0, sy = 0, sxy = 0;
    for (size_t i = threadIdx.x; i < N; i += 256) { const double a = ref[i], b = y[i]; mx += a; my += b; sx += a * a; sy += b * b; sxy += a * b; }
    const double v[5] = {mx, my, sx, sy, sxy};
    xh_tree256(red, v);
    if (threadIdx.x != 0) return 0.f;
    const double n = (double)N;
    mx = red[0][0] / n; my = red[1][0] / n;
    const double f = N > 1 ? (double)(N / (N - 1)) : 0.0;
    sx = sqrt(fabs((red[2][0] / n - mx * mx) * f)); sy = sqrt(fabs((red[3][0] / n - my * my) * f));
    double r = 0;
    if (!(fabs(sx) < 1e-6 || fabs(sy) < 1e-6)) r = (red[4][0] - n * mx * my) / ((sx * sy) * n);          // sum (x - mx)(y - my) = sum xy - n mx my
    return (float)r;
}
// ---- PolarRotationEstimator (polar_rotation_estimator.cpp:49-99) as the reference computes it: rings sampled with BsplineOrder 1
// (polar.h:689-693: interpolatedElement2DOutsideZero, bilinear, zero outside the image), not normalised, every ring's
// DFT / nsam (polar.cpp:34-54), the ring-weighted products summed per frequency and brought back over 2 N - 1 angles
// (:58; polar.cpp:99-148), the first maximum (polar.cpp:212-233).  Double precision throughout, as the reference.
struct EsRing { int nsam, soff, coff; double w; };

__global__ void __launch_bounds__(256) k_es_polar_linear(const float *__restrict__ imgs, const float *__restrict__ sx, const float *__restrict__ sy, int nsamples, int D,
                                                         double *__restrict__ rings)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nsamples) return;
    const float *img = imgs + (size_t)blockIdx.y * D * D;
    const int first = -(D / 2), last = first + D - 1;
    const double minp = first, maxp = last;
    double xp = (double)sx[t], yp = (double)sy[t];
    // coordinates outside [min - 1e-6, max + 1e-6] are wrapped (polar.h:683-686)
    if (xp < minp - 1e-6 || xp > maxp + 1e-6) xp = d_realwrap<double>(xp, minp - 0.5, maxp + 0.5);
    if (yp < minp - 1e-6 || yp > maxp + 1e-6) yp = d_realwrap<double>(yp, minp - 0.5, maxp + 0.5);
    const int x0 = (int)floor(xp), y0 = (int)floor(yp);
    const double fx = xp - x0, fy = yp - y0;
    auto at = [&](int i, int j) -> double { return (j < first || j > last || i < first || i > last) ? 0.0 : (double)img[(size_t)(i - first) * D + (j - first)]; };
    const double d00 = at(y0, x0), d01 = at(y0, x0 + 1), d10 = at(y0 + 1, x0), d11 = at(y0 + 1, x0 + 1);
    const double d0 = d00 + (d01 - d00) * fx, d1 = d10 + (d11 - d10) * fx;
    rings[(size_t)blockIdx.y * nsamples + t] = d0 + (d1 - d0) * fy;
}

// block = (ring, image): the ring's samples and the nsam twiddles in LDS, thread k sums sample s against twiddle (s k) mod nsam
__global__ void __launch_bounds__(256) k_es_ring_dft(const double *__restrict__ rings, const EsRing *__restrict__ ringTab, int nsamples, int ncoefs, int conjugate,
                                                     double2 *__restrict__ coefs)
{
    extern __shared__ double es_lds[];
    const EsRing R = ringTab[blockIdx.x];
    const int n = R.nsam;
    double *x = es_lds;
    double2 *tw = (double2 *)(es_lds + n + (n & 1));
    const double *src = rings + (size_t)blockIdx.y * nsamples + R.soff;
    for (int s = threadIdx.x; s < n; s += 256) {
        x[s] = src[s];
        double sn, cs;
        sincospi(2.0 * (double)s / (double)n, &sn, &cs);
        tw[s] = double2{cs, sn};
    }
    __syncthreads();
    const double inv = 1.0 / n;
    for (int k = threadIdx.x; k <= n / 2; k += 256) {
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int s = 0; s < n; ++s) {
            const double2 t = tw[idx];
            const double v = x[s];
            re += v * t.x;
            im -= v * t.y;
            idx += k;
            if (idx >= n) idx -= n;
        }
        re *= inv; im *= inv;
        if (conjugate) im = -im;
        coefs[(size_t)blockIdx.y * ncoefs + R.coff + k] = double2{re, im};
    }
}

// Fsum[k] = sum over the rings that have frequency k of 2 pi r . F1[k] F2[k] (F2 arrives conjugated), polar.cpp:122-135
__device__ __forceinline__ double2 es_rot_fsum_at(const double2 *__restrict__ Fref, const double2 *__restrict__ f2, const EsRing *__restrict__ ringTab, int nrings, int k)
{
    double re = 0.0, im = 0.0;
    for (int r = 0; r < nrings; ++r) {
        const EsRing R = ringTab[r];
        if (k > R.nsam / 2) continue;
        const double2 a = Fref[R.coff + k], c = f2[R.coff + k];
        re += R.w * (a.x * c.x - a.y * c.y);
        im += R.w * (a.y * c.x + a.x * c.y);
    }
    return double2{re, im};
}

// the inverse transform of the Hermitian half Fsum over len = 2 nh - 1 (odd) angles, un-normalised: corr[j] = Re F0 + 2 sum_k Re(F_k e^{2 pi i j k / len})
__global__ void __launch_bounds__(256) k_es_rot_corr(const double2 *__restrict__ Fsum, int nh, int len, double *__restrict__ corr)
{
    extern __shared__ double es_lds[];
    double2 *F = (double2 *)es_lds;
    const double2 *src = Fsum + (size_t)blockIdx.y * nh;
    for (int k = threadIdx.x; k < nh; k += 256) F[k] = src[k];
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= len) return;
    double acc = 0.0;
    int idx = 0;
    const double step = 2.0 / (double)len;
    for (int k = 1; k < nh; ++k) {
        idx += j;
        if (idx >= len) idx -= len;
        double sn, cs;
        sincospi(step * (double)idx, &sn, &cs);
        acc += F[k].x * cs - F[k].y * sn;
    }
    corr[(size_t)blockIdx.y * len + j] = F[0].x + 2.0 * acc;
}

// best_rotation (polar.cpp:218-229): the first element that is strictly greater than everything before it
__global__ void __launch_bounds__(256) k_es_first_max(const double *__restrict__ corr, int len, int *__restrict__ imax)
{
    __shared__ double sv[256];
    __shared__ int si[256];
    const double *c = corr + (size_t)blockIdx.x * len;
    double best = c[0];
    int bi = 0;
    for (int i = threadIdx.x; i < len; i += 256)
        if (c[i] > best) { best = c[i]; bi = i; }
    sv[threadIdx.x] = best; si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double v = sv[threadIdx.x + o];
            const int k = si[threadIdx.x + o];
            if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && k < si[threadIdx.x])) { sv[threadIdx.x] = v; si[threadIdx.x] = k; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) imax[blockIdx.x] = si[0];
}
}  // namespace

// the rotation estimator's plan: ring table and sample coordinates on the device, the reference's polar Fourier transform
struct EsRotation {
    xh_ctx *ctx = nullptr;
    int D = 0, first = 0, last = 0, nrings = 0, nsamples = 0, ncoefs = 0, N = 0, len = 0, maxNsam = 0;
    XhBuf ringTab, sx, sy, Fref, rings, coefs, Fsum, corr, imax;
};

// polarFourierTransform<false>(..., BsplineOrder = 1) of n images [n][D][D] (float) into coefs [n][ncoefs]
static int es_rotation_transform(EsRotation &R, const float *d_imgs, int n, int conjugate, double2 *d_coefs)
{
    xh_ctx *ctx = R.ctx;
    XH_TRY(xh_buf_reserve(ctx, R.rings, sizeof(double) * (size_t)R.nsamples * n));
    hipLaunchKernelGGL(k_es_polar_linear, dim3((unsigned)((R.nsamples + 255) / 256), n), dim3(256), 0, ctx->stream, d_imgs, (const float *)R.sx.p, (const float *)R.sy.p, R.nsamples,
                       R.D, (double *)R.rings.p);
    XH_LAUNCH_CHECK();
    const size_t smem = sizeof(double) * (size_t)(R.maxNsam + (R.maxNsam & 1)) + sizeof(double2) * (size_t)R.maxNsam;
    hipLaunchKernelGGL(k_es_ring_dft, dim3(R.nrings, n), dim3(256), smem, ctx->stream, (const double *)R.rings.p, (const EsRing *)R.ringTab.p, R.nsamples, R.ncoefs, conjugate,
                       d_coefs);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

// the plan without a reference: ring table, sample coordinates and the buffer of the reference's transform (ncoefs per reference)
static int es_rotation_plan(xh_ctx *ctx, int32_t D, int32_t first_ring, int32_t last_ring, EsRotation &R)
{
    // RotationEstimationSetting::check + PolarRotationEstimator::check (arotation_estimator.h:80-130, polar_rotation_estimator.cpp:125-141)
    XH_CHECK(D >= 6, XH_ERR_ARG, "xh_rotation_estimate: The input signal is too small.");
    XH_CHECK(first_ring >= 1 && last_ring > first_ring && last_ring < D, XH_ERR_ARG, "xh_rotation_estimate: rings %d .. %d of a %d px image (first >= 1, last > first, last < size)",
             first_ring, last_ring, D);
    R.ctx = ctx; R.D = D; R.first = first_ring; R.last = last_ring; R.nrings = last_ring - first_ring + 1;
    std::vector<EsRing> tab(R.nrings);
    int ns = 0, nc = 0;
    for (int r = 0; r < R.nrings; ++r) {
        const float radius = (float)r + first_ring;
        int nsam = 2 * (int)(0.5 * 1.0 * 6.2831853071795864769 * radius);          // getNoOfSamples, polar.h:723-726
        nsam = nsam > 1 ? nsam : 1;
        tab[r].nsam = nsam; tab[r].soff = ns; tab[r].coff = nc;
        tab[r].w = 2. * 3.14159265358979323846 * (double)radius;                     // polar.cpp:123
        ns += nsam; nc += nsam / 2 + 1;
        R.maxNsam = nsam > R.maxNsam ? nsam : R.maxNsam;
    }
    R.nsamples = ns; R.ncoefs = nc; R.N = tab[R.nrings - 1].nsam; R.len = 2 * R.N - 1;
    const size_t smem = sizeof(double) * (size_t)(R.maxNsam + (R.maxNsam & 1)) + sizeof(double2) * (size_t)R.maxNsam;
    XH_CHECK(smem <= 160 * 1024 && sizeof(double2) * (size_t)R.N <= 160 * 1024, XH_ERR_UNSUPPORTED, "xh_rotation_estimate: a ring of %d samples does not fit the 160 KB of LDS", R.maxNsam);
    XH_HIP(hipFuncSetAttribute((const void *)k_es_ring_dft, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    XH_HIP(hipFuncSetAttribute((const void *)k_es_rot_corr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double2) * (size_t)R.N)));
    // the angle cache of Polar<T>::ensureAngleCache (polar.cpp:57-83): float angle, float product, stored as floats
    std::vector<float> sx(ns), sy(ns);
    for (int r = 0; r < R.nrings; ++r) {
        const float radius = (float)(r + first_ring);
        const int n = tab[r].nsam;
        const float dphi = (float)(6.2831853071795864769 / (float)n);
        for (int i = 0; i < n; ++i) {
            const float phi = i * dphi;
            sx[tab[r].soff + i] = sinf(phi) * radius;
            sy[tab[r].soff + i] = cosf(phi) * radius;
        }
    }
    XH_TRY(xh_buf_alloc(ctx, R.ringTab, sizeof(EsRing) * tab.size()));
    XH_TRY(xh_buf_alloc(ctx, R.sx, sizeof(float) * ns));
    XH_TRY(xh_buf_alloc(ctx, R.sy, sizeof(float) * ns));
    XH_TRY(xh_buf_alloc(ctx, R.Fref, sizeof(double2) * nc));
    XH_HIP(hipMemcpyAsync(R.ringTab.p, tab.data(), sizeof(EsRing) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
    XH_HIP(hipMemcpyAsync(R.sx.p, sx.data(), sizeof(float) * ns, hipMemcpyHostToDevice, ctx->stream));
    XH_HIP(hipMemcpyAsync(R.sy.p, sy.data(), sizeof(float) * ns, hipMemcpyHostToDevice, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));                // the host vectors go out of scope
    return XH_OK;
}

static int es_rotation_create(xh_ctx *ctx, const float *d_ref, int32_t D, int32_t first_ring, int32_t last_ring, EsRotation &R)
{
    XH_TRY(es_rotation_plan(ctx, D, first_ring, last_ring, R));
    return es_rotation_transform(R, d_ref, 1, 0, (double2 *)R.Fref.p);                // load2DReferenceOneToN: not conjugated
}

#endif
