// xh_image2d.h -- the particle-image pieces shared by the continuous assignment (xh_ca2.hip), the Zernike3D alignment (xh_asa.hip) and
// the Zernike3D ART reconstruction (xh_faz.hip), in doubles: FourierFilter's raised-cosine low pass with a row's CTF factor
// (xh_k_lowpass_ctf), its CTFINV mask (xh_k_ctfinv), the particle load through the low pass (xh_lowpass_images), the 2-D circular mask,
// applyGeometry's LINEAR branch and the masked correlation index of a cost kernel.
#ifndef XH_IMAGE2D_H
#define XH_IMAGE2D_H
#include "xh_common.h"
#include "xh_plan.h"
#include "xh_reduce.h"
#include "xh_ctf.h"
#include <algorithm>
#include <vector>

namespace {
const double kAcc = 1e-6;       // XMIPP_EQUAL_ACCURACY

// FourierFilter LOWPASS / RAISED_COSINE (fourier_filter.cpp:423-432) at the digital frequency absw
__device__ __forceinline__ double d_lowpass_raised_cosine(double absw, double w1, double raised_w)
{
    double m;
    if (absw < w1) m = 1;
    else if (absw < w1 + raised_w) m = (1 + cos(3.14159265358979323846 / raised_w * (absw - w1))) / 2;
    else m = 0;
    return m;
}

// what xh_k_lowpass_ctf multiplies into the low pass: nothing, the damping envelope of generateEnvelope (ctf.h:1271-1290), or FilterCTF's
// mask (generateCTF at K = 1 without the noise model, its absolute value when the particles were phase flipped)
enum { XH_FACTOR_NONE, XH_FACTOR_ENVELOPE, XH_FACTOR_CTF };

// The raised-cosine low pass on the full spectra F [images][D][D], the 1 / D^2 of the inverse folded in, times the image's CTF factor.
// rows: one row of `stride` doubles per image; rows[ctf] != 0 says the image has a CTF, and its CtfSide follows at rows[ctf + 1].
// Low pass and factor are real and even, so one pass over the full spectrum of a real image is the reference's passes over the half
// spectrum. The factor is taken at the HALF-SPECTRUM index of (i, j): (i, j) itself for j <= D / 2, else the mirrored (-i, -j). The
// two are the same frequency up to sign, but the factor is computed from rounded coordinates, and only one index per conjugate pair
// gives both cells the same bits: the product stays Hermitian and the inverse transform real. Where the low pass is exactly 0 the
// factor is not evaluated (it is finite: a load refuses non-finite CTF parameters; the product is 0 either way).
template <int FACTOR>
__global__ void __launch_bounds__(256)
xh_k_lowpass_ctf(xh_cd *__restrict__ F, size_t total, int D, double w1, double raised_w, const double *__restrict__ rows, int stride, int ctf,
                 double iTs, int phaseFlipped)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = idx % D, i = (idx / D) % D;
    const double fy = d_digfreq(i, D), fx = d_digfreq(j, D);
    double m = d_lowpass_raised_cosine(sqrt(fx * fx + fy * fy), w1, raised_w);
    m /= (double)D * (double)D;
    if (FACTOR != XH_FACTOR_NONE && m != 0.0) {
        const double *q = rows + (size_t)stride * (idx / ((size_t)D * D)) + ctf;
        if (q[0] != 0.0) {
            D_CTF_SIDE_FROM_ROW(s, q + 1)
            int ih = i, jh = j;
            if (jh > D / 2) { jh = D - jh; ih = (D - ih) % D; }
            const double X = d_digfreq(jh, D) * iTs, Y = d_digfreq(ih, D) * iTs;
            if (FACTOR == XH_FACTOR_ENVELOPE) m *= d_ctf_envelope(s, X, Y);
            else {
                double v = d_ctf_at(s, X, Y, true);
                if (phaseFlipped) v = fabs(v);
                m *= v;
            }
        }
    }
    const xh_cd v = F[idx];
    F[idx] = xh_cd{v.x * m, v.y * m};
}

// FourierFilter CTFINV (fourier_filter.cpp:533-541) on the full spectra F [images][D][D], the 1 / D^2 of the inverse folded in: 0 where
// |ctf| <= minCTF, else 1 / ctf, with ctf = getValueAt with its damping (its absolute value when phaseFlipped); an image whose row says it
// has no CTF is only normalised. Rows and the half-spectrum index are those of xh_k_lowpass_ctf. A template, so that only the files that
// launch it hold it.
template <bool PHASE_FLIPPED>
__global__ void __launch_bounds__(256)
xh_k_ctfinv(xh_cd *__restrict__ F, size_t total, int D, const double *__restrict__ rows, int stride, int ctf, double iTs, double minCTF)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = idx % D, i = (idx / D) % D;
    double m = 1.0 / ((double)D * (double)D);
    const double *q = rows + (size_t)stride * (idx / ((size_t)D * D)) + ctf;
    if (q[0] != 0.0) {
        D_CTF_SIDE_FROM_ROW(s, q + 1)
        int ih = i, jh = j;
        if (jh > D / 2) { jh = D - jh; ih = (D - ih) % D; }
        double v = d_ctf_at(s, d_digfreq(jh, D) * iTs, d_digfreq(ih, D) * iTs, true);
        if (PHASE_FLIPPED) v = fabs(v);
        m = fabs(v) <= minCTF ? 0.0 : m / v;
    }
    const xh_cd v = F[idx];
    F[idx] = xh_cd{v.x * m, v.y * m};
}

// n host float images [D][D] -> their low pass (w1, raised_w = 0.02) as doubles at d_out [n][D][D], in chunks of at most 256 MiB of
// spectra: float -> complex, forward, filter, inverse, real part. d_rows (nullable): a row per image whose envelope goes into the filter.
int xh_lowpass_images(xh_ctx *ctx, const XhFft2d64 &fft, const float *h_images, int n, int D, double w1, double iTs, const double *d_rows,
                      int stride, int ctf, double *d_out)
{
    const size_t DD = (size_t)D * D;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(n, ((size_t)256 << 20) / (DD * sizeof(xh_cd))));
    XhBuf d_img, d_F;
    XH_TRY(xh_buf_alloc(ctx, d_img, sizeof(float) * DD * chunk));
    XH_TRY(xh_buf_alloc(ctx, d_F, sizeof(xh_cd) * DD * chunk));
    xh_cd *F = (xh_cd *)d_F.p;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        const size_t total = DD * m;
        const unsigned g = (unsigned)((total + 255) / 256);
        XH_HIP(hipMemcpyAsync(d_img.p, h_images + DD * i0, sizeof(float) * total, hipMemcpyHostToDevice, ctx->stream));
        XH_LAUNCH256(ctx, xh_k_to_complex64<float>, g, (const float *)d_img.p, F, total);
        XH_TRY(xh_fft2d64(ctx, fft, F, m, false));
        if (d_rows) XH_LAUNCH256(ctx, xh_k_lowpass_ctf<XH_FACTOR_ENVELOPE>, g, F, total, D, w1, 0.02, d_rows + (size_t)stride * i0, stride, ctf, iTs, 0);
        else XH_LAUNCH256(ctx, xh_k_lowpass_ctf<XH_FACTOR_NONE>, g, F, total, D, w1, 0.02, (const double *)nullptr, 0, 0, iTs, 0);
        XH_TRY(xh_fft2d64(ctx, fft, F, m, true));
        XH_LAUNCH256(ctx, xh_k_real64<double>, g, (const xh_cd *)F, d_out + DD * i0, total);
        XH_HIP(hipStreamSynchronize(ctx->stream));
    }
    return XH_OK;
}

// BINARY_CIRCULAR_MASK, INNER_MASK, R1 = R about the Xmipp origin, [D][D] on the device; R = 0 is the empty mask, which is refused.
// *nmask: the pixels inside.
int xh_circular_mask2d(xh_ctx *ctx, const char *who, int D, double R, XhBuf &d_mask, int *nmask)
{
    std::vector<int32_t> mask((size_t)D * D);
    XH_TRY(xh_halves_circular_mask(1, D, D, -R, 0, 0, 0, mask.data()));
    if (R == 0) for (auto &v : mask) v = 0;
    *nmask = 0;
    for (int32_t v : mask) *nmask += v;
    XH_CHECK(*nmask > 0, XH_ERR_ARG, "%s: the mask of radius %g is empty", who, R);
    return xh_buf_upload(ctx, d_mask, mask.data(), sizeof(int32_t) * mask.size());
}

// applyGeometry's 2-D LINEAR branch at one output pixel (i, j), DONT_WRAP, outside 0; A is the matrix already inverted (rows 0 and 1).
// The same interpolation as xh_apply_geometry2d's, in doubles.
__device__ __forceinline__ double d_ca2_linear(const double *__restrict__ V1, int D, const double *A, int i, int j)
{
    const int cen = D / 2;
    const double minp = -cen - kAcc, maxp = (D - cen - 1) + kAcc;
    const double x = (double)(j - cen), y = (double)(i - cen);
    const double xp = x * A[0] + y * A[1] + A[2], yp = x * A[3] + y * A[4] + A[5];
    if (!(xp >= minp && xp <= maxp && yp >= minp && yp <= maxp)) return 0.0;      // a NaN coordinate is outside, too
    double wx = xp + cen;
    const int m1 = (int)wx;
    wx = wx - m1;
    const int m2 = m1 + 1;
    double wy = yp + cen;
    const int n1 = (int)wy;
    wy = wy - n1;
    const int n2 = n1 + 1;
    const double wx_1 = 1 - wx, wy_1 = 1 - wy;
    double aux2 = wy_1 * wx_1;
    double tmp = aux2 * V1[(size_t)n1 * D + m1];
    if (wx != 0 && m2 < D) tmp += (wy_1 - aux2) * V1[(size_t)n1 * D + m2];
    if (wy != 0 && n2 < D) {
        aux2 = wy * wx_1;
        tmp += aux2 * V1[(size_t)n2 * D + m1];
        if (wx != 0 && m2 < D) tmp += (wy - aux2) * V1[(size_t)n2 * D + m2];
    }
    return tmp;
}

// correlationIndex(x, y, mask) of one image pair per 256-thread workgroup, the tail of a cost kernel. Thread t has visited the pixels
// n = t, t + 256, .. < DD: it wrote x[n] and y[n], and over those inside the mask it brings s0 = sum x, s1 = sum y, s2 = sum x^2,
// s3 = sum y^2. Population sigmas over the nmask pixels; 0 when one is below XMIPP_EQUAL_ACCURACY, else the second pass' sum of
// (x - mean x)(y - mean y) over (sigma x sigma y) nmask. Every sum goes through the fixed tree of xh_reduce.h; every thread returns the
// same value.
__device__ __forceinline__ double d_masked_correlation(double s0, double s1, double s2, double s3, const int *__restrict__ mask, const double *x,
                                                       const double *y, int DD, double nmask, double (&red)[1][256])
{
    s0 = xh_block_sum(s0, red);
    s1 = xh_block_sum(s1, red);
    s2 = xh_block_sum(s2, red);
    s3 = xh_block_sum(s3, red);
    const double mx = s0 / nmask, my = s1 / nmask;
    const double sx = sqrt(fabs(s2 / nmask - mx * mx)), sy = sqrt(fabs(s3 / nmask - my * my));
    if (fabs(sx) < kAcc || fabs(sy) < kAcc) return 0.0;      // uniform over the workgroup: every thread holds the same sums
    double r = 0;
    for (int n = threadIdx.x; n < DD; n += 256)
        if (mask[n]) r += (x[n] - mx) * (y[n] - my);      // both were written by this thread
    r = xh_block_sum(r, red);
    return r / ((sx * sy) * nmask);
}
}  // namespace

#endif
