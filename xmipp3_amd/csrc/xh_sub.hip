// xh_sub.hip -- xmipp_subtract_projection on the device (gfx950): project the refined volume at each particle's pose, fit the
// projection to the particle in Fourier space, remove it, keeping or removing the region of a 3-D mask.
// Reference: libraries/reconstruction/subtract_projection.cpp -- createMask (L177-197), applyCTF (L217-240), processParticle (L242-301),
// evaluateFitting / checkBestModel (L323-364), preProcess (L514-632), processImage (L634-826). Everything is fp64; the reference runs one
// particle at a time on CPU threads, here `capacity` particles go through one stream of kernels and one wait for the results.
//
//   create : vM / ivM (createMask), V *= ivM, the projector (FourierProjector through xh_fp_create, or xh_rsp in value mode for
//            --realSpaceProjection), xh_rsp in support mode for vM and for the --mask volume, the circle RaisedCosineMask(R, R) (r1 == r2:
//            a binary disc, data/mask.cpp:36-65), the frequency map wi and maxwiIdx (L554-580), the cells of the half spectrum grouped by wi
//   run    : per chunk  P (projector; Fourier path: selfTranslate(LINEAR, -shift, WRAP))  ->  Pctf (window to padding D, half spectrum times
//            getValueAt() at Tm = sampling, back, crop)  ->  PmaskImg, M, iM  ->  b, I -= b  ->  the four spectra  ->  the sums per wi
//            (fixed tree of xh_reduce.h)  ->  the fit (sub_fit, the code of the host's xh_sub_fit, one thread per particle)  ->  the two
//            models against IFourier, checkBestModel  ->  the chosen model (or IFourier / T(w) with --boost) back to real space, Idiff.
//
// As written, kept: wi takes YSIZE on both axes; cutFreq halves sampling / maxResol and substractionCutFreq divides it by sqrt(2); the
// padded window runs from (int)padding STARTING to (int)padding FINISHING, so it has (int)padding (D - 1) + 1 pixels; b is taken from I
// after the mask and from P before the mask; I -= b on every pixel and IFourier is not recomputed; A1(1,1) += 2 win and
// A1(0,1) += win (re + im); PFourier0 is scaled only where wi < maxwiIdx, PFourier1 everywhere and then (0,0) := IiMFourier(0,0).
// applyCTF writes its result back into the projection it was given (mpad.window(mproj, ..), L237), so for a particle with a CTF the P of
// the background adjustment b is the projection after the CTF; the `last` hook returns both.
//
// Deviations:
//   - xh_fp_create takes floats: on the Fourier path the masked volume is rounded to float (exact for a binary mask on a float volume).
//   - transforms are full complex [D][D] transforms; sums and models read the half spectrum j <= D / 2 out of them, and a cell beyond it
//     takes the factor of its mirrored cell, as the half-spectrum transform implies.
//   - the per-wi sums go through the fixed tree and the bins are then added in increasing wi; A1(0,0) is the sum of den0's bins.
//   - solveLinearSystem is restated as least squares through the normal equations with the closed 2 x 2 inverse; xmippCore is not in the
//     tree (parity unpinned). The same holds for applyGeometry's WRAP branch behind selfTranslate.
// The fit compares and divides doubles whose last bits matter to the host twin: this file is built with -ffp-contract=off.
#include "xh_common.h"
#include "xh_fft.h"
#include "xh_plan.h"
#include "xh_reduce.h"
#include "xh_ctf.h"
#include "xh_image2d.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {
const int kRow = 32;          // doubles per particle row on the device: E[9], shift x, y, has CTF, CtfSide[18], pad
const int kRowCtf = 11;       // rows[kRowCtf] != 0: the CtfSide follows (the layout xh_k_lowpass_ctf reads)
const int kSubStages = 7;     // the stages a timed run reports: projection, CTF, masks, prepare + spectra, sums + fit, models, output
const int kRes = 8;           // doubles per result: R2adj, beta0, beta1, b, model, disable, beta00, R20adj

// the fit of L732-759 from the per-wi sums S [bins][4] = num0, den0, sum(re + im) of PiMFourier, sum(re + im) of IiMFourier;
// a11 = sum 2 win. out: beta00, beta01, beta1
__host__ __device__ inline void sub_fit(const double *S, int maxwi, double a11, double *out)
{
    double num = 0, den = 0, a01 = 0, b11 = 0;
    for (int w = 1; w < maxwi; ++w) {
        num += S[4 * w];
        den += S[4 * w + 1];
        a01 += (double)w * S[4 * w + 2];
        b11 += (double)w * S[4 * w + 3];
    }
    out[0] = num / den;
    // solveLinearSystem: (A^t A)^-1 A^t b with A = [den a01; a01 a11], b = (num, b11)
    const double A00 = den, A01 = a01, A10 = a01, A11 = a11;
    const double M00 = A00 * A00 + A10 * A10, M01 = A00 * A01 + A10 * A11, M10 = A01 * A00 + A11 * A10, M11 = A01 * A01 + A11 * A11;
    const double v0 = A00 * num + A10 * b11, v1 = A01 * num + A11 * b11;
    const double idet = 1.0 / (M00 * M11 - M01 * M10);
    const double I00 = M11 * idet, I01 = -M01 * idet, I10 = -M10 * idet, I11 = M00 * idet;
    out[1] = I00 * v0 + I01 * v1;
    out[2] = I10 * v0 + I11 * v1;
}

// evaluateFitting twice and checkBestModel (L323-364) from the sums over the `size` cells of the half spectrum. out: R2adj, model, R20adj
__host__ __device__ inline void sub_choose(double sumY, double sumY2, double sumE0, double sumE1, double size, double *out)
{
    const double meanY = sumY / (2.0 * size);
    const double varY = sumY2 / (2.0 * size) - meanY * meanY;
    const double R20adj = 1.0 - (sumE0 / (2.0 * size)) / varY;
    const double R21 = 1.0 - (sumE1 / (2.0 * size)) / varY;
    const double N = 2.0 * size;
    const double R21adj = 1.0 - (1.0 - R21) * (N - 1.0) / (N - 2.0);
    if (R21adj > R20adj) { out[0] = R21adj; out[1] = 1; }
    else { out[0] = R20adj; out[1] = 0; }
    out[2] = R20adj;
}

// selfTranslate(LINEAR, P, roffset, WRAP) = applyGeometry(LINEAR, ., translation(roffset), IS_NOT_INV, WRAP): one thread per row of one
// image walks the row as the reference does (xp += 1 per pixel, a wrapped coordinate is carried on). tx, ty: -roffset = the shift.
__global__ void __launch_bounds__(64)
k_sub_translate(const double *__restrict__ in, const double *__restrict__ rows, double *__restrict__ out, int D, int m)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= m * D) return;
    const int p = t / D, i = t - p * D;
    const double *V1 = in + (size_t)p * D * D;
    double *V2 = out + (size_t)p * D * D + (size_t)i * D;
    const double tx = rows[(size_t)kRow * p + 9], ty = rows[(size_t)kRow * p + 10];
    if (fabs(tx) < kAcc && fabs(ty) < kAcc) {               // A.isIdentity(): the input is copied
        for (int j = 0; j < D; ++j) V2[j] = V1[(size_t)i * D + j];
        return;
    }
    const int cen = D / 2;
    const double minxp = -cen, maxxp = D - cen - 1;
    const double minxpp = minxp - kAcc, maxxpp = maxxp + kAcc;
    const double lo = minxp - 0.5, hi = maxxp + 0.5;
    const double x = -cen, y = i - cen;
    double xp = x * 1.0 + y * 0.0 + tx, yp = x * 0.0 + y * 1.0 + ty;
    for (int j = 0; j < D; ++j) {
        if (xp < minxpp || xp > maxxpp) {                     // realWRAP(xp, minxp - 0.5, maxxp + 0.5)
            if (!(xp >= lo && xp <= hi)) xp = xp < lo ? xp - (int)((xp - lo) / (hi - lo) - 1) * (hi - lo) : xp - (int)((xp - hi) / (hi - lo) + 1) * (hi - lo);
        }
        if (yp < minxpp || yp > maxxpp) {
            if (!(yp >= lo && yp <= hi)) yp = yp < lo ? yp - (int)((yp - lo) / (hi - lo) - 1) * (hi - lo) : yp - (int)((yp - hi) / (hi - lo) + 1) * (hi - lo);
        }
        double wx = xp + cen;
        int m1 = (int)wx;
        wx = wx - m1;
        int m2 = m1 + 1;
        double wy = yp + cen;
        int n1 = (int)wy;
        wy = wy - n1;
        int n2 = n1 + 1;
        if (m2 >= D) m2 = 0;
        if (n2 >= D) n2 = 0;
        // a coordinate the wrap left outside (a shift too large for its integer cast) stays inside the image
        m1 = min(max(m1, 0), D - 1);
        n1 = min(max(n1, 0), D - 1);
        m2 = min(max(m2, 0), D - 1);
        n2 = min(max(n2, 0), D - 1);
        const double wx_1 = 1 - wx, wy_1 = 1 - wy;
        double aux2 = wy_1 * wx_1;
        double tmp = aux2 * V1[(size_t)n1 * D + m1];
        if (wx != 0 && m2 < D) tmp += (wy_1 - aux2) * V1[(size_t)n1 * D + m2];
        if (wy != 0 && n2 < D) {
            aux2 = wy * wx_1;
            tmp += aux2 * V1[(size_t)n2 * D + m1];
            if (wx != 0 && m2 < D) tmp += (wy - aux2) * V1[(size_t)n2 * D + m2];
        }
        V2[j] = tmp;
        xp += 1.0;
        yp += 0.0;
    }
}

// the particles as doubles
__global__ void __launch_bounds__(256) k_sub_widen(const float *__restrict__ in, double *__restrict__ out, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < total) out[idx] = (double)in[idx];
}

// mproj.window(mpad, pad STARTING .., pad FINISHING ..) (L232): P [m][D][D] -> complex [m][Np][Np], zero outside
__global__ void __launch_bounds__(256)
k_sub_pad(const double *__restrict__ P, xh_cd *__restrict__ F, int D, int Np, int off, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = idx % Np, i = (idx / Np) % Np;
    const size_t p = idx / ((size_t)Np * Np);
    const int jj = j - off, ii = i - off;
    double v = 0;
    if (jj >= 0 && jj < D && ii >= 0 && ii < D) v = P[(p * D + ii) * D + jj];
    F[idx] = xh_cd{v, 0.0};
}

// mpad.window(mproj, ..) (L237): the crop back; a row without a CTF keeps its projection
__global__ void __launch_bounds__(256)
k_sub_crop(const xh_cd *__restrict__ F, const double *__restrict__ P, const double *__restrict__ rows, double *__restrict__ Pc, int D, int Np, int off,
           size_t total)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = idx % D, i = (idx / D) % D;
    const size_t p = idx / ((size_t)D * D);
    Pc[idx] = rows[(size_t)kRow * p + kRowCtf] != 0.0 ? F[(p * Np + i + off) * Np + j + off].x : P[idx];
}

// L289-296, L644-703 for one particle per workgroup: the masks, b, I -= b, and the four real images whose spectra the fit needs, written as
// complex: F[0] = Pctf, F[1] = I (both zeroed outside PmaskImg), F[2] = (I - b) iM, F[3] = Pctf iM; stride between them `plane`.
// Pmask: per particle (pmStride = DD) or one shared disc (0). M: the support projection of vM, or null (no ROI mask: M = 0).
__global__ void __launch_bounds__(256)
k_sub_prepare(const double *__restrict__ Pc, const double *__restrict__ I, const double *__restrict__ Pmask, size_t pmStride, const double *__restrict__ M,
              int subtract, double *__restrict__ iMout, double *__restrict__ I2, double *__restrict__ bout, xh_cd *__restrict__ F, size_t plane, int DD)
{
    __shared__ double red[3][256];
    const int p = blockIdx.x, tid = threadIdx.x;
    const double *pc = Pc + (size_t)p * DD, *im = I + (size_t)p * DD, *pm = Pmask + pmStride * p;
    const double *mm = M ? M + (size_t)p * DD : nullptr;
    double v[3] = {0, 0, 0};
    for (int n = tid; n < DD; n += 256) {
        const double mv = mm ? mm[n] : 0.0;
        const double iM = subtract && mm ? mv : mv * (-1) + 1;
        const bool in = pm[n] > 0;
        if (iM > 0 && in) { v[0] += pc[n]; v[1] += im[n]; v[2] += 1.0; }
    }
    xh_tree256(red, v);
    const double b = (red[1][0] - red[0][0]) / red[2][0];
    if (tid == 0) bout[p] = b;
    xh_cd *f = F + (size_t)p * DD;
    for (int n = tid; n < DD; n += 256) {
        const double mv = mm ? mm[n] : 0.0;
        const double iM = subtract && mm ? mv : mv * (-1) + 1;
        const bool in = pm[n] > 0;
        const double pv = in ? pc[n] : 0.0, iv = in ? im[n] : 0.0;
        const double i2 = iv - b;
        iMout[(size_t)p * DD + n] = iM;
        I2[(size_t)p * DD + n] = i2;
        f[n] = xh_cd{pv, 0.0};
        f[plane + n] = xh_cd{iv, 0.0};
        f[2 * plane + n] = xh_cd{i2 * iM, 0.0};
        f[3 * plane + n] = xh_cd{pv * iM, 0.0};
    }
}

// the sums of L714-729 for one wi of one particle per workgroup: S [m][bins][4]. cells: the half spectrum's cells (as indices into the full
// [D][D] spectrum) grouped by wi, binStart [bins + 1]
__global__ void __launch_bounds__(256)
k_sub_bins(const xh_cd *__restrict__ F, size_t plane, const int *__restrict__ cells, const int *__restrict__ binStart, double *__restrict__ S, int bins,
           int DD, double inv)
{
    __shared__ double red[4][256];
    const int w = blockIdx.x, p = blockIdx.y;
    const xh_cd *Fi = F + 2 * plane + (size_t)p * DD, *Fp = F + 3 * plane + (size_t)p * DD;
    double v[4] = {0, 0, 0, 0};
    for (int k = binStart[w] + threadIdx.x; k < binStart[w + 1]; k += 256) {
        const int c = cells[k];
        const double pr = Fp[c].x * inv, pi = Fp[c].y * inv, ir = Fi[c].x * inv, ii = Fi[c].y * inv;
        v[0] += ir * pr + ii * pi;
        v[1] += pr * pr + pi * pi;
        v[2] += pr + pi;
        v[3] += ir + ii;
    }
    xh_tree256(red, v);
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; ++c) S[((size_t)p * bins + w) * 4 + c] = red[c][0];
}

__global__ void k_sub_fit(const double *__restrict__ S, int bins, int maxwi, double a11, double *__restrict__ beta, int m)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < m) sub_fit(S + (size_t)p * bins * 4, maxwi, a11, beta + 3 * (size_t)p);
}

// L741-768 for one particle per workgroup: PFourier0 and PFourier1 against IFourier over the half spectrum, then checkBestModel and the
// row's results. wiHalf [D][D/2+1]
__global__ void __launch_bounds__(256)
k_sub_models(const xh_cd *__restrict__ F, size_t plane, const int *__restrict__ wiHalf, const double *__restrict__ beta, const double *__restrict__ bvals,
             double *__restrict__ res, int D, int maxwi, int nonNegative, double inv)
{
    __shared__ double red[4][256];
    const int p = blockIdx.x, xh = D / 2 + 1, DD = D * D;
    const xh_cd *Fp = F + (size_t)p * DD, *Fi = F + plane + (size_t)p * DD, *Fim = F + 2 * plane + (size_t)p * DD;
    const double beta00 = beta[3 * p], beta01 = beta[3 * p + 1], beta1 = beta[3 * p + 2];
    double v[4] = {0, 0, 0, 0};
    for (int n = threadIdx.x; n < D * xh; n += 256) {
        const int i = n / xh, j = n - i * xh, c = i * D + j, win = wiHalf[n];
        const double yr = Fi[c].x * inv, yi = Fi[c].y * inv, pr = Fp[c].x * inv, pi = Fp[c].y * inv;
        const double t1 = beta01 + beta1 * win;
        double p0r = pr, p0i = pi;
        if (win < maxwi) { p0r *= beta00; p0i *= beta00; }
        double p1r = pr * t1, p1i = pi * t1;
        if (n == 0) { p1r = Fim[0].x * inv; p1i = Fim[0].y * inv; }
        v[0] += yr + yi;
        v[1] += yr * yr + yi * yi;
        const double e0r = yr - p0r, e0i = yi - p0i, e1r = yr - p1r, e1i = yi - p1i;
        v[2] += e0r * e0r + e0i * e0i;
        v[3] += e1r * e1r + e1i * e1i;
    }
    xh_tree256(red, v);
    if (threadIdx.x == 0) {
        double o[3];
        sub_choose(red[0][0], red[1][0], red[2][0], red[3][0], (double)D * xh, o);
        double *r = res + (size_t)kRes * p;
        const int model = (int)o[1];
        r[0] = o[0];
        r[1] = model == 0 ? beta00 : beta01;
        r[2] = model == 0 ? 0.0 : beta1;
        r[3] = bvals[p];
        r[4] = model;
        r[5] = (nonNegative && beta00 < 0) ? 1.0 : 0.0;
        r[6] = beta00;
        r[7] = o[2];
    }
}

// the spectrum that goes back to real space (L789-807), over the full [D][D] cells into plane 0 of G: the chosen model of PFourier, or with
// boost IFourier / T(w). wiFull: wi of the cell's half-spectrum twin
__global__ void __launch_bounds__(256)
k_sub_spectrum(const xh_cd *__restrict__ F, size_t plane, const int *__restrict__ wiFull, const double *__restrict__ beta, const double *__restrict__ res,
               xh_cd *__restrict__ G, int DD, int maxwi, int boost, double inv, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t p = idx / DD;
    const int c = idx - p * DD, win = wiFull[c];
    const int model = (int)res[(size_t)kRes * p + 4];
    const double beta00 = beta[3 * p], t1 = beta[3 * p + 1] + beta[3 * p + 2] * win;
    xh_cd o;
    if (boost) {
        const xh_cd y = F[plane + idx];
        const double t = model == 0 ? beta00 : t1;
        o = xh_cd{y.x * inv / t, y.y * inv / t};
    } else {
        const xh_cd q = F[idx];
        if (model == 0) {
            o = xh_cd{q.x * inv, q.y * inv};
            if (win < maxwi) { o.x *= beta00; o.y *= beta00; }
        } else {
            o = xh_cd{q.x * inv * t1, q.y * inv * t1};
            if (c == 0) o = xh_cd{F[2 * plane + idx].x * inv, F[2 * plane + idx].y * inv};
        }
    }
    G[idx] = o;
}

// L801 / L806-810
__global__ void __launch_bounds__(256)
k_sub_out(const xh_cd *__restrict__ G, const double *__restrict__ I2, double *__restrict__ out, int boost, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    out[idx] = boost ? G[idx].x : I2[idx] - G[idx].x;
}

void sub_freq_map(int D, double sampling, double maxResol, int32_t *wi, int32_t *maxwi)
{
    const int xh = D / 2 + 1;
    for (int i = 0; i < D; ++i) {
        const double wy = (double)(i <= (D >> 1) ? i : i - D) / (double)D;          // FFT_IDX2DIGFREQ(i, YSIZE, .)
        for (int j = 0; j < xh; ++j) {
            const double wx = (double)j / (double)D;                                  // YSIZE here too, as written; j <= D / 2
            if (wi) wi[i * xh + j] = (int)std::round(std::sqrt(wy * wy + wx * wx) * D);
        }
    }
    if (maxResol == -1.0) maxResol = sampling;
    const double cut = (sampling / maxResol) / std::sqrt(2.0);
    int idx = (int)std::round((double)D * cut);                                      // DIGFREQ2FFT_IDX
    if (idx < 0) idx += D;
    *maxwi = idx;
}
}  // namespace

struct xh_sub {
    xh_ctx *ctx = nullptr;
    xh_sub_params prm;
    int D = 0, Np = 0, padOff = 0, capacity = 0, maxwi = 0, bins = 0, n = 0, lastCount = 0;
    double a11 = 0;
    bool hasRoi = false, hasMaskVol = false;
    xh_fp *fp = nullptr;
    xh_rsp *rspV = nullptr, *rspRoi = nullptr, *rspMask = nullptr;
    XhFft2d64 fftD, fftP;
    XhBuf d_circle, d_cells, d_binStart, d_wiHalf, d_wiFull;
    XhBuf d_images, d_rows;                                  // the load: [n][D][D] doubles, [n][kRow]
    XhBuf d_Praw, d_P, d_Pc, d_Pmask, d_M, d_iM, d_I2, d_b, d_F, d_Fpad, d_S, d_beta, d_res, d_out;
    std::vector<double> rows;                                // host copy of the rows
    std::vector<double> ang, off;                            // per particle: angles [3], roffset [2]
    std::vector<XhEvent> ev;                                 // kSubStages + 1 events while timing is on
    double stage_ms[kSubStages] = {};                        // of the last timed run, summed over its chunks
    ~xh_sub()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        if (fp) xh_fp_destroy(fp);
        if (rspV) xh_rsp_destroy(rspV);
        if (rspRoi) xh_rsp_destroy(rspRoi);
        if (rspMask) xh_rsp_destroy(rspMask);
    }
};

extern "C" {

void xh_sub_defaults(xh_sub_params *p)
{
    if (!p) return;
    p->sampling = 1; p->max_resolution = -1; p->padding = 2; p->cirmaskrad = -1;
    p->subtract = p->real_space = p->ignore_ctf = p->boost = p->non_negative = 0;
}

int xh_sub_freq_map(int32_t D, double sampling, double max_resolution, int32_t *h_wi, int32_t *maxwiIdx)
{
    XH_CHECK(D >= 1 && maxwiIdx && sampling > 0 && (max_resolution > 0 || max_resolution == -1.0), XH_ERR_ARG, "xh_sub_freq_map: bad argument");
    sub_freq_map(D, sampling, max_resolution, h_wi, maxwiIdx);
    return XH_OK;
}

int xh_sub_fit(const double *h_sums, int32_t maxwiIdx, double a11, double *h_betas)
{
    XH_CHECK(h_sums && h_betas && maxwiIdx >= 0, XH_ERR_ARG, "xh_sub_fit: bad argument");
    sub_fit(h_sums, maxwiIdx, a11, h_betas);
    return XH_OK;
}

int xh_sub_choose(double sumY, double sumY2, double sumE0, double sumE1, double cells, double *h_out)
{
    XH_CHECK(h_out && cells > 1, XH_ERR_ARG, "xh_sub_choose: bad argument");
    sub_choose(sumY, sumY2, sumE0, sumE1, cells, h_out);
    return XH_OK;
}

int xh_sub_create(xh_ctx *ctx, const double *h_vol, int32_t D, const double *h_roi, const double *h_maskvol, const xh_sub_params *prm, int32_t capacity,
                  xh_sub **out)
{
    XH_CHECK(ctx && h_vol && prm && out, XH_ERR_ARG, "xh_sub_create: bad argument");
    XH_CHECK(D >= 4 && D <= 1024, XH_ERR_ARG, "xh_sub_create: size %d outside 4 .. 1024", D);
    XH_CHECK(capacity >= 1 && capacity <= 16384, XH_ERR_ARG, "xh_sub_create: capacity %d outside 1 .. 16384", capacity);
    XH_CHECK(prm->sampling > 0 && (prm->max_resolution > 0 || prm->max_resolution == -1.0), XH_ERR_ARG,
             "xh_sub_create: sampling %g / max_resolution %g", prm->sampling, prm->max_resolution);
    XH_CHECK((int)prm->padding >= 1 && (int)prm->padding * (D - 1) + 1 <= 2048, XH_ERR_ARG, "xh_sub_create: padding %g", prm->padding);
    XH_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<xh_sub> h(new xh_sub);
    h->ctx = ctx; h->prm = *prm; h->D = D; h->capacity = capacity;
    h->hasRoi = h_roi != nullptr; h->hasMaskVol = h_maskvol != nullptr;
    const size_t N3 = (size_t)D * D * D, DD = (size_t)D * D;
    const int xh = D / 2 + 1;
    // createMask (L177-197) and V *= ivM (L597-614)
    std::vector<double> V(h_vol, h_vol + N3);
    if (h_roi)
        for (size_t k = 0; k < N3; ++k) V[k] *= prm->subtract ? h_roi[k] : h_roi[k] * (-1) + 1;
    XhBuf d_tmp;
    const double maxResol = prm->max_resolution == -1.0 ? prm->sampling : prm->max_resolution;
    if (prm->real_space) {
        XH_TRY(xh_buf_upload(ctx, d_tmp, V.data(), sizeof(double) * N3));
        XH_TRY(xh_rsp_create(ctx, (const double *)d_tmp.p, D, XH_RSP_VALUE, &h->rspV));
    } else {
        std::vector<float> Vf(N3);
        for (size_t k = 0; k < N3; ++k) Vf[k] = (float)V[k];
        XH_TRY(xh_buf_upload(ctx, d_tmp, Vf.data(), sizeof(float) * N3));
        XH_TRY(xh_fp_create(ctx, (const float *)d_tmp.p, D, prm->padding, 0.5 * (prm->sampling / maxResol), 3, &h->fp));
    }
    if (h_roi) {
        XH_TRY(xh_buf_upload(ctx, d_tmp, h_roi, sizeof(double) * N3));
        XH_TRY(xh_rsp_create(ctx, (const double *)d_tmp.p, D, XH_RSP_SUPPORT, &h->rspRoi));
    }
    if (h_maskvol) {
        XH_TRY(xh_buf_upload(ctx, d_tmp, h_maskvol, sizeof(double) * N3));
        XH_TRY(xh_rsp_create(ctx, (const double *)d_tmp.p, D, XH_RSP_SUPPORT, &h->rspMask));
    } else {
        // RaisedCosineMask(maskVol, R, R) about the Xmipp origin (L536-542): 1 where r^2 <= R^2
        const double R = prm->cirmaskrad == -1.0 ? (double)D / 2 : prm->cirmaskrad;
        std::vector<double> c(DD);
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                const double y = i - D / 2, x = j - D / 2;
                c[(size_t)i * D + j] = (0.0 + y * y + x * x) <= R * R ? 1.0 : 0.0;
            }
        XH_TRY(xh_buf_upload(ctx, h->d_circle, c.data(), sizeof(double) * DD));
    }
    xh_buf_free(d_tmp);
    // wi, maxwiIdx, the cells grouped by wi
    std::vector<int32_t> wi((size_t)D * xh), wiFull(DD);
    sub_freq_map(D, prm->sampling, prm->max_resolution, wi.data(), &h->maxwi);
    h->bins = h->maxwi + 1;
    std::vector<int32_t> binStart((size_t)h->bins + 1, 0), cells;
    h->a11 = 0;
    for (int w = 0; w < h->bins; ++w) {
        binStart[w] = (int32_t)cells.size();
        if (w > 0 && w < h->maxwi)
            for (int n = 0; n < D * xh; ++n)
                if (wi[n] == w) { cells.push_back((n / xh) * D + n % xh); h->a11 += 2 * w; }
    }
    binStart[h->bins] = (int32_t)cells.size();
    if (cells.empty()) cells.push_back(0);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            int ih = i, jh = j;
            if (jh > D / 2) { jh = D - jh; ih = (D - ih) % D; }
            wiFull[(size_t)i * D + j] = wi[(size_t)ih * xh + jh];
        }
    XH_TRY(xh_buf_upload(ctx, h->d_cells, cells.data(), sizeof(int32_t) * cells.size()));
    XH_TRY(xh_buf_upload(ctx, h->d_binStart, binStart.data(), sizeof(int32_t) * binStart.size()));
    XH_TRY(xh_buf_upload(ctx, h->d_wiHalf, wi.data(), sizeof(int32_t) * wi.size()));
    XH_TRY(xh_buf_upload(ctx, h->d_wiFull, wiFull.data(), sizeof(int32_t) * wiFull.size()));
    // the padded window of applyCTF (L232): from (int)pad STARTING to (int)pad FINISHING
    const int pad = (int)prm->padding, start = -(D / 2), finish = start + D - 1;
    h->Np = pad * finish - pad * start + 1;
    h->padOff = start - pad * start;
    XH_TRY(xh_fft2d64_create(ctx, D, D, h->fftD, "xh_sub_create"));
    XH_TRY(xh_fft2d64_create(ctx, h->Np, h->Np, h->fftP, "xh_sub_create"));
    const size_t cap = capacity;
    for (XhBuf *b : {&h->d_Praw, &h->d_P, &h->d_Pc, &h->d_Pmask, &h->d_M, &h->d_iM, &h->d_I2, &h->d_out}) XH_TRY(xh_buf_alloc(ctx, *b, sizeof(double) * DD * cap));
    XH_TRY(xh_buf_alloc(ctx, h->d_F, sizeof(xh_cd) * DD * cap * 5));
    XH_TRY(xh_buf_alloc(ctx, h->d_Fpad, sizeof(xh_cd) * (size_t)h->Np * h->Np * cap));
    XH_TRY(xh_buf_alloc(ctx, h->d_b, sizeof(double) * cap));
    XH_TRY(xh_buf_alloc(ctx, h->d_S, sizeof(double) * 4 * h->bins * cap));
    XH_TRY(xh_buf_alloc(ctx, h->d_beta, sizeof(double) * 3 * cap));
    XH_TRY(xh_buf_alloc(ctx, h->d_res, sizeof(double) * kRes * cap));
    XH_HIP(hipMemsetAsync(h->d_M.p, 0, h->d_M.bytes, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    *out = h.release();
    return XH_OK;
}

int xh_sub_destroy(xh_sub *h)
{
    delete h;
    return XH_OK;
}

int xh_sub_info(const xh_sub *h, int32_t *maxwiIdx, int32_t *padded, double *a11)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_sub_info: null handle");
    if (maxwiIdx) *maxwiIdx = h->maxwi;
    if (padded) *padded = h->Np;
    if (a11) *a11 = h->a11;
    return XH_OK;
}

int xh_sub_load(xh_sub *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_sub_row *rows)
{
    XH_CHECK(h && h_images && rows && n >= 1, XH_ERR_ARG, "xh_sub_load: bad argument");
    XH_CHECK(ydim == xdim, XH_ERR_UNSUPPORTED, "xh_sub_load: images must be square, got %d x %d", ydim, xdim);
    XH_CHECK(xdim == h->D, XH_ERR_UNSUPPORTED, "xh_sub_load: particles of size %d against a volume of size %d", xdim, h->D);
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    h->n = 0; h->lastCount = 0;
    const size_t DD = (size_t)h->D * h->D;
    h->rows.assign((size_t)kRow * n, 0.0);
    h->ang.resize(3 * (size_t)n);
    h->off.resize(2 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        const xh_sub_row &r = rows[i];
        const double v[5] = {r.rot, r.tilt, r.psi, r.shift_x, r.shift_y};
        for (double q : v) XH_CHECK(std::isfinite(q), XH_ERR_ARG, "xh_sub_load: particle %d has a non-finite pose", i);
        double *q = &h->rows[(size_t)kRow * i];
        xh_fp_euler(r.rot, r.tilt, r.psi, q);
        q[9] = r.shift_x; q[10] = r.shift_y;
        h->ang[3 * (size_t)i] = r.rot; h->ang[3 * (size_t)i + 1] = r.tilt; h->ang[3 * (size_t)i + 2] = r.psi;
        h->off[2 * (size_t)i] = -r.shift_x; h->off[2 * (size_t)i + 1] = -r.shift_y;       // roffset *= -1 (L252)
        if (r.has_ctf && !h->prm.ignore_ctf) {
            const double *c = reinterpret_cast<const double *>(&r.ctf);
            for (size_t k = 0; k < sizeof(xh_ctf_params) / sizeof(double); ++k)
                XH_CHECK(std::isfinite(c[k]), XH_ERR_ARG, "xh_sub_load: particle %d has a non-finite CTF parameter", i);
            xh_ctf_params cc = r.ctf;
            cc.Tm = h->prm.sampling;                                                       // L221
            const CtfSide s = side_info(cc, false);
            q[kRowCtf] = 1.0;
            std::memcpy(q + kRowCtf + 1, &s, sizeof(s));
        }
    }
    XH_TRY(xh_buf_upload(ctx, h->d_rows, h->rows.data(), sizeof(double) * h->rows.size()));
    XH_TRY(xh_buf_alloc(ctx, h->d_images, sizeof(double) * DD * n));
    XhBuf d_f;
    XH_TRY(xh_buf_upload(ctx, d_f, h_images, sizeof(float) * DD * n));
    XH_LAUNCH256(ctx, k_sub_widen, (unsigned)((DD * n + 255) / 256), (const float *)d_f.p, (double *)h->d_images.p, DD * n);
    XH_HIP(hipStreamSynchronize(ctx->stream));
    h->n = n;
    return XH_OK;
}

int xh_sub_run(xh_sub *h, double *h_out, xh_sub_result *h_res)
{
    XH_CHECK(h && h_out && h_res, XH_ERR_ARG, "xh_sub_run: null argument");
    XH_CHECK(h->n > 0, XH_ERR_STATE, "xh_sub_run: no particles loaded");
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const int D = h->D, Np = h->Np;
    const size_t DD = (size_t)D * D, NN = (size_t)Np * Np;
    std::vector<double> res((size_t)kRes * h->capacity);
    const bool timing = !h->ev.empty();
    int stage = 0;
    // an event before each stage of a timed run; they do not synchronise, the chunk still waits once
#define SUB_MARK() do { if (timing) XH_HIP(hipEventRecord(h->ev[stage++], ctx->stream)); } while (0)
    for (double &v : h->stage_ms) v = 0.0;
    for (int p0 = 0; p0 < h->n; p0 += h->capacity) {
        const int m = std::min(h->capacity, h->n - p0);
        const size_t total = DD * m, plane = DD * h->capacity;
        const unsigned g = (unsigned)((total + 255) / 256);
        const double *rows = (const double *)h->d_rows.p + (size_t)kRow * p0;
        const double *ang = &h->ang[3 * (size_t)p0], *off = &h->off[2 * (size_t)p0];
        double *P = (double *)h->d_P.p, *Pc = (double *)h->d_Pc.p;
        stage = 0;
        SUB_MARK();
        // 1. the projection
        if (h->prm.real_space) XH_TRY(xh_rsp_project(h->rspV, ang, off, m, P));
        else {
            XH_TRY(xh_fp_project_f64(h->fp, rows, kRow, m, nullptr, 0, (double *)h->d_Praw.p));
            hipLaunchKernelGGL(k_sub_translate, dim3((unsigned)((m * D + 63) / 64)), dim3(64), 0, ctx->stream, (const double *)h->d_Praw.p, rows, P, D, m);
            XH_LAUNCH_CHECK();
        }
        SUB_MARK();
        // 2. Pctf (applyCTF, L217-240)
        {
            const size_t tp = NN * m;
            const unsigned gp = (unsigned)((tp + 255) / 256);
            xh_cd *Fp = (xh_cd *)h->d_Fpad.p;
            XH_LAUNCH256(ctx, k_sub_pad, gp, (const double *)P, Fp, D, Np, h->padOff, tp);
            XH_TRY(xh_fft2d64(ctx, h->fftP, Fp, m, false));
            XH_LAUNCH256(ctx, xh_k_lowpass_ctf<XH_FACTOR_CTF>, gp, Fp, tp, Np, 10.0, 0.02, rows, kRow, kRowCtf, 1.0 / h->prm.sampling, 0);
            XH_TRY(xh_fft2d64(ctx, h->fftP, Fp, m, true));
            XH_LAUNCH256(ctx, k_sub_crop, g, (const xh_cd *)Fp, (const double *)P, rows, Pc, D, Np, h->padOff, total);
        }
        SUB_MARK();
        // 3. / 4. the masks
        const double *Pmask = (const double *)h->d_circle.p;
        size_t pmStride = 0;
        if (h->hasMaskVol) {
            XH_TRY(xh_rsp_project(h->rspMask, ang, off, m, (double *)h->d_Pmask.p));
            Pmask = (const double *)h->d_Pmask.p;
            pmStride = DD;
        }
        if (h->hasRoi) XH_TRY(xh_rsp_project(h->rspRoi, ang, off, m, (double *)h->d_M.p));
        SUB_MARK();
        // 5. / 6. b, I -= b, the four images; their spectra
        xh_cd *F = (xh_cd *)h->d_F.p;
        hipLaunchKernelGGL(k_sub_prepare, dim3(m), dim3(256), 0, ctx->stream, (const double *)Pc, (const double *)h->d_images.p + DD * p0, Pmask, pmStride,
                           h->hasRoi ? (const double *)h->d_M.p : (const double *)nullptr, h->prm.subtract, (double *)h->d_iM.p, (double *)h->d_I2.p,
                           (double *)h->d_b.p, F, plane, (int)DD);
        XH_LAUNCH_CHECK();
        for (int k = 0; k < 4; ++k) XH_TRY(xh_fft2d64(ctx, h->fftD, F + plane * k, m, false));
        SUB_MARK();
        // 7. / 8. the sums per wi and the fit
        const double inv = 1.0 / (double)DD;
        hipLaunchKernelGGL(k_sub_bins, dim3(h->bins, m), dim3(256), 0, ctx->stream, (const xh_cd *)F, plane, (const int *)h->d_cells.p,
                           (const int *)h->d_binStart.p, (double *)h->d_S.p, h->bins, (int)DD, inv);
        XH_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sub_fit, dim3((m + 63) / 64), dim3(64), 0, ctx->stream, (const double *)h->d_S.p, h->bins, h->maxwi, h->a11, (double *)h->d_beta.p, m);
        XH_LAUNCH_CHECK();
        SUB_MARK();
        // 9. / 10. the models and the choice
        hipLaunchKernelGGL(k_sub_models, dim3(m), dim3(256), 0, ctx->stream, (const xh_cd *)F, plane, (const int *)h->d_wiHalf.p, (const double *)h->d_beta.p,
                           (const double *)h->d_b.p, (double *)h->d_res.p, D, h->maxwi, h->prm.non_negative, inv);
        XH_LAUNCH_CHECK();
        SUB_MARK();
        // 11. the output
        xh_cd *G = F + plane * 4;
        XH_LAUNCH256(ctx, k_sub_spectrum, g, (const xh_cd *)F, plane, (const int *)h->d_wiFull.p, (const double *)h->d_beta.p, (const double *)h->d_res.p, G,
                     (int)DD, h->maxwi, h->prm.boost, inv, total);
        XH_TRY(xh_fft2d64(ctx, h->fftD, G, m, true));
        XH_LAUNCH256(ctx, k_sub_out, g, (const xh_cd *)G, (const double *)h->d_I2.p, (double *)h->d_out.p, h->prm.boost, total);
        SUB_MARK();
        XH_HIP(hipMemcpyAsync(h_out + DD * p0, h->d_out.p, sizeof(double) * total, hipMemcpyDeviceToHost, ctx->stream));
        XH_HIP(hipMemcpyAsync(res.data(), h->d_res.p, sizeof(double) * kRes * m, hipMemcpyDeviceToHost, ctx->stream));
        XH_HIP(hipStreamSynchronize(ctx->stream));
        for (int t = 0; timing && t < kSubStages; ++t) {
            float ms = 0.f;
            XH_HIP(hipEventElapsedTime(&ms, h->ev[t], h->ev[t + 1]));
            h->stage_ms[t] += ms;
        }
        for (int r = 0; r < m; ++r) {
            const double *q = &res[(size_t)kRes * r];
            xh_sub_result &o = h_res[p0 + r];
            o.R2adj = q[0]; o.beta0 = q[1]; o.beta1 = q[2]; o.b = q[3];
            o.model = (int)q[4]; o.disable = (int)q[5];
            o.enabled = (h->prm.non_negative && (o.disable || o.R2adj < 0)) ? -1 : 1;       // writeParticle (L170-173)
            o.beta00 = q[6]; o.R20adj = q[7];
        }
        h->lastCount = m;
    }
#undef SUB_MARK
    return XH_OK;
}

int xh_sub_set_timing(xh_sub *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_sub_set_timing: null handle");
    XH_HIP(hipSetDevice(h->ctx->device));
    if (on && h->ev.empty()) {
        std::vector<XhEvent> ev(kSubStages + 1);
        for (XhEvent &e : ev) XH_TRY(xh_event_create(e));
        h->ev.swap(ev);
    } else if (!on) {
        XH_HIP(hipStreamSynchronize(h->ctx->stream));
        h->ev.clear();
    }
    return XH_OK;
}

int xh_sub_stage_ms(const xh_sub *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_sub_stage_ms: null argument");
    for (int t = 0; t < kSubStages; ++t) h_ms[t] = h->stage_ms[t];
    return XH_OK;
}

int xh_sub_last(xh_sub *h, int32_t index, double *d_P, double *d_Pctf, double *d_PmaskImg, double *d_M, double *d_iM, double *d_Idiff, double *h_sums,
                double *h_betas)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_sub_last: null handle");
    XH_CHECK(index >= 0 && index < h->lastCount, XH_ERR_STATE, "xh_sub_last: particle %d of the %d the last chunk held", index, h->lastCount);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const size_t bytes = sizeof(double) * h->D * h->D;
    const struct { double *dst; const XhBuf *src; bool shared; } planes[] = {
        {d_P, &h->d_P, false}, {d_Pctf, &h->d_Pc, false}, {d_PmaskImg, h->hasMaskVol ? &h->d_Pmask : &h->d_circle, !h->hasMaskVol},
        {d_M, &h->d_M, false}, {d_iM, &h->d_iM, false}, {d_Idiff, &h->d_out, false}};
    for (const auto &q : planes)
        if (q.dst) XH_HIP(hipMemcpyAsync(q.dst, (const char *)q.src->p + (q.shared ? 0 : bytes * index), bytes, hipMemcpyDeviceToDevice, st));
    if (h_sums) XH_HIP(hipMemcpyAsync(h_sums, (const double *)h->d_S.p + (size_t)4 * h->bins * index, sizeof(double) * 4 * h->bins, hipMemcpyDeviceToHost, st));
    if (h_betas) XH_HIP(hipMemcpyAsync(h_betas, (const double *)h->d_beta.p + 3 * (size_t)index, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

}  // extern "C"
