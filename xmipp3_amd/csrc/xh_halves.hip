// xh_halves.hip -- the device side of xmipp_volume_halves_restoration (reconstruction_cuda/cuda_volume_halves_restorator.cpp,
// cuda_volume_restoration_kernels.{cpp,cu}, cuda_cdf.{cpp,cu}; CPU counterpart reconstruction/volume_halves_restoration.cpp), fp64.
//
// The handle holds the two half maps and runs the reference's four stages on them in place: denoising, deconvolution, filter bank,
// difference. 3-D transforms are the r2c / c2r pair of xh_fft3d.h, un-normalised both ways as cuFFT's; where the reference multiplies
// by 1/N right after an inverse (normalizeForFFT) or right before a forward, the factor rides in the transform's row kernel: the same
// single rounding. R2 (squared digital frequency, FFT_IDX2DIGFREQ) is recomputed from the index wherever it is read.
//
// CDF (Gpu::CDF): the reference sorts all N keys to read 200 order statistics (plus the minimum and maximum). Here the 202 ranks are
// selected together by radix select over the keys' IEEE bit patterns (every key is a square, so non-negative, and non-negative doubles
// order as their bits do): an 11-bit pass over the exponent, then 6-bit digits. Each pass histograms, in LDS, the next digit of every
// key whose resolved prefix equals the prefix of some rank (binary search over the <= 202 distinct prefixes), and one workgroup walks
// each rank's histogram row (prefix-summed in LDS, then a binary search) to extend its prefix. 10 passes; the keys are written once by the
// first and read by the other nine. Masked
// out voxels get the key ~0, whose top bit no prefix has, so they never count. The result equals sorting the keys, bit for bit.
//
// Reductions (Powell cost, mean / standard deviation, mask count) are one pass of per-workgroup partial sums and one workgroup that adds
// them in a fixed order: deterministic, one value copied to the host.
//
// Deviations from the reference, each where the reference divides 0 by 0, reads out of bounds or does not terminate:
//  - computeDifference: where the standard deviation is 0 the reference's weight is exp(-inf * 0) = NaN; the weight is 0 there.
//  - computeWeights, weightFun 2: where w1 + w2 = 0 the reference computes 0 / 0 = NaN; the weight is 0 there.
//  - computeWeights, weightFun 3: the GPU reference leaves the weight uninitialised; it is 0, as in the CPU program.
//  - The reference sizes its half spectrum X Y (Z/2 + 1), which is the true Z Y (X/2 + 1) only when Z = X; the true size is used,
//    for the loops and for the Powell cost's 1 / (2 size).
//  - CDF rank round(p N) is clamped to N - 1 (the reference reads past its array when N <= 200).
//  - An empty mask and a filter bank whose step (1 - overlap) is not positive are refused (the reference reads out of bounds / loops
//    forever).
// The reference's power(double, int) truncates weightPower to an integer before pow; so does this file.
#include "xh_volume.h"
#include "xh_reduce.h"
#include <cmath>

namespace {

constexpr int HV_NSTEPS = 200;          // round(1 / probStep), probStep 0.005
constexpr int HV_NR = HV_NSTEPS + 2;    // ranks: 0, the 200 steps, N - 1
constexpr int HV_W0 = 11;               // first digit: bits 62 .. 52
constexpr int HV_W = 6;                 // later digits
constexpr int HV_HIST = HV_NR << HV_W;  // >= 1 << HV_W0

struct CdfDev {
    unsigned long long prefix[HV_NR];
    unsigned long long krem[HV_NR];
    unsigned long long distinct[HV_NR];
    int P;
    unsigned int hist[HV_HIST];
    double prob[HV_NSTEPS];            // p of the reference's loop for (p = step / 2; p < 1; p += step)
    double tab[2][HV_NR];              // [min, x_0 .. x_199, max] of two CDFs
};

// R2 of half-spectrum element e of [Z][Y][xh] (initializeFilter)
__device__ __forceinline__ double hv_r2(size_t e, int Y, int X, int Z, int xh)
{
    const int j = (int)(e % xh);
    const size_t r = e / xh;
    const int i = (int)(r % Y), k = (int)(r / Y);
    const double fz = d_digfreq(k, Z), fy = d_digfreq(i, Y), fx = d_digfreq(j, X);
    return fx * fx + fy * fy + fz * fz;
}

__device__ __forceinline__ double hv_interp(double x, double x0, double y0, double xF, double yF) { return y0 + ((x - x0) * (yF - y0)) / (xF - x0); }

// Gpu::getCDFProbability over a table [min, x_0 .. x_{N-1}, max]. A NaN argument gives NaN (the reference's search never ends there).
__device__ double hv_cdf_prob(double xi, const double *t, const double *prob)
{
    const double minVal = t[0], maxVal = t[HV_NR - 1];
    const double *x = t + 1;
    const int N = HV_NSTEPS;
    if (xi != xi) return xi;
    if (xi > maxVal) return 1;
    if (xi < minVal) return 0;
    if (xi < x[0]) return hv_interp(xi, minVal, 0.0, x[0], prob[0]);
    if (xi > x[N - 1]) return hv_interp(xi, x[N - 1], prob[N - 1], maxVal, 1.0);
    int iLeft = 0, iRight = N - 1;
    while (iLeft <= iRight) {
        const int iMiddle = iLeft + (iRight - iLeft) / 2;
        if (xi >= x[iMiddle] && xi <= x[iMiddle + 1]) {
            if (x[iMiddle] == x[iMiddle + 1]) return 0.5 * (prob[iMiddle] + prob[iMiddle + 1]);
            return hv_interp(xi, x[iMiddle], prob[iMiddle], x[iMiddle + 1], prob[iMiddle + 1]);
        } else if (xi < x[iMiddle]) iRight = iMiddle;
        else iLeft = iMiddle;
    }
    return 0;
}

// one or two CDF tables and the probabilities into LDS
__device__ __forceinline__ void hv_load_tabs(double *s, const CdfDev *cd, int ntab)
{
    for (int i = threadIdx.x; i < HV_NSTEPS; i += blockDim.x) s[i] = cd->prob[i];
    for (int i = threadIdx.x; i < ntab * HV_NR; i += blockDim.x) s[HV_NSTEPS + i] = cd->tab[i / HV_NR][i % HV_NR];
    __syncthreads();
}


// ---------------------------------------------------------------- CDF by radix select
__global__ void __launch_bounds__(256) k_cdf_init(CdfDev *cd, unsigned long long N)
{
    const int r = threadIdx.x;
    if (r < HV_NR) {
        unsigned long long rank;
        if (r == 0) rank = 0;
        else if (r == HV_NR - 1) rank = N - 1;
        else rank = min((unsigned long long)(long long)round(cd->prob[r - 1] * (double)N), N - 1);
        cd->krem[r] = rank;
        cd->prefix[r] = 0;
    }
    if (r == 0) { cd->distinct[0] = 0; cd->P = 1; }
}

// keys (MODE 0: a^2; MODE 1: mult (a - b)^2, as multConst * diff * diff) and the histogram of bits 62 .. 52
template <int MODE>
__global__ void __launch_bounds__(256)
k_cdf_first(const double *__restrict__ a, const double *__restrict__ b, const int *__restrict__ mask, double mult, unsigned long long *__restrict__ keys,
            size_t N, CdfDev *cd)
{
    __shared__ unsigned int h[1 << HV_W0];
    for (int i = threadIdx.x; i < (1 << HV_W0); i += blockDim.x) h[i] = 0;
    __syncthreads();
    XH_GRID_LOOP(n, N) {
        double v;
        if (MODE == 0) v = a[n] * a[n];
        else { const double d = a[n] - b[n]; v = mult * d * d; }
        const unsigned long long k = (mask && mask[n] == 0) ? ~0ull : (unsigned long long)__double_as_longlong(v);
        keys[n] = k;
        if (!(k >> 63)) atomicAdd(&h[(k >> 52) & ((1u << HV_W0) - 1)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (1 << HV_W0); i += blockDim.x)
        if (h[i]) atomicAdd(&cd->hist[i], h[i]);
}

// histogram of the w bits below the b resolved ones, one row per distinct prefix of a rank
__global__ void __launch_bounds__(256)
k_cdf_pass(const unsigned long long *__restrict__ keys, size_t N, int b, int w, CdfDev *cd)
{
    __shared__ unsigned long long pre[HV_NR];
    __shared__ unsigned int h[HV_HIST];
    const int P = cd->P;
    for (int i = threadIdx.x; i < P; i += blockDim.x) pre[i] = cd->distinct[i];
    for (int i = threadIdx.x; i < (P << w); i += blockDim.x) h[i] = 0;
    __syncthreads();
    const unsigned long long lo = pre[0], hi = pre[P - 1];
    const unsigned dmask = (1u << w) - 1;
    XH_GRID_LOOP(n, N) {
        const unsigned long long k = keys[n], top = k >> (64 - b);
        if (top < lo || top > hi) continue;
        int l = 0, r = P - 1;
        while (l < r) {
            const int m = (l + r) >> 1;
            if (pre[m] < top) l = m + 1; else r = m;
        }
        if (pre[l] == top) atomicAdd(&h[(l << w) | (unsigned)((k >> (64 - b - w)) & dmask)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (P << w); i += blockDim.x)
        if (h[i]) atomicAdd(&cd->hist[i], h[i]);
}

// one workgroup: the histogram is prefix-summed in LDS, every rank finds by binary search the digit its remaining rank falls in, the
// distinct prefixes are listed again; the histogram is left zeroed for the next pass
__global__ void __launch_bounds__(256) k_cdf_select(CdfDev *cd, int w)
{
    __shared__ unsigned int sc[HV_HIST];
    __shared__ unsigned int part[256];
    __shared__ unsigned long long dis[HV_NR], npre[HV_NR];
    __shared__ int flag[HV_NR];
    const int t = threadIdx.x, P = cd->P, T = P << w;
    const int chunk = (T + 255) / 256, c0 = min(t * chunk, T), c1 = min(c0 + chunk, T);
    for (int i = t; i < T; i += 256) { sc[i] = cd->hist[i]; cd->hist[i] = 0; }
    if (t < P) dis[t] = cd->distinct[t];
    __syncthreads();
    unsigned int s = 0;
    for (int i = c0; i < c1; ++i) { s += sc[i]; sc[i] = s; }
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned int v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const unsigned int before = t ? part[t - 1] : 0u;
    for (int i = c0; i < c1; ++i) sc[i] += before;             // sc: inclusive prefix sum over all rows
    __syncthreads();
    if (t < HV_NR) {
        const unsigned long long pr = cd->prefix[t];
        int l = 0, r = P - 1;
        while (l < r) {
            const int m = (l + r) >> 1;
            if (dis[m] < pr) l = m + 1; else r = m;
        }
        const int row = l << w;
        const unsigned int base = row ? sc[row - 1] : 0u;
        const unsigned int target = base + (unsigned int)cd->krem[t];
        int a = 0, z = (1 << w) - 1;                           // first digit whose inclusive count exceeds the target
        while (a < z) {
            const int m = (a + z) >> 1;
            if (sc[row + m] > target) z = m; else a = m + 1;
        }
        const unsigned int below = a ? sc[row + a - 1] : base;
        cd->krem[t] = target - below;
        npre[t] = (pr << w) | (unsigned long long)a;
        cd->prefix[t] = npre[t];
    }
    __syncthreads();
    if (t < HV_NR) flag[t] = (t == 0 || npre[t] != npre[t - 1]) ? 1 : 0;
    __syncthreads();
    if (t < HV_NR && flag[t]) {
        int pos = 0;
        for (int q = 1; q <= t; ++q) pos += flag[q];
        cd->distinct[pos] = npre[t];
    }
    if (t == HV_NR - 1) {
        int q = 0;
        for (int i = 0; i < HV_NR; ++i) q += flag[i];
        cd->P = q;
    }
}

__global__ void __launch_bounds__(256) k_cdf_finish(CdfDev *cd, int slot)
{
    const int r = threadIdx.x;
    if (r < HV_NR) cd->tab[slot][r] = __longlong_as_double((long long)cd->prefix[r]);
}

// ---------------------------------------------------------------- per-voxel kernels
__global__ void __launch_bounds__(256)
k_avg_positivity(const double *__restrict__ V1, const double *__restrict__ V2, const int *__restrict__ mask, double *__restrict__ S, size_t N)
{
    XH_GRID_LOOP(n, N) {
        const double val = 0.5 * (V1[n] + V2[n]);
        S[n] = (val <= 0 || (mask && mask[n] == 0)) ? 0.0 : val;
    }
}

__global__ void __launch_bounds__(256) k_filter_s(xh_cd *__restrict__ F, int Z, int Y, int X, int xh)
{
    XH_GRID_LOOP(e, (size_t)Z * Y * xh) {
        if (hv_r2(e, Y, X, Z, xh) > 0.25) F[e] = xh_cd{0.0, 0.0};
    }
}

__global__ void __launch_bounds__(256) k_mask_noise(double *__restrict__ V, const CdfDev *__restrict__ cd, size_t N)
{
    __shared__ double s[HV_NSTEPS + 2 * HV_NR];
    hv_load_tabs(s, cd, 2);
    const double *tS = s + HV_NSTEPS, *tN = s + HV_NSTEPS + HV_NR;
    XH_GRID_LOOP(n, N) {
        const double v = V[n], e = v * v;
        double pN = hv_cdf_prob(e, tN, s);
        if (pN < 1) {
            pN *= hv_cdf_prob(e, tS, s);
            V[n] = pN * v;
        }
    }
}

__global__ void __launch_bounds__(256)
k_deconvolve(xh_cd *__restrict__ fVol, xh_cd *__restrict__ fV1, xh_cd *__restrict__ fV2, double K1, double K2, double lambda, int Z, int Y, int X, int xh)
{
    XH_GRID_LOOP(e, (size_t)Z * Y * xh) {
        const double R2n = hv_r2(e, Y, X, Z, xh);
        if (R2n <= 0.25) {
            double H1 = exp(K1 * R2n), H2 = exp(K2 * R2n);
            xh_cd a = fV1[e], b = fV2[e];
            fVol[e] = xh_cd{(H1 * a.x + H2 * b.x) / (H1 * H1 + H2 * H2 + lambda * R2n), (H1 * a.y + H2 * b.y) / (H1 * H1 + H2 * H2 + lambda * R2n)};
            H1 = 1.0 / H1;
            H2 = 1.0 / H2;
            fV1[e] = xh_cd{a.x * H1, a.y * H1};
            fV2[e] = xh_cd{b.x * H2, b.y * H2};
        }
    }
}

__global__ void __launch_bounds__(256) k_convolve(xh_cd *__restrict__ F, double K, int Z, int Y, int X, int xh)
{
    XH_GRID_LOOP(e, (size_t)Z * Y * xh) {
        const double R2n = hv_r2(e, Y, X, Z, xh);
        if (R2n <= 0.25) {
            const double g = exp(K * R2n);
            F[e] = xh_cd{F[e].x * g, F[e].y * g};
        }
    }
}

__global__ void __launch_bounds__(256)
k_band(const xh_cd *__restrict__ fV, xh_cd *__restrict__ out, double w2, double w2Step, int Z, int Y, int X, int xh)
{
    XH_GRID_LOOP(e, (size_t)Z * Y * xh) {
        const double R2n = hv_r2(e, Y, X, Z, xh);
        out[e] = (R2n >= w2 && R2n < w2Step) ? fV[e] : xh_cd{0.0, 0.0};
    }
}

__global__ void __launch_bounds__(256)
k_weights(const double *__restrict__ Vf1, const double *__restrict__ Vf2, double *__restrict__ V1r, double *__restrict__ V2r, double *__restrict__ S,
          const CdfDev *__restrict__ cd, double weightPower, int weightFun, size_t N)
{
    __shared__ double s[HV_NSTEPS + HV_NR];
    hv_load_tabs(s, cd, 1);
    const double *t = s + HV_NSTEPS;
    const double ipow = (double)(int)weightPower;     // power(double, int)
    XH_GRID_LOOP(n, N) {
        const double f1 = Vf1[n], e1 = f1 * f1, w1 = hv_cdf_prob(e1, t, s);
        const double f2 = Vf2[n], e2 = f2 * f2, w2 = hv_cdf_prob(e2, t, s);
        double weight = 0;
        switch (weightFun) {
            case 0: weight = 0.5 * (w1 + w2); break;
            case 1: weight = fmin(w1, w2); break;
            case 2: weight = (w1 + w2 == 0) ? 0.0 : 0.5 * (w1 + w2) * (1 - fabs(w1 - w2) / (w1 + w2)); break;
            default: break;
        }
        weight = pow(weight, ipow);
        const double Vf1w = f1 * weight, Vf2w = f2 * weight;
        V1r[n] += Vf1w;
        V2r[n] += Vf2w;
        S[n] += e1 > e2 ? Vf1w : Vf2w;
    }
}

__global__ void __launch_bounds__(256) k_scale3(double *__restrict__ a, double *__restrict__ b, double *__restrict__ c, double f, size_t N)
{
    XH_GRID_LOOP(n, N) { a[n] = a[n] * f; b[n] = b[n] * f; c[n] = c[n] * f; }
}

__global__ void __launch_bounds__(256)
k_difference(double *__restrict__ V1, double *__restrict__ V2, const double *__restrict__ S, const double *__restrict__ D, double k, size_t N)
{
    XH_GRID_LOOP(n, N) {
        const double Nn = D[n];
        const double w = (isinf(k) && Nn == 0) ? 0.0 : exp(k * Nn * Nn);
        const double s = S[n];
        V1[n] = s + (V1[n] - s) * w;
        V2[n] = s + (V2[n] - s) * w;
    }
}

// ---------------------------------------------------------------- reductions (xh_reduce.h): partials [NC][gridDim.x], then one workgroup
// restorationSigmaCostError
__global__ void __launch_bounds__(256)
k_sigma_cost(const xh_cd *__restrict__ fVol, const xh_cd *__restrict__ fV1, const xh_cd *__restrict__ fV2, double K1, double K2, double inv_size,
             int Z, int Y, int X, int xh, double *__restrict__ partials)
{
    double acc[1] = {0.0};
    XH_GRID_LOOP(e, (size_t)Z * Y * xh) {
        const double R2n = hv_r2(e, Y, X, Z, xh);
        if (R2n <= 0.25) {
            const double H1 = exp(K1 * R2n), H2 = exp(K2 * R2n);
            const xh_cd f = fVol[e], a = fV1[e], b = fV2[e];
            const double d1x = (f.x * H1 - a.x) * inv_size, d1y = (f.y * H1 - a.y) * inv_size;
            const double d2x = (f.x * H2 - b.x) * inv_size, d2y = (f.y * H2 - b.y) * inv_size;
            acc[0] += sqrt(d1x * d1x + d1y * d1y) + sqrt(d2x * d2x + d2y * d2y);
        }
    }
    xh_block_partials(acc, partials);
}

// computeDiffAndAverage, with the sums of D and D^2 (over the mask, if any) of computeAvgStd[WithMask] riding along
__global__ void __launch_bounds__(256)
k_diff_avg(const double *__restrict__ V1, const double *__restrict__ V2, double *__restrict__ S, double *__restrict__ D, const int *__restrict__ mask,
           size_t N, double *__restrict__ partials)
{
    double acc[2] = {0.0, 0.0};
    XH_GRID_LOOP(n, N) {
        const double a = V1[n], b = V2[n], d = a - b;
        D[n] = d;
        S[n] = (a + b) * 0.5;
        if (!mask || mask[n]) { acc[0] += d; acc[1] += d * d; }
    }
    if (partials) xh_block_partials(acc, partials);
}

__global__ void __launch_bounds__(256) k_mask_count(const int *__restrict__ mask, size_t N, double *__restrict__ partials)
{
    double acc[1] = {0.0};
    XH_GRID_LOOP(n, N) acc[0] += mask[n] != 0 ? 1.0 : 0.0;
    xh_block_partials(acc, partials);
}

}  // namespace

// ---------------------------------------------------------------- the handle
enum { HV_OUT_RESTORED1 = 0, HV_OUT_RESTORED2, HV_OUT_FILTERBANK, HV_OUT_DECONVOLVED, HV_OUT_CONVOLVED, HV_OUT_AVGDIFF, HV_NOUT };

struct xh_halves : XhVolume {
    unsigned grid = 0;                       // per-voxel kernels and reductions
    unsigned gridPass = 0;                   // CDF histogram passes (53 KB of LDS each)
    XhBuf V1, V2, S, B2, B3, keys, C1, C2, C3, cdf, partials, result;
    XhBuf out[4];                            // filter bank, deconvolved, convolved, average difference
    bool loaded = false, has[HV_NOUT] = {};
    bool timing = false;
    XhEvent ev[4];
    double band_ms[3] = {0, 0, 0};
    int bands = 0;
    int costRc = XH_OK;
    ~xh_halves() { finish(); }
};

namespace {

CdfDev *cdfp(xh_halves *h) { return (CdfDev *)h->cdf.p; }

// sum of NC partial rows -> NC doubles on the host (synchronous)
int hv_sums(xh_halves *h, int NC, double *out) { return xh_reduce_finish(h->ctx, dp(h->partials), (int)h->grid, NC, dp(h->result), out); }

int hv_mask_count(xh_halves *h, const int *d_mask, size_t *count)
{
    XH_LAUNCH256(h->ctx, k_mask_count, h->grid, d_mask, h->N, dp(h->partials));
    double c = 0;
    XH_TRY(hv_sums(h, 1, &c));
    *count = (size_t)c;
    XH_CHECK(*count > 0, XH_ERR_ARG, "xh_halves: the mask is empty");
    return XH_OK;
}

// Gpu::CDF::calculateCDF into table `slot`: keys a^2 (b null) or mult (a - b)^2 over the voxels of the mask (null: all), n of them
int hv_cdf(xh_halves *h, const double *a, const double *b, const int *mask, double mult, size_t n, int slot)
{
    CdfDev *cd = cdfp(h);
    XH_LAUNCH256(h->ctx, k_cdf_init, 1, cd, (unsigned long long)n);
    unsigned long long *keys = (unsigned long long *)h->keys.p;
    if (b) XH_LAUNCH256(h->ctx, k_cdf_first<1>, h->grid, a, b, mask, mult, keys, h->N, cd);
    else XH_LAUNCH256(h->ctx, k_cdf_first<0>, h->grid, a, b, mask, mult, keys, h->N, cd);
    XH_LAUNCH256(h->ctx, k_cdf_select, 1, cd, HV_W0);
    for (int bits = 1 + HV_W0; bits < 64;) {
        const int w = std::min(HV_W, 64 - bits);
        XH_LAUNCH256(h->ctx, k_cdf_pass, h->gridPass, (const unsigned long long *)keys, h->N, bits, w, cd);
        XH_LAUNCH256(h->ctx, k_cdf_select, 1, cd, w);
        bits += w;
    }
    XH_LAUNCH256(h->ctx, k_cdf_finish, 1, cd, slot);
    return XH_OK;
}

// estimateS + normalizeForFFT: S = ifft(filterS(fft(averagePositivity(V1, V2)))) / N
int hv_estimate_s(xh_halves *h, const int *mask)
{
    XH_LAUNCH256(h->ctx, k_avg_positivity, h->grid, dp(h->V1), dp(h->V2), mask, dp(h->S), h->N);
    XH_TRY(h->fft.r2c(dp(h->S), cp(h->C1)));
    XH_LAUNCH256(h->ctx, k_filter_s, h->grid, cp(h->C1), h->fft.Z, h->fft.Y, h->fft.X, h->fft.xh);
    return h->fft.c2r(cp(h->C1), dp(h->S), 1.0 / (double)h->N);
}

double hv_sigma_cost_cb(double *x, void *prm)
{
    xh_halves *h = (xh_halves *)prm;
    const double sigma1 = x[1], sigma2 = x[2];
    if (sigma1 < 0 || sigma2 < 0 || sigma1 > 2 || sigma2 > 2) return 1e38;
    double err = 0;
    if (h->costRc == XH_OK) h->costRc = xh_halves_sigma_cost(h, sigma1, sigma2, &err);
    return h->costRc == XH_OK ? err : 1e38;
}

}  // namespace

extern "C" {

int xh_halves_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, xh_halves **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_halves_create: null argument");
    XH_CHECK(Z >= 1 && Y >= 1 && X >= 2, XH_ERR_ARG, "xh_halves_create: bad size %d x %d x %d", Z, Y, X);
    XH_CHECK(Z <= 1024 && Y <= 1024 && X <= 1024, XH_ERR_UNSUPPORTED, "xh_halves_create: sizes above 1024 are not supported (%d x %d x %d)", Z, Y, X);
    std::unique_ptr<xh_halves> h(new xh_halves);
    XH_TRY(h->init(ctx, Z, Y, X));
    h->grid = xh_grid256(h->NF, ctx->num_cus, 4);
    h->gridPass = xh_grid256(h->N, ctx->num_cus, 2);
    const size_t vb = sizeof(double) * h->N, fb = sizeof(xh_cd) * h->NF;
    for (XhBuf *b : {&h->V1, &h->V2, &h->S, &h->B2, &h->B3, &h->keys, &h->out[0], &h->out[1], &h->out[2], &h->out[3]}) XH_TRY(xh_buf_alloc(ctx, *b, vb));
    for (XhBuf *b : {&h->C1, &h->C2, &h->C3}) XH_TRY(xh_buf_alloc(ctx, *b, fb));
    XH_TRY(xh_buf_alloc(ctx, h->cdf, sizeof(CdfDev)));
    XH_TRY(xh_buf_alloc(ctx, h->partials, sizeof(double) * 2 * h->grid));
    XH_TRY(xh_buf_alloc(ctx, h->result, sizeof(double) * 2));
    std::vector<double> prob;
    for (double p = 0.005 / 2; p < 1; p += 0.005) prob.push_back(p);     // CDF<double>::_updateProbabilities
    XH_CHECK(prob.size() == HV_NSTEPS, XH_ERR_STATE, "xh_halves_create: %zu CDF steps", prob.size());
    hipError_t e = hipMemset(h->cdf.p, 0, sizeof(CdfDev));
    if (e == hipSuccess) e = hipMemcpy((char *)h->cdf.p + offsetof(CdfDev, prob), prob.data(), sizeof(double) * HV_NSTEPS, hipMemcpyHostToDevice);
    XH_CHECK(e == hipSuccess, XH_ERR_HIP, "xh_halves_create: %s", hipGetErrorString(e));
    for (XhEvent &x : h->ev) XH_TRY(xh_event_create(x));
    *out = h.release();
    return XH_OK;
}

int xh_halves_destroy(xh_halves *h)
{
    delete h;
    return XH_OK;
}

int xh_halves_load(xh_halves *h, const double *d_v1, const double *d_v2)
{
    XH_CHECK(h && d_v1 && d_v2, XH_ERR_ARG, "xh_halves_load: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(h->V1.p, d_v1, h->V1.bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
    XH_HIP(hipMemcpyAsync(h->V2.p, d_v2, h->V2.bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
    h->loaded = true;
    for (bool &b : h->has) b = false;
    h->has[HV_OUT_RESTORED1] = h->has[HV_OUT_RESTORED2] = true;
    return XH_OK;
}

int xh_halves_denoise(xh_halves *h, int32_t iters, const int32_t *d_mask)
{
    XH_CHECK(h && iters >= 0, XH_ERR_ARG, "xh_halves_denoise: bad argument");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_halves_denoise: no volumes loaded");
    if (iters == 0) return XH_OK;
    XH_HIP(hipSetDevice(h->ctx->device));
    size_t nS = h->N;
    if (d_mask) XH_TRY(hv_mask_count(h, d_mask, &nS));
    for (int it = 0; it < iters; ++it) {
        XH_TRY(hv_estimate_s(h, d_mask));
        XH_TRY(hv_cdf(h, dp(h->S), nullptr, d_mask, 1.0, nS, 0));
        for (XhBuf *V : {&h->V1, &h->V2}) {
            XH_TRY(hv_cdf(h, dp(*V), dp(h->S), nullptr, 1.0, h->N, 1));
            XH_LAUNCH256(h->ctx, k_mask_noise, h->grid, dp(*V), (const CdfDev *)h->cdf.p, h->N);
        }
    }
    return XH_OK;
}

int xh_halves_deconv_spectra(xh_halves *h)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_halves_deconv_spectra: null handle");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_halves_deconv_spectra: no volumes loaded");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_TRY(hv_estimate_s(h, nullptr));
    XH_TRY(h->fft.r2c(dp(h->S), cp(h->C1)));
    XH_TRY(h->fft.r2c(dp(h->V1), cp(h->C2)));
    return h->fft.r2c(dp(h->V2), cp(h->C3));
}

int xh_halves_sigma_cost(xh_halves *h, double sigma1, double sigma2, double *h_cost)
{
    XH_CHECK(h && h_cost, XH_ERR_ARG, "xh_halves_sigma_cost: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    const double K1 = -0.5 / (sigma1 * sigma1), K2 = -0.5 / (sigma2 * sigma2);
    const double inv_size = 1.0 / (2 * (double)h->NF);
    XH_LAUNCH256(h->ctx, k_sigma_cost, h->grid, (const xh_cd *)h->C1.p, (const xh_cd *)h->C2.p, (const xh_cd *)h->C3.p, K1, K2, inv_size, h->fft.Z, h->fft.Y, h->fft.X, h->fft.xh,
              dp(h->partials));
    return hv_sums(h, 1, h_cost);
}

int xh_halves_deconvolve(xh_halves *h, int32_t iters, double sigma0, double lambda, double *h_sigmas)
{
    XH_CHECK(h && iters >= 0, XH_ERR_ARG, "xh_halves_deconvolve: bad argument");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_halves_deconvolve: no volumes loaded");
    if (iters == 0) return XH_OK;
    XH_HIP(hipSetDevice(h->ctx->device));
    const double inv = 1.0 / (double)h->N;
    double sigmaConv1 = sigma0, sigmaConv2 = sigma0;
    for (int it = 0; it < iters; ++it) {
        XH_TRY(xh_halves_deconv_spectra(h));
        double p[2] = {sigmaConv1, sigmaConv2}, cost;
        const double steps[2] = {1.0, 1.0};
        int32_t iter;
        h->costRc = XH_OK;
        XH_TRY(xh_powell_minimize(2, p, steps, 0.01, hv_sigma_cost_cb, h, &cost, &iter));
        XH_TRY(h->costRc);
        sigmaConv1 = p[0]; sigmaConv2 = p[1];
        if (h_sigmas) { h_sigmas[2 * it] = sigmaConv1; h_sigmas[2 * it + 1] = sigmaConv2; }
        const double K1 = -0.5 / (sigmaConv1 * sigmaConv1), K2 = -0.5 / (sigmaConv2 * sigmaConv2);
        XH_LAUNCH256(h->ctx, k_deconvolve, h->grid, cp(h->C1), cp(h->C2), cp(h->C3), K1, K2, lambda, h->fft.Z, h->fft.Y, h->fft.X, h->fft.xh);
        XH_TRY(h->fft.c2r(cp(h->C2), dp(h->V1), inv));
        XH_TRY(h->fft.c2r(cp(h->C3), dp(h->V2), inv));
    }
    XH_HIP(hipMemcpyAsync(h->out[HV_OUT_DECONVOLVED - 2].p, h->S.p, h->S.bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
    const double sigmaConv = (sigmaConv1 + sigmaConv2) / 2;
    XH_LAUNCH256(h->ctx, k_convolve, h->grid, cp(h->C1), -0.5 / (sigmaConv * sigmaConv), h->fft.Z, h->fft.Y, h->fft.X, h->fft.xh);
    XH_TRY(h->fft.c2r(cp(h->C1), dp(h->out[HV_OUT_CONVOLVED - 2]), inv));
    h->has[HV_OUT_DECONVOLVED] = h->has[HV_OUT_CONVOLVED] = true;
    return XH_OK;
}

int xh_halves_filter_bank(xh_halves *h, double step, double overlap, int32_t weightFun, double weightPower)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_halves_filter_bank: null handle");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_halves_filter_bank: no volumes loaded");
    XH_CHECK(weightFun >= 0 && weightFun <= 3, XH_ERR_ARG, "xh_halves_filter_bank: weightFun %d (0 .. 3)", weightFun);
    if (step == 0) return XH_OK;
    const double filterStep = step * (1 - overlap);
    XH_CHECK(filterStep > 0, XH_ERR_ARG, "xh_halves_filter_bank: step (1 - overlap) = %g is not positive", filterStep);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const double inv = 1.0 / (double)h->N;
    XH_TRY(h->fft.r2c(dp(h->V1), cp(h->C1), inv));
    XH_TRY(h->fft.r2c(dp(h->V2), cp(h->C2), inv));
    double *S = dp(h->out[HV_OUT_FILTERBANK - 2]);
    XH_HIP(hipMemsetAsync(h->V1.p, 0, h->V1.bytes, st));
    XH_HIP(hipMemsetAsync(h->V2.p, 0, h->V2.bytes, st));
    XH_HIP(hipMemsetAsync(S, 0, h->V1.bytes, st));
    h->bands = 0;
    for (double &t : h->band_ms) t = 0;
    for (double w = 0; w < 0.5; w += filterStep) {
        const double w2 = w * w, w2Step = (w + step) * (w + step);
        if (h->timing) XH_HIP(hipEventRecord(h->ev[0], st));
        XH_LAUNCH256(h->ctx, k_band, h->grid, (const xh_cd *)h->C1.p, cp(h->C3), w2, w2Step, h->fft.Z, h->fft.Y, h->fft.X, h->fft.xh);
        XH_TRY(h->fft.c2r(cp(h->C3), dp(h->B2), 1.0));
        XH_LAUNCH256(h->ctx, k_band, h->grid, (const xh_cd *)h->C2.p, cp(h->C3), w2, w2Step, h->fft.Z, h->fft.Y, h->fft.X, h->fft.xh);
        XH_TRY(h->fft.c2r(cp(h->C3), dp(h->B3), 1.0));
        if (h->timing) XH_HIP(hipEventRecord(h->ev[1], st));
        XH_TRY(hv_cdf(h, dp(h->B2), dp(h->B3), nullptr, 0.5, h->N, 0));
        if (h->timing) XH_HIP(hipEventRecord(h->ev[2], st));
        XH_LAUNCH256(h->ctx, k_weights, h->grid, dp(h->B2), dp(h->B3), dp(h->V1), dp(h->V2), S, (const CdfDev *)h->cdf.p, weightPower, (int)weightFun, h->N);
        if (h->timing) {
            XH_HIP(hipEventRecord(h->ev[3], st));
            XH_HIP(hipEventSynchronize(h->ev[3]));
            for (int i = 0; i < 3; ++i) {
                float ms = 0;
                XH_HIP(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
                h->band_ms[i] += ms;
            }
        }
        ++h->bands;
    }
    XH_LAUNCH256(h->ctx, k_scale3, h->grid, S, dp(h->V1), dp(h->V2), 1 - overlap, h->N);
    h->has[HV_OUT_FILTERBANK] = true;
    return XH_OK;
}

int xh_halves_difference(xh_halves *h, int32_t iters, double K, const int32_t *d_mask)
{
    XH_CHECK(h && iters >= 0, XH_ERR_ARG, "xh_halves_difference: bad argument");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_halves_difference: no volumes loaded");
    if (iters == 0) return XH_OK;
    XH_HIP(hipSetDevice(h->ctx->device));
    size_t size = h->N;
    if (d_mask) XH_TRY(hv_mask_count(h, d_mask, &size));
    for (int it = 0; it < iters; ++it) {
        XH_LAUNCH256(h->ctx, k_diff_avg, h->grid, dp(h->V1), dp(h->V2), dp(h->S), dp(h->B2), d_mask, h->N, dp(h->partials));
        double sums[2];
        XH_TRY(hv_sums(h, 2, sums));
        // normAvgStd
        double avg = sums[0] / size, std = sums[1];
        if (size > 1) {
            std = std / size - avg * avg;
            std *= (double)size / (size - 1);
            std = sqrt(fabs(std));
        } else std = 0;
        std *= K;
        XH_LAUNCH256(h->ctx, k_difference, h->grid, dp(h->V1), dp(h->V2), dp(h->S), dp(h->B2), -0.5 / (std * std), h->N);
    }
    XH_LAUNCH256(h->ctx, k_diff_avg, h->grid, dp(h->V1), dp(h->V2), dp(h->out[HV_OUT_AVGDIFF - 2]), dp(h->B2), nullptr, h->N, nullptr);
    h->has[HV_OUT_AVGDIFF] = true;
    return XH_OK;
}

int xh_halves_output(xh_halves *h, int32_t which, double *d_out, int32_t *present)
{
    XH_CHECK(h && present && which >= 0 && which < HV_NOUT, XH_ERR_ARG, "xh_halves_output: bad argument");
    *present = h->has[which] ? 1 : 0;
    if (!h->has[which] || !d_out) return XH_OK;
    XH_HIP(hipSetDevice(h->ctx->device));
    const void *src = which == HV_OUT_RESTORED1 ? h->V1.p : which == HV_OUT_RESTORED2 ? h->V2.p : h->out[which - 2].p;
    XH_HIP(hipMemcpyAsync(d_out, src, h->V1.bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
    return XH_OK;
}

int xh_halves_fft_r2c(xh_halves *h, const double *d_in, void *d_out)
{
    XH_CHECK(h && d_in && d_out, XH_ERR_ARG, "xh_halves_fft_r2c: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    return h->fft.r2c(d_in, (xh_cd *)d_out);
}

int xh_halves_fft_c2r(xh_halves *h, const void *d_in, double *d_out, double scale)
{
    XH_CHECK(h && d_in && d_out, XH_ERR_ARG, "xh_halves_fft_c2r: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(h->C3.p, d_in, h->C3.bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
    return h->fft.c2r(cp(h->C3), d_out, scale);
}

int xh_halves_cdf(xh_halves *h, const double *d_a, const double *d_b, const int32_t *d_mask, double mult, double *h_table)
{
    XH_CHECK(h && d_a && h_table, XH_ERR_ARG, "xh_halves_cdf: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    size_t n = h->N;
    if (d_mask) XH_TRY(hv_mask_count(h, d_mask, &n));
    XH_TRY(hv_cdf(h, d_a, d_b, d_mask, mult, n, 0));
    XH_HIP(hipMemcpyAsync(h_table, (char *)h->cdf.p + offsetof(CdfDev, tab), sizeof(double) * HV_NR, hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

int xh_halves_set_timing(xh_halves *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_halves_set_timing: null handle");
    h->timing = on != 0;
    return XH_OK;
}

int xh_halves_band_timing(xh_halves *h, int32_t *bands, double *h_ms)
{
    XH_CHECK(h && bands && h_ms, XH_ERR_ARG, "xh_halves_band_timing: null argument");
    *bands = h->bands;
    for (int i = 0; i < 3; ++i) h_ms[i] = h->band_ms[i];
    return XH_OK;
}

int xh_halves_circular_mask(int32_t Z, int32_t Y, int32_t X, double R1, double x0, double y0, double z0, int32_t *h_mask)
{
    XH_CHECK(Z >= 1 && Y >= 1 && X >= 1 && h_mask, XH_ERR_ARG, "xh_halves_circular_mask: bad argument");
    // BinaryCircularMask (data/mask.cpp) with Mask::readParams' mode: R1 < 0 INNER_MASK with |R1|, R1 > 0 OUTSIDE_MASK
    const bool inner = R1 < 0;
    const double radius = std::fabs(R1), radius2 = radius * radius;
    for (int kk = 0; kk < Z; ++kk) {
        double diff = (double)(kk - Z / 2) - z0;
        const double z2 = diff * diff;
        for (int ii = 0; ii < Y; ++ii) {
            diff = (double)(ii - Y / 2) - y0;
            const double z2y2 = z2 + diff * diff;
            for (int jj = 0; jj < X; ++jj) {
                diff = (double)(jj - X / 2) - x0;
                const double r2 = z2y2 + diff * diff;
                h_mask[((size_t)kk * Y + ii) * X + jj] = ((inner && r2 <= radius2) || (!inner && r2 >= radius2)) ? 1 : 0;
            }
        }
    }
    return XH_OK;
}

int xh_halves_binary_mask(const float *h_values, size_t n, int32_t *h_mask)
{
    XH_CHECK(h_values && h_mask, XH_ERR_ARG, "xh_halves_binary_mask: null argument");
    for (size_t i = 0; i < n; ++i) h_mask[i] = (int32_t)h_values[i] != 0 ? 1 : 0;   // getImage(imask): truncated to int
    return XH_OK;
}

int xh_halves_cylinder_mask(int32_t Z, int32_t Y, int32_t X, double R, double H, double x0, double y0, double z0, int32_t *h_mask)
{
    XH_CHECK(Z >= 1 && Y >= 1 && X >= 1 && h_mask, XH_ERR_ARG, "xh_halves_cylinder_mask: bad argument");
    // BinaryCylinderMask (data/mask.cpp:471-486) with Mask::readParams' mode (:1396-1405)
    XH_CHECK((R < 0 && H < 0) || (R > 0 && H > 0), XH_ERR_ARG, "xh_halves_cylinder_mask: cannot determine mode for cylinder (R %g, H %g)", R, H);
    const bool inner = R < 0;
    const double R2 = std::fabs(R) * std::fabs(R), H_2 = std::fabs(H) / 2;
    for (int kk = 0; kk < Z; ++kk)
        for (int ii = 0; ii < Y; ++ii)
            for (int jj = 0; jj < X; ++jj) {
                const double k = kk - Z / 2, i = ii - Y / 2, j = jj - X / 2;
                const double r2 = (i - y0) * (i - y0) + (j - x0) * (j - x0);
                const bool in = r2 <= R2 && std::fabs(k - z0) <= H_2;
                h_mask[((size_t)kk * Y + ii) * X + jj] = in == inner ? 1 : 0;
            }
    return XH_OK;
}

int xh_halves_tube_mask(int32_t Z, int32_t Y, int32_t X, double R1, double R2, double H, double x0, double y0, double z0, int32_t *h_mask)
{
    XH_CHECK(Z >= 1 && Y >= 1 && X >= 1 && h_mask, XH_ERR_ARG, "xh_halves_tube_mask: bad argument");
    // BinaryTubeMask (data/mask.cpp:261-276) with Mask::readParams' mode (:1419-1429); z0 is not used there, and H is not halved
    XH_CHECK((R1 < 0 && R2 < 0 && H < 0) || (R1 > 0 && R2 > 0 && H > 0), XH_ERR_ARG, "xh_halves_tube_mask: cannot determine mode for tube (R1 %g, R2 %g, H %g)", R1, R2, H);
    (void)z0;
    const bool inner = R1 < 0;
    const double R12 = std::fabs(R1) * std::fabs(R1), R22 = std::fabs(R2) * std::fabs(R2), Ha = std::fabs(H);
    for (int kk = 0; kk < Z; ++kk)
        for (int ii = 0; ii < Y; ++ii)
            for (int jj = 0; jj < X; ++jj) {
                const double k = kk - Z / 2, i = ii - Y / 2, j = jj - X / 2;
                const double r2 = (i - y0) * (i - y0) + (j - x0) * (j - x0);
                const bool in = r2 >= R12 && r2 <= R22 && std::fabs(k) < Ha;
                h_mask[((size_t)kk * Y + ii) * X + jj] = in == inner ? 1 : 0;
            }
    return XH_OK;
}

}  // extern "C"
