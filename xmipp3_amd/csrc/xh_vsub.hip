// xh_vsub.hip -- the device side of xmipp_volume_subtraction (reconstruction/volume_subtraction.{h,cpp}, ProgVolumeSubtraction; the
// reference has no GPU version), fp64: a volume V is adjusted to a reference V1 by projections onto convex sets, and V1 minus the
// adjusted V is formed inside a mask.
//
// The handle owns the plans and every buffer of a Z x Y x X volume. The volume and its spectrum stay on the device over all iterations;
// the host reads two sums per iteration (the moments behind stddev(V)) and nothing else.
//   set_reference  V1 *= mask, V1 = max(0, V1) (run :425-426), min, max and stddev of that (:427, :432), V1FourierMag (:435) and, for
//                  --radavg, V1's radial mean (:264). Done once for any number of volumes adjusted to it.
//   adjust         V *= mask, V = max(0, V) (:430-431), the phase of its transform as (cos phi, sin phi) (:434), the quotient table
//                  (:437) with --radavg, then `iter` times runIteration (:362-418):
//                    r2c (1 / N on load, times the pending scale) | amplitude | c2r | clip and mask, one kernel |
//                    r2c | phase | c2r | max(0, .) with the sum and the sum of squares, one kernel |
//                    with --cutFreq: r2c | raised-cosine low pass | c2r.
//                  std1 / std2 of :403 is never a pass of its own: it rides in the scale of the next r2c (the filter's, or the next
//                  iteration's) and reaches memory once, with the copy to the output.
//   subtract       V1 (1 - m) + (V1F - min(V, V1F)) m (:298-304), V1F being V1 through the same low pass when cutFreq != 0.
// The radial mean (radialAverage :223-257) sums the octant k < Z/2, i < Y/2, j < X/2 only, into the bin round(w X): along a row the bin
// never decreases and never skips a value, so a row is a sequence of runs. The thread at the head of a run adds it up and writes it to the
// row's slot (bin - first bin of the row); one workgroup per bin then adds the rows in row order with the fixed tree (xh_reduce.h). No
// atomics: two runs give the same bytes. The counts depend on the box alone and are formed on the host.
// The energies of --computeEnergy (computeEnergy :205-211 forms each and throws it away) come from extra kernels that only read: with
// them or without, the output has the same bytes.
//
// Reference behaviours kept as written:
//  - the average's bin is a round (:250), the amplitude step's a floor (:172), clamped to the last bin;
//  - FFT_IDX2DIGFREQ_FAST in those two (the index times 1 / size), the division of FFT_IDX2DIGFREQ in the filters (fourier_filter.cpp);
//  - mod > 1e-10 on the normalised modulus (:142); a zero coefficient has phase (1, 0) (atan2(0, 0) = 0);
//  - the quotient is min(q, 1) and then NaN -> 0 (:270-272), so a NaN survives the min and becomes 0, +inf becomes 1.
// Not computed: without --radavg the reference still forms the quotient it never uses.
// Refused, each where the reference writes past an array or divides by zero:
//  - --radavg on a box whose largest octant bin round(w X) reaches the number of bins (radial_mean is written past its end);
//  - stddev(V) == 0 after a phase step (:403), and a reference whose masked, clipped volume is constant;
//  - lambda outside [0, 1], cutFreq outside [0, 0.5], a negative iteration count or sigma.
#include "xh_volume.h"
#include "xh_reduce.h"
#include <cmath>
#include <cstring>

namespace {

constexpr double VS_PI = 3.14159265358979323846;
constexpr double VS_RAISED_W = 0.02;   // createFilter :280
enum { VS_T_TRANSFORMS = 0, VS_T_SPECTRUM, VS_T_REAL, VS_T_FILTER, VS_NT };
enum { VS_E_AMP_CLIP_MASK = 0, VS_E_PHASE_NONNEG, VS_E_SCALE, VS_E_FILTER };

// FFT_IDX2DIGFREQ_FAST (xmippCore xmipp_fft.h): the index, or the index minus the size, times 1 / size
__host__ __device__ __forceinline__ double vs_freq_fast(int idx, int size)
{
    const double isize = 1.0 / size;
    return (idx <= size / 2 ? idx : idx - size) * isize;
}

__host__ __device__ __forceinline__ double vs_w_fast(int k, int i, int j, int Z, int Y, int X)
{
    const double wz = vs_freq_fast(k, Z), wy = vs_freq_fast(i, Y), wx = vs_freq_fast(j, X);
    const double wz2 = wz * wz;
    const double wy2_wz2 = wy * wy + wz2;
    return sqrt(wx * wx + wy2_wz2);
}

// radialAverage :250
__host__ __device__ __forceinline__ int vs_bin_round(int k, int i, int j, int Z, int Y, int X) { return (int)round(vs_w_fast(k, i, j, Z, Y, X) * X); }

__device__ __forceinline__ double vs_nonneg(double v) { return 0.0 < v ? v : 0.0; }   // std::max(0.0, v)

__device__ __forceinline__ double vs_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }   // POCSMinMax :179-187

// ---------------------------------------------------------------- real space
// POCSmask and POCSnonnegative of an input (:425-426, :430-431) with the sum and the sum of squares; mask null: ones
__global__ void __launch_bounds__(256)
k_vs_prepare(const double *__restrict__ in, const double *__restrict__ mask, double *__restrict__ out, size_t N, double *__restrict__ partials)
{
    double s[2] = {0, 0};
    XH_GRID_LOOP(n, N) {
        double v = in[n];
        if (mask) v *= mask[n];
        v = vs_nonneg(v);
        out[n] = v;
        s[0] += v;
        s[1] += v * v;
    }
    xh_block_partials(s, partials);
}

// computeDoubleMinMax: a workgroup's minimum and maximum to mm [2][gridDim.x]. The order of comparisons does not change either
__global__ void __launch_bounds__(256) k_vs_minmax(const double *__restrict__ v, size_t N, double *__restrict__ mm)
{
    __shared__ double lo[256], hi[256];
    double a = v[0], b = v[0];
    XH_GRID_LOOP(n, N) {
        const double x = v[n];
        a = x < a ? x : a;
        b = x > b ? x : b;
    }
    lo[threadIdx.x] = a;
    hi[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            if (lo[threadIdx.x + s] < lo[threadIdx.x]) lo[threadIdx.x] = lo[threadIdx.x + s];
            if (hi[threadIdx.x + s] > hi[threadIdx.x]) hi[threadIdx.x] = hi[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mm[blockIdx.x] = lo[0];
        mm[gridDim.x + blockIdx.x] = hi[0];
    }
}

// POCSMinMax and POCSmask (:380, :385) in one pass; mask null: ones
__global__ void __launch_bounds__(256) k_vs_clip_mask(double *__restrict__ v, const double *__restrict__ mask, size_t N, double lo, double hi)
{
    XH_GRID_LOOP(n, N) {
        double x = vs_clip(v[n], lo, hi);
        if (mask) x *= mask[n];
        v[n] = x;
    }
}

// POCSnonnegative (:397) with the moments of its result for computeStddev (:402)
__global__ void __launch_bounds__(256) k_vs_nonneg_moments(double *__restrict__ v, size_t N, double *__restrict__ partials)
{
    double s[2] = {0, 0};
    XH_GRID_LOOP(n, N) {
        const double x = vs_nonneg(v[n]);
        v[n] = x;
        s[0] += x;
        s[1] += x * x;
    }
    xh_block_partials(s, partials);
}

// V *= std1 / std2 (:403) on its way out
__global__ void __launch_bounds__(256) k_vs_scale(const double *__restrict__ v, double *__restrict__ out, size_t N, double f)
{
    XH_GRID_LOOP(n, N) out[n] = v[n] * f;
}

// the sums behind computeEnergy (:205-211) of the steps between two states in memory, read only. prev fprev is the state before, cur the
// one after the transform pair.
//   VS_E_AMP_CLIP_MASK  (prev fprev - cur)^2, (cur - clip)^2, (clip - clip mask)^2     :376-389
//   VS_E_PHASE_NONNEG   (prev - cur)^2, (cur - max(0, cur))^2                          :393-401
//   VS_E_SCALE          (cur - cur fprev)^2                                            :404-407
//   VS_E_FILTER         (prev fprev - cur)^2                                           :413-416
__global__ void __launch_bounds__(256)
k_vs_energy(const double *__restrict__ prev, double fprev, const double *__restrict__ cur, const double *__restrict__ mask, size_t N, double lo, double hi, int mode,
            double *__restrict__ partials)
{
    double s[3] = {0, 0, 0};
    XH_GRID_LOOP(n, N) {
        const double x = cur[n];
        if (mode == VS_E_SCALE) {
            const double d = x - x * fprev;
            s[0] += d * d;
            continue;
        }
        const double a = prev[n] * fprev;
        const double d0 = a - x;
        s[0] += d0 * d0;
        if (mode == VS_E_AMP_CLIP_MASK) {
            const double c = vs_clip(x, lo, hi);
            const double m = mask ? c * mask[n] : c;
            const double d1 = x - c, d2 = c - m;
            s[1] += d1 * d1;
            s[2] += d2 * d2;
        } else if (mode == VS_E_PHASE_NONNEG) {
            const double d1 = x - vs_nonneg(x);
            s[1] += d1 * d1;
        }
    }
    xh_block_partials(s, partials);
}

// subtraction :298-304
__global__ void __launch_bounds__(256)
k_vs_subtract(const double *__restrict__ v1, const double *__restrict__ v1f, const double *__restrict__ v, const double *__restrict__ m, double *__restrict__ out, size_t N)
{
    XH_GRID_LOOP(n, N) {
        const double f = v1f[n], mk = m[n];
        const double a = v1[n] * (1 - mk);
        const double mn = v[n] < f ? v[n] : f;   // std::min(V, V1F)
        const double b = (f - mn) * mk;
        out[n] = a + b;
    }
}

// ---------------------------------------------------------------- spectrum
// FFT_magnitude: std::abs of every coefficient
__global__ void __launch_bounds__(256) k_vs_magnitude(const xh_cd *__restrict__ F, double *__restrict__ mag, size_t NF)
{
    XH_GRID_LOOP(e, NF) mag[e] = hypot(F[e].x, F[e].y);
}

// extractPhase :197-203, and the magnitude when mag is not null
__global__ void __launch_bounds__(256) k_vs_extract_phase(const xh_cd *__restrict__ F, xh_cd *__restrict__ P, double *__restrict__ mag, size_t NF)
{
    XH_GRID_LOOP(e, NF) {
        const xh_cd f = F[e];
        const double phi = atan2(f.y, f.x);
        P[e] = xh_cd{cos(phi), sin(phi)};
        if (mag) mag[e] = hypot(f.x, f.y);
    }
}

// POCSFourierAmplitude :138-147
__global__ void __launch_bounds__(256) k_vs_amplitude(xh_cd *__restrict__ F, const double *__restrict__ v1mag, size_t NF, double l)
{
    XH_GRID_LOOP(e, NF) {
        const xh_cd f = F[e];
        const double mod = hypot(f.x, f.y);
        if (mod > 1e-10) {
            const double g = ((1 - l) + l * v1mag[e]) / mod;
            F[e] = xh_cd{f.x * g, f.y * g};
        }
    }
}

// POCSFourierAmplitudeRadAvg :149-177
__global__ void __launch_bounds__(256) k_vs_amplitude_radavg(xh_cd *__restrict__ F, const double *__restrict__ rq, int nbins, size_t NF, XhDims d, double l)
{
    XH_GRID_LOOP(e, NF) {
        int k, i, j;
        xh_kij(e, d, k, i, j);
        const double w = vs_w_fast(k, i, j, d.Z, d.Y, d.X);
        const int iw = min((int)floor(w * d.X), nbins - 1);
        const double g = (1 - l) + l * rq[iw];
        const xh_cd f = F[e];
        F[e] = xh_cd{f.x * g, f.y * g};
    }
}

// POCSFourierPhase :189-194
__global__ void __launch_bounds__(256) k_vs_phase(xh_cd *__restrict__ F, const xh_cd *__restrict__ P, size_t NF)
{
    XH_GRID_LOOP(e, NF) {
        const double mod = hypot(F[e].x, F[e].y);
        F[e] = xh_cd{mod * P[e].x, mod * P[e].y};
    }
}

// FourierFilter LOWPASS (fourier_filter.cpp:423-439): RAISED_COSINE with w1 = cut (GAUSS false) or REALGAUSSIAN with w1 = cut (GAUSS true)
template <bool GAUSS> __global__ void __launch_bounds__(256) k_vs_lowpass(xh_cd *__restrict__ F, size_t NF, XhDims d, double cut)
{
    XH_GRID_LOOP(e, NF) {
        int k, i, j;
        xh_kij(e, d, k, i, j);
        const double wx = d_digfreq(j, d.X), wy = d_digfreq(i, d.Y), wz = d_digfreq(k, d.Z);
        const double absw = sqrt(wx * wx + wy * wy + wz * wz);
        double m;
        if (GAUSS) m = exp(-VS_PI * VS_PI * absw * absw * cut * cut);
        else if (absw < cut) m = 1;
        else if (absw < cut + VS_RAISED_W) m = (1 + cos(VS_PI / VS_RAISED_W * (absw - cut))) / 2;
        else m = 0;
        F[e] = xh_cd{F[e].x * m, F[e].y * m};
    }
}

// ---------------------------------------------------------------- radial mean
// the runs of one octant row (k, i): a row per workgroup and lap. slots [nrows][xq], zeroed before
__global__ void __launch_bounds__(256) k_vs_radial_rows(const double *__restrict__ mag, double *__restrict__ slots, XhDims d)
{
    const int zq = d.Z / 2, yq = d.Y / 2, xq = d.X / 2;
    const int nrows = zq * yq;
    for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int k = row / yq, i = row - k * yq;
        const int b0 = vs_bin_round(k, i, 0, d.Z, d.Y, d.X);
        const double *line = mag + ((size_t)k * d.Y + i) * d.xh;
        for (int j = threadIdx.x; j < xq; j += 256) {
            const int b = vs_bin_round(k, i, j, d.Z, d.Y, d.X);
            if (j > 0 && vs_bin_round(k, i, j - 1, d.Z, d.Y, d.X) == b) continue;   // not the head of its run
            double s = line[j];
            for (int jj = j + 1; jj < xq && vs_bin_round(k, i, jj, d.Z, d.Y, d.X) == b; ++jj) s += line[jj];
            const int slot = b - b0;
            if (slot < xq) slots[(size_t)row * xq + slot] = s;   // always: the bin grows by at most one per element
        }
    }
}

// bin b = blockIdx.x: the rows in row order, then the tree
__global__ void __launch_bounds__(256) k_vs_radial_bins(const double *__restrict__ slots, double *__restrict__ sums, XhDims d)
{
    __shared__ double red[1][256];
    const int zq = d.Z / 2, yq = d.Y / 2, xq = d.X / 2;
    const int nrows = zq * yq, b = blockIdx.x;
    double v[1] = {0.0};
    for (int row = threadIdx.x; row < nrows; row += 256) {
        const int k = row / yq, i = row - k * yq;
        const int slot = b - vs_bin_round(k, i, 0, d.Z, d.Y, d.X);
        if (slot >= 0 && slot < xq) v[0] += slots[(size_t)row * xq + slot];
    }
    xh_tree256(red, v);
    if (threadIdx.x == 0) sums[b] = red[0][0];
}

// :235
int vs_num_bins(int Z, int Y, int X)
{
    const int x2 = X / 2, y2 = Y / 2, z2 = Z / 2;
    return (int)std::floor(std::sqrt((double)(x2 * x2 + y2 * y2 + z2 * z2)));
}

// the largest bin radialAverage writes: w grows with every index inside the octant
int vs_max_bin(int Z, int Y, int X) { return vs_bin_round(Z / 2 - 1, Y / 2 - 1, X / 2 - 1, Z, Y, X); }

}  // namespace

struct xh_vsub : XhVolume {
    unsigned grid = 0;
    int nbins = 0;
    XhBuf F, P, v1mag, mag, mask, V, prev, tmp, slots, binsums, rq, partials, result, energies;
    XhPinned host;
    XhLapTimer<VS_NT> tm;
    bool haveRef = false, haveMask = false, haveRadial = false, havePhase = false;
    double v1min = 0, v1max = 0, std1 = 0;
    std::vector<double> count, meanV1, meanV, quotient;
    ~xh_vsub() { finish(); }
};

namespace {

const double *maskp(xh_vsub *h) { return h->haveMask ? (const double *)h->mask.p : nullptr; }

// computeStddev from the sum and the sum of squares
double vs_stddev(double sum, double sum2, double N)
{
    const double avg = sum / N;
    return N > 1 ? std::sqrt(std::fabs(sum2 / N - avg * avg) * N / (N - 1)) : 0.0;
}

int vs_check_radavg(const XhDims &d)
{
    const int nb = vs_num_bins(d.Z, d.Y, d.X), mb = vs_max_bin(d.Z, d.Y, d.X);
    XH_CHECK(d.Z >= 2 && d.Y >= 2 && d.X >= 2 && nb >= 1 && mb < nb, XH_ERR_UNSUPPORTED,
             "volume subtraction: --radavg on a %d x %d x %d box: the radial average's largest bin %d reaches its %d bins (the reference writes past radial_mean)", d.Z, d.Y,
             d.X, mb, nb);
    return XH_OK;
}

// radialAverage of a magnitude [Z][Y][xh] on the device, to the host
int vs_radial_mean(xh_vsub *h, const double *d_mag, std::vector<double> &mean)
{
    XH_TRY(vs_check_radavg(h->d));
    const XhDims d = h->d;
    const int zq = d.Z / 2, yq = d.Y / 2, xq = d.X / 2, nrows = zq * yq, nb = h->nbins;
    if (h->count.empty()) {
        h->count.assign(nb, 0.0);
        for (int k = 0; k < zq; ++k)
            for (int i = 0; i < yq; ++i)
                for (int j = 0; j < xq; ++j) h->count[vs_bin_round(k, i, j, d.Z, d.Y, d.X)] += 1.0;
        XH_TRY(xh_buf_alloc(h->ctx, h->slots, sizeof(double) * (size_t)nrows * xq));
        XH_TRY(xh_buf_alloc(h->ctx, h->binsums, sizeof(double) * nb));
        XH_TRY(xh_buf_alloc(h->ctx, h->rq, sizeof(double) * nb));
    }
    hipStream_t st = h->ctx->stream;
    XH_HIP(hipMemsetAsync(h->slots.p, 0, h->slots.bytes, st));
    XH_LAUNCH256(h->ctx, k_vs_radial_rows, (unsigned)std::min(nrows, 4096), d_mag, dp(h->slots), d);
    XH_LAUNCH256(h->ctx, k_vs_radial_bins, (unsigned)nb, (const double *)h->slots.p, dp(h->binsums), d);
    mean.resize(nb);
    XH_HIP(hipMemcpyAsync(mean.data(), h->binsums.p, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < nb; ++b) mean[b] /= h->count[b];   // :256, 0 / 0 included
    return XH_OK;
}

// computeRadQuotient :267-273
void vs_quotient(const std::vector<double> &m1, const std::vector<double> &m2, std::vector<double> &q)
{
    q.resize(m1.size());
    for (size_t b = 0; b < m1.size(); ++b) {
        double v = m1[b] / m2[b];
        v = std::min(v, 1.0);
        if (v != v) v = 0;
        q[b] = v;
    }
}

// the phase of d_v's transform (:434) and, with radavg, the quotient table of its magnitude against the reference's (:436-437)
int vs_target(xh_vsub *h, const double *d_v, bool radavg)
{
    XH_TRY(h->tm.start());
    XH_TRY(h->fft.r2c(d_v, cp(h->F), 1.0 / (double)h->N));
    XH_TRY(h->tm.lap(VS_T_TRANSFORMS));
    XH_LAUNCH256(h->ctx, k_vs_extract_phase, h->grid, (const xh_cd *)h->F.p, cp(h->P), radavg ? dp(h->mag) : (double *)nullptr, h->NF);
    XH_TRY(h->tm.lap(VS_T_SPECTRUM));
    h->havePhase = true;
    if (radavg) {
        XH_CHECK(h->haveRadial, XH_ERR_STATE, "volume subtraction: the reference was set without its radial mean");
        XH_TRY(vs_radial_mean(h, (const double *)h->mag.p, h->meanV));
        vs_quotient(h->meanV1, h->meanV, h->quotient);
        XH_HIP(hipMemcpyAsync(h->rq.p, h->quotient.data(), sizeof(double) * h->nbins, hipMemcpyHostToDevice, h->ctx->stream));
        XH_HIP(hipStreamSynchronize(h->ctx->stream));
        XH_TRY(h->tm.start());
    }
    return XH_OK;
}

// three sums of an energy kernel to e [3] on the device
int vs_energy(xh_vsub *h, const double *prev, double fprev, const double *cur, int mode, double *e)
{
    XH_LAUNCH256(h->ctx, k_vs_energy, h->grid, prev, fprev, cur, maskp(h), h->N, h->v1min, h->v1max, mode, dp(h->partials));
    XH_LAUNCH256(h->ctx, xh_k_reduce_final, 1, (const double *)h->partials.p, (int)h->grid, 3, e);
    return XH_OK;
}

int vs_check_options(const char *who, int32_t iter, double lambda, double cutFreq)
{
    XH_CHECK(iter >= 0, XH_ERR_ARG, "%s: %d iterations", who, iter);
    XH_CHECK(lambda >= 0 && lambda <= 1, XH_ERR_ARG, "%s: lambda %g is outside [0, 1]", who, lambda);
    XH_CHECK(cutFreq >= 0 && cutFreq <= 0.5, XH_ERR_ARG, "%s: cutFreq %g is outside [0, 0.5]", who, cutFreq);
    return XH_OK;
}

// runIteration (:362-418) on h->V, whose values stand for V times *pending. e: 12 doubles on the device for the energy sums, or null
int vs_iteration(xh_vsub *h, double lambda, bool radavg, double cutFreq, double *pending, double *e)
{
    hipStream_t st = h->ctx->stream;
    const double iN = 1.0 / (double)h->N;
    double *V = dp(h->V), *prev = dp(h->prev);
    XH_TRY(h->tm.start());
    // :365-375
    XH_TRY(h->fft.r2c(V, cp(h->F), *pending * iN));
    XH_TRY(h->tm.lap(VS_T_TRANSFORMS));
    if (radavg) XH_LAUNCH256(h->ctx, k_vs_amplitude_radavg, h->grid, cp(h->F), (const double *)h->rq.p, h->nbins, h->NF, h->d, lambda);
    else XH_LAUNCH256(h->ctx, k_vs_amplitude, h->grid, cp(h->F), (const double *)h->v1mag.p, h->NF, lambda);
    XH_TRY(h->tm.lap(VS_T_SPECTRUM));
    if (e) XH_HIP(hipMemcpyAsync(prev, V, h->V.bytes, hipMemcpyDeviceToDevice, st));
    XH_TRY(h->fft.c2r(cp(h->F), V, 1.0));
    XH_TRY(h->tm.lap(VS_T_TRANSFORMS));
    // :376-389
    if (e) XH_TRY(vs_energy(h, prev, *pending, V, VS_E_AMP_CLIP_MASK, e));
    XH_LAUNCH256(h->ctx, k_vs_clip_mask, h->grid, V, maskp(h), h->N, h->v1min, h->v1max);
    XH_TRY(h->tm.lap(VS_T_REAL));
    // :390-392
    XH_TRY(h->fft.r2c(V, cp(h->F), iN));
    XH_TRY(h->tm.lap(VS_T_TRANSFORMS));
    XH_LAUNCH256(h->ctx, k_vs_phase, h->grid, cp(h->F), (const xh_cd *)h->P.p, h->NF);
    XH_TRY(h->tm.lap(VS_T_SPECTRUM));
    if (e) XH_HIP(hipMemcpyAsync(prev, V, h->V.bytes, hipMemcpyDeviceToDevice, st));
    XH_TRY(h->fft.c2r(cp(h->F), V, 1.0));
    XH_TRY(h->tm.lap(VS_T_TRANSFORMS));
    // :393-403
    if (e) XH_TRY(vs_energy(h, prev, 1.0, V, VS_E_PHASE_NONNEG, e + 3));
    XH_LAUNCH256(h->ctx, k_vs_nonneg_moments, h->grid, V, h->N, dp(h->partials));
    double *hp = h->host.f64();
    XH_TRY(xh_reduce_finish(h->ctx, (const double *)h->partials.p, (int)h->grid, 2, dp(h->result), hp));
    const double std2 = vs_stddev(hp[0], hp[1], (double)h->N);
    XH_CHECK(std2 > 0 && std::isfinite(std2), XH_ERR_ARG, "volume subtraction: stddev(V) = %g after the phase step: std1 / stddev(V) is undefined", std2);
    *pending = h->std1 / std2;
    XH_TRY(h->tm.lap(VS_T_REAL));
    if (e) XH_TRY(vs_energy(h, V, *pending, V, VS_E_SCALE, e + 6));
    // :409-417
    if (cutFreq != 0) {
        XH_TRY(h->fft.r2c(V, cp(h->F), *pending * iN));
        XH_LAUNCH256(h->ctx, k_vs_lowpass<false>, h->grid, cp(h->F), h->NF, h->d, cutFreq);
        if (e) XH_HIP(hipMemcpyAsync(prev, V, h->V.bytes, hipMemcpyDeviceToDevice, st));
        XH_TRY(h->fft.c2r(cp(h->F), V, 1.0));
        if (e) XH_TRY(vs_energy(h, prev, *pending, V, VS_E_FILTER, e + 9));
        *pending = 1.0;
        XH_TRY(h->tm.lap(VS_T_FILTER));
    }
    return XH_OK;
}

// `iter` iterations on h->V, then the pending scale on the way to d_out
int vs_iterate(xh_vsub *h, int32_t iter, double lambda, bool radavg, double cutFreq, xh_vsub_energy *energies, double *d_out)
{
    hipStream_t st = h->ctx->stream;
    if (energies && iter > 0) {
        XH_TRY(xh_buf_reserve(h->ctx, h->energies, sizeof(double) * 12 * (size_t)iter));
        XH_HIP(hipMemsetAsync(h->energies.p, 0, sizeof(double) * 12 * (size_t)iter, st));
    }
    double pending = 1.0;
    for (int32_t n = 0; n < iter; ++n) XH_TRY(vs_iteration(h, lambda, radavg, cutFreq, &pending, energies ? dp(h->energies) + 12 * (size_t)n : nullptr));
    XH_TRY(h->tm.start());
    XH_LAUNCH256(h->ctx, k_vs_scale, h->grid, (const double *)h->V.p, d_out, h->N, pending);
    XH_TRY(h->tm.lap(VS_T_REAL));
    if (energies && iter > 0) {
        std::vector<double> s(12 * (size_t)iter);
        XH_HIP(hipMemcpyAsync(s.data(), h->energies.p, sizeof(double) * s.size(), hipMemcpyDeviceToHost, st));
        XH_HIP(hipStreamSynchronize(st));
        const double N = (double)h->N;
        for (int32_t n = 0; n < iter; ++n) {
            const double *q = s.data() + 12 * (size_t)n;
            xh_vsub_energy &r = energies[n];
            r.amplitude = std::sqrt(q[0] / N); r.minmax = std::sqrt(q[1] / N); r.mask = std::sqrt(q[2] / N);
            r.phase = std::sqrt(q[3] / N); r.nonneg = std::sqrt(q[4] / N); r.scale = std::sqrt(q[6] / N);
            r.filter = cutFreq != 0 ? std::sqrt(q[9] / N) : 0.0;
        }
    }
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

// d_in through a low pass, to d_out (d_in == d_out allowed)
template <bool GAUSS> int vs_lowpass(xh_vsub *h, const double *d_in, double cut, double *d_out)
{
    XH_TRY(h->fft.r2c(d_in, cp(h->F), 1.0 / (double)h->N));
    XH_LAUNCH256(h->ctx, k_vs_lowpass<GAUSS>, h->grid, cp(h->F), h->NF, h->d, cut);
    return h->fft.c2r(cp(h->F), d_out, 1.0);
}

}  // namespace

extern "C" {

int xh_vsub_radial_bins(int32_t Z, int32_t Y, int32_t X, int32_t *nbins, int32_t *maxbin)
{
    XH_CHECK(nbins && maxbin, XH_ERR_ARG, "xh_vsub_radial_bins: null argument");
    XH_CHECK(Z >= 2 && Y >= 2 && X >= 2, XH_ERR_ARG, "xh_vsub_radial_bins: bad size %d x %d x %d", Z, Y, X);
    *nbins = vs_num_bins(Z, Y, X);
    *maxbin = vs_max_bin(Z, Y, X);
    return XH_OK;
}

int xh_vsub_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, xh_vsub **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_vsub_create: null argument");
    XH_CHECK(Z >= 2 && Y >= 2 && X >= 2, XH_ERR_ARG, "xh_vsub_create: bad size %d x %d x %d", Z, Y, X);
    XH_CHECK(Z <= 1024 && Y <= 1024 && X <= 1024, XH_ERR_UNSUPPORTED, "xh_vsub_create: sizes above 1024 are not supported (%d x %d x %d)", Z, Y, X);
    std::unique_ptr<xh_vsub> h(new xh_vsub);
    XH_TRY(h->init(ctx, Z, Y, X));
    h->nbins = vs_num_bins(Z, Y, X);
    h->grid = xh_grid256(h->N, ctx->num_cus, 8);
    const size_t vb = sizeof(double) * h->N, fb = sizeof(xh_cd) * h->NF;
    for (XhBuf *b : {&h->mask, &h->V, &h->prev, &h->tmp}) XH_TRY(xh_buf_alloc(ctx, *b, vb));
    for (XhBuf *b : {&h->F, &h->P}) XH_TRY(xh_buf_alloc(ctx, *b, fb));
    for (XhBuf *b : {&h->v1mag, &h->mag}) XH_TRY(xh_buf_alloc(ctx, *b, fb / 2));
    XH_TRY(xh_buf_alloc(ctx, h->partials, sizeof(double) * 3 * h->grid));
    XH_TRY(xh_buf_alloc(ctx, h->result, sizeof(double) * 4));
    XH_TRY(xh_pinned_alloc(ctx, h->host, sizeof(double) * 8));
    XH_TRY(h->tm.create(ctx));
    *out = h.release();
    return XH_OK;
}

int xh_vsub_destroy(xh_vsub *h)
{
    delete h;
    return XH_OK;
}

int xh_vsub_set_reference(xh_vsub *h, const double *d_V1, const double *d_mask, int32_t radavg)
{
    XH_CHECK(h && d_V1, XH_ERR_ARG, "xh_vsub_set_reference: null argument");
    if (radavg) XH_TRY(vs_check_radavg(h->d));
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    h->haveRef = h->haveRadial = h->havePhase = false;
    h->haveMask = d_mask != nullptr;
    if (d_mask) XH_HIP(hipMemcpyAsync(h->mask.p, d_mask, h->mask.bytes, hipMemcpyDeviceToDevice, st));
    // :425-427, :432
    double *w = dp(h->tmp);
    XH_LAUNCH256(h->ctx, k_vs_prepare, h->grid, d_V1, maskp(h), w, h->N, dp(h->partials));
    double *hp = h->host.f64();
    XH_TRY(xh_reduce_finish(h->ctx, (const double *)h->partials.p, (int)h->grid, 2, dp(h->result), hp));
    h->std1 = vs_stddev(hp[0], hp[1], (double)h->N);
    XH_LAUNCH256(h->ctx, k_vs_minmax, h->grid, (const double *)w, h->N, dp(h->partials));
    std::vector<double> mm(2 * (size_t)h->grid);
    XH_HIP(hipMemcpyAsync(mm.data(), h->partials.p, sizeof(double) * mm.size(), hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    h->v1min = mm[0];
    h->v1max = mm[h->grid];
    for (unsigned g = 0; g < h->grid; ++g) {
        h->v1min = std::min(h->v1min, mm[g]);
        h->v1max = std::max(h->v1max, mm[h->grid + g]);
    }
    XH_CHECK(h->std1 > 0 && std::isfinite(h->std1), XH_ERR_ARG, "xh_vsub_set_reference: the masked, clipped reference has stddev %g", h->std1);
    // :435
    XH_TRY(h->fft.r2c(w, cp(h->F), 1.0 / (double)h->N));
    XH_LAUNCH256(h->ctx, k_vs_magnitude, h->grid, (const xh_cd *)h->F.p, dp(h->v1mag), h->NF);
    if (radavg) {
        XH_TRY(vs_radial_mean(h, (const double *)h->v1mag.p, h->meanV1));
        h->haveRadial = true;
    }
    XH_HIP(hipStreamSynchronize(st));
    h->haveRef = true;
    return XH_OK;
}

int xh_vsub_info(const xh_vsub *h, double *v1min, double *v1max, double *std1, int32_t *nbins)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_vsub_info: null handle");
    XH_CHECK(h->haveRef, XH_ERR_STATE, "xh_vsub_info: no reference is set");
    if (v1min) *v1min = h->v1min;
    if (v1max) *v1max = h->v1max;
    if (std1) *std1 = h->std1;
    if (nbins) *nbins = h->nbins;
    return XH_OK;
}

int xh_vsub_reference_magnitude(xh_vsub *h, double *d_out)
{
    XH_CHECK(h && d_out, XH_ERR_ARG, "xh_vsub_reference_magnitude: null argument");
    XH_CHECK(h->haveRef, XH_ERR_STATE, "xh_vsub_reference_magnitude: no reference is set");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(d_out, h->v1mag.p, h->v1mag.bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
    return XH_OK;
}

int xh_vsub_radial_mean(xh_vsub *h, const double *d_mag, double *h_mean)
{
    XH_CHECK(h && d_mag && h_mean, XH_ERR_ARG, "xh_vsub_radial_mean: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    std::vector<double> m;
    XH_TRY(vs_radial_mean(h, d_mag, m));
    std::memcpy(h_mean, m.data(), sizeof(double) * m.size());
    return XH_OK;
}

int xh_vsub_quotient(xh_vsub *h, const double *d_V, double *h_quotient)
{
    XH_CHECK(h && d_V && h_quotient, XH_ERR_ARG, "xh_vsub_quotient: null argument");
    XH_CHECK(h->haveRef && h->haveRadial, XH_ERR_STATE, "xh_vsub_quotient: no reference with its radial mean is set");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_TRY(vs_target(h, d_V, true));
    std::memcpy(h_quotient, h->quotient.data(), sizeof(double) * h->quotient.size());
    return XH_OK;
}

int xh_vsub_iteration(xh_vsub *h, const double *d_V0, const double *d_V, double lambda, int32_t radavg, double cutFreq, double *d_out)
{
    XH_CHECK(h && d_V0 && d_V && d_out, XH_ERR_ARG, "xh_vsub_iteration: null argument");
    XH_CHECK(h->haveRef, XH_ERR_STATE, "xh_vsub_iteration: no reference is set");
    XH_TRY(vs_check_options("xh_vsub_iteration", 1, lambda, cutFreq));
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_TRY(vs_target(h, d_V0, radavg != 0));
    XH_HIP(hipMemcpyAsync(h->V.p, d_V, h->V.bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
    return vs_iterate(h, 1, lambda, radavg != 0, cutFreq, nullptr, d_out);
}

int xh_vsub_adjust(xh_vsub *h, const double *d_V, int32_t iter, double lambda, int32_t radavg, double cutFreq, xh_vsub_energy *h_energies, double *d_out)
{
    XH_CHECK(h && d_V && d_out, XH_ERR_ARG, "xh_vsub_adjust: null argument");
    XH_CHECK(h->haveRef, XH_ERR_STATE, "xh_vsub_adjust: no reference is set");
    XH_TRY(vs_check_options("xh_vsub_adjust", iter, lambda, cutFreq));
    XH_HIP(hipSetDevice(h->ctx->device));
    h->tm.zero();
    // :430-431
    XH_TRY(h->tm.start());
    XH_LAUNCH256(h->ctx, k_vs_prepare, h->grid, d_V, maskp(h), dp(h->V), h->N, dp(h->partials));
    XH_TRY(h->tm.lap(VS_T_REAL));
    if (iter > 0) XH_TRY(vs_target(h, (const double *)h->V.p, radavg != 0));
    return vs_iterate(h, iter, lambda, radavg != 0, cutFreq, h_energies, d_out);
}

int xh_vsub_lowpass(xh_vsub *h, const double *d_in, double cutFreq, double *d_out)
{
    XH_CHECK(h && d_in && d_out, XH_ERR_ARG, "xh_vsub_lowpass: null argument");
    XH_CHECK(cutFreq > 0 && cutFreq <= 0.5, XH_ERR_ARG, "xh_vsub_lowpass: cutFreq %g is outside (0, 0.5]", cutFreq);
    XH_HIP(hipSetDevice(h->ctx->device));
    return vs_lowpass<false>(h, d_in, cutFreq, d_out);
}

int xh_vsub_smooth_mask(xh_vsub *h, const double *d_mask, double sigma, double *d_out)
{
    XH_CHECK(h && d_mask && d_out, XH_ERR_ARG, "xh_vsub_smooth_mask: null argument");
    XH_CHECK(sigma >= 0 && std::isfinite(sigma), XH_ERR_ARG, "xh_vsub_smooth_mask: sigma %g", sigma);
    XH_HIP(hipSetDevice(h->ctx->device));
    return vs_lowpass<true>(h, d_mask, sigma, d_out);
}

int xh_vsub_subtract(xh_vsub *h, const double *d_V1_raw, const double *d_Vadj, const double *d_masksub, double cutFreq, double *d_V1F, double *d_out)
{
    XH_CHECK(h && d_V1_raw && d_Vadj && d_masksub && d_out, XH_ERR_ARG, "xh_vsub_subtract: null argument");
    XH_CHECK(cutFreq >= 0 && cutFreq <= 0.5, XH_ERR_ARG, "xh_vsub_subtract: cutFreq %g is outside [0, 0.5]", cutFreq);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    // :287-291
    const double *v1f = d_V1_raw;
    if (cutFreq != 0) {
        XH_TRY(vs_lowpass<false>(h, d_V1_raw, cutFreq, dp(h->tmp)));
        v1f = (const double *)h->tmp.p;
    }
    if (d_V1F) XH_HIP(hipMemcpyAsync(d_V1F, v1f, h->tmp.bytes, hipMemcpyDeviceToDevice, st));
    XH_LAUNCH256(h->ctx, k_vs_subtract, h->grid, d_V1_raw, v1f, d_Vadj, d_masksub, d_out, h->N);
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

int xh_vsub_set_timing(xh_vsub *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_vsub_set_timing: null handle");
    h->tm.set(on != 0);
    return XH_OK;
}

int xh_vsub_stage_ms(const xh_vsub *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_vsub_stage_ms: null argument");
    h->tm.read(h_ms);
    return XH_OK;
}

}  // extern "C"
