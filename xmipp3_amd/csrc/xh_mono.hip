// xh_mono.hip -- the device side of xmipp_resolution_monogenic_signal, MonoRes (reconstruction/resolution_monogenic_signal.{h,cpp} with the
// Monogenic class of data/monogenic_signal.{h,cpp}; the reference has no GPU version), fp64.
//
// The handle owns every buffer of a Z x Y x X volume. A frequency of the sweep is
//   split      one kernel reads the map's spectrum once and writes the four spectra of the step: the raised-cosine high-passed map and its
//              three Riesz components -J ux|uy|uz iu F (amplitudeMonoSig3D_LPF :295-373; iu and the axis vectors come from the index);
//   inverse    the y and z line passes of the four inverse transforms as one batch;
//   rows       the x lines: the four Hermitian lines of a row are two complex lines in LDS (V + i Rx, Ry + i Rz: an inverse transform of
//              A + i B with A, B Hermitian gives a + i b), and only sqrt(((v v + rx rx) + rz rz) + ry ry) is written: the four real
//              volumes never reach memory. The imaginary parts of the DC and Nyquist elements are dropped first, as FFTW's c2r does;
//   smoothing  r2c of the amplitude (1 / N in the row kernel), the low-pass cosine tail, c2r (:388-408);
//   statistics NS, NN and the four sums in one fixed-order reduction (xh_reduce.h), the noise percentile by a one-rank radix select over
//              an order-preserving transform of the doubles' bits (11-bit digits, the keys are recomputed from the values in every pass,
//              so no sentinel key exists); the rank size_t(NN significance) is computed on the device;
//   one wait   a small record goes to the host, which takes every stop decision of ProgMonogenicSignalRes::run (:392-536);
//   assign     setLocalResolutionMap / setLocalResolutionHalfMaps as one kernel on the int mask and the resolution map.
// The select is this file's own: the selection passes of xh_halves.hip resolve 202 ranks of non-negative keys together and mark masked
// voxels with a key, neither of which fits one rank of signed values.
//
// Reference behaviours kept as written:
//  - minRes is overwritten with 2 sampling (:362);
//  - freqL = freq + 0.02 and freqH = freq - 0.02, clipped to 0.5 and 0, replace what resolution2eval returned (:422-427);
//  - freq_step is floored at 0.25 (:162);
//  - volsize = XSIZE (:380): resolution2eval reads the x size whatever the box;
//  - max_meanS starts at -DBL_MIN (:354);
//  - the Riesz components are accumulated V, x, z, y in the sweep (monogenic_signal.cpp :330-386) and V, x, y, z in
//    monogenicAmplitude_3D_Fourier (:606-660);
//  - a voxel that fails the threshold three times is dropped to -1 with a single map and to 0 with half maps (:534, :564);
//  - refiningMask always reads the spectrum of the (mean) map and the noise set mask == 0 (:203-256).
//
// Deviations from the reference, each where it divides by zero, reads past an array or cannot terminate:
//  - a mask without a voxel equal to 1 is refused (NVoxelsOriginalMask = 0: NS / 0);
//  - an empty noise set (NN = 0) is refused, in refiningMask and in the sweep (the reference reads element 0 of an empty vector);
//  - refiningMask leaving no voxel (NVoxelsOriginalMask = 0) is refused;
//  - a sweep that evaluated no frequency, or a map without a voxel at or above the last resolution, is refused in post-processing (the
//    reference reads list[-1], element 0 of an empty array);
//  - resolution2eval: a resolution <= 0 ends the sweep (the reference divides by it and converts the quotient to int);
//  - the low-pass tail with freqL = freq (freq = 0.5): the reference's PI / 0 times 0 is NaN at un = freq and the NaN floods the
//    amplitude; the tail's value there is 1, its limit;
//  - the median of post-processing: the reference counts N with >= and copies with >, leaving zeros where a value equals the bound; the
//    zeros are counted in, not stored.
// icdf_gauss (xmippCore, not in the tree) is restated as Abramowitz-Stegun 26.2.23 (parity unpinned).
#include "xh_volume.h"
#include "xh_reduce.h"
#include <cfloat>
#include <cmath>
#include <cstring>

namespace {

constexpr int MN_W = 11;                 // select: digit width
constexpr int MN_BINS = 1 << MN_W;
enum { MN_SET_ALL = 0, MN_SET_MASK_EQ0 = 1, MN_SET_MASK_GE0 = 2, MN_SET_VAL_GT = 3 };
enum { MN_T_SPLIT = 0, MN_T_INVERSE, MN_T_ROWS, MN_T_SMOOTH, MN_T_STATS, MN_T_SELECT, MN_T_ASSIGN, MN_NT };

struct MnSel {
    unsigned long long prefix, krem, bad;
    double value;
    unsigned int hist[MN_BINS];
};

// fourierFreqVector (monogenic_signal.cpp :132-143): 1e-38 at index 0
__device__ __forceinline__ double mn_axis(int idx, int size) { return idx == 0 ? 1e-38 : d_digfreq(idx, size); }

// fourierFreqs_3D (:174-199): 1 / sqrt(u2), 1e38 at the origin
__device__ __forceinline__ double mn_iu(int k, int i, int j, XhDims d)
{
    if (k == 0 && i == 0 && j == 0) return 1e38;
    const double uz = d_digfreq(k, d.Z), uy = d_digfreq(i, d.Y), ux = d_digfreq(j, d.X);
    const double uz2 = uz * uz;
    const double uz2y2 = uz2 + uy * uy;
    const double u2 = uz2y2 + ux * ux;
    return 1 / sqrt(u2);
}

// ---------------------------------------------------------------- side info
// V = 0.5 (V1 + V2), noise = (V1 - V2) / 2 (produceSideInfo :101-105)
__global__ void __launch_bounds__(256) k_mn_mean_diff(const double *__restrict__ V1, const double *__restrict__ V2, double *__restrict__ V, double *__restrict__ Nz, size_t N)
{
    XH_GRID_LOOP(n, N) {
        const double a = V1[n], b = V2[n];
        V[n] = 0.5 * (a + b);
        Nz[n] = (a - b) / 2;
    }
}

// proteinRadiusVolumeAndShellStatistics (:36-55): the largest R2 of a voxel equal to 1 and their number. Integer atomics: any order
// gives the same result
__global__ void __launch_bounds__(256) k_mn_radius(const int *__restrict__ mask, XhDims d, unsigned long long *__restrict__ out)
{
    unsigned long long r2max = 0, cnt = 0;
    XH_GRID_LOOP(n, (size_t)d.Z * d.Y * d.X) {
        if (mask[n] == 1) {
            const long long j = (long long)(n % d.X) - d.X / 2;
            const size_t r = n / d.X;
            const long long i = (long long)(r % d.Y) - d.Y / 2, k = (long long)(r / d.Y) - d.Z / 2;
            r2max = max(r2max, (unsigned long long)(k * k + i * i + j * j));
            ++cnt;
        }
    }
    if (cnt) {
        atomicMax(out, r2max);
        atomicAdd(out + 1, cnt);
    }
}

__device__ __forceinline__ long long mn_isqrt(long long n)
{
    long long r = (long long)sqrt((double)n);
    while (r * r > n) --r;
    while ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

// findCliffValue's shells (:75-94) in one pass: workgroup kk takes plane kk, thread t the shells t, t + 256, ..: it walks its ring of the
// plane row by row, x ascending, so every sum has a fixed order. part [Z][3][nshell]: sum, sum2, N
__global__ void __launch_bounds__(256) k_mn_shell_planes(const double *__restrict__ V, XhDims d, int nshell, double *__restrict__ part)
{
    const int kk = blockIdx.x;
    const long long k = kk - d.Z / 2, k2 = k * k;
    const int x0 = -(d.X / 2), x1 = x0 + d.X - 1;
    for (int r = threadIdx.x; r < nshell; r += 256) {
        double s = 0, s2 = 0, c = 0;
        const long long lo = (long long)r * r - k2, hi = (long long)(r + 1) * (r + 1) - k2;
        if (hi > 0)
            for (int ii = 0; ii < d.Y; ++ii) {
                const long long i = ii - d.Y / 2;
                const long long lo_i = lo - i * i, hi_i = hi - i * i;
                if (hi_i <= 0) continue;
                const long long jmax = mn_isqrt(hi_i - 1), jmin = lo_i <= 0 ? 0 : mn_isqrt(lo_i - 1) + 1;
                if (jmin > jmax) continue;
                const double *row = V + ((size_t)kk * d.Y + ii) * d.X - x0;
                for (long long j = max(-jmax, (long long)x0); j <= min(-max(jmin, 1LL), (long long)x1); ++j) {
                    const double v = row[j];
                    s += v; s2 += v * v; c += 1;
                }
                for (long long j = max(jmin, (long long)x0); j <= min(jmax, (long long)x1); ++j) {
                    const double v = row[j];
                    s += v; s2 += v * v; c += 1;
                }
            }
        double *p = part + (size_t)kk * 3 * nshell;
        p[r] = s; p[nshell + r] = s2; p[2 * nshell + r] = c;
    }
}

// planes added in increasing order: out [3][nshell]
__global__ void __launch_bounds__(256) k_mn_shell_final(const double *__restrict__ part, int Z, int nshell, double *__restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * nshell) return;
    double s = 0;
    for (int kk = 0; kk < Z; ++kk) s += part[(size_t)kk * 3 * nshell + t];
    out[t] = s;
}

// findCliffValue :119-124: voxels at or beyond raux are -1
__global__ void __launch_bounds__(256) k_mn_cliff_mask(int *__restrict__ mask, XhDims d, double raux2)
{
    XH_GRID_LOOP(n, (size_t)d.Z * d.Y * d.X) {
        const long long j = (long long)(n % d.X) - d.X / 2;
        const size_t r = n / d.X;
        const long long i = (long long)(r % d.Y) - d.Y / 2, k = (long long)(r / d.Y) - d.Z / 2;
        const double aux = (double)(k * k + i * i + j * j);
        if (aux >= raux2) mask[n] = -1;
    }
}

// excludeArea (:169-200) with excl, the --noiseonlyinhalves relabelling (:143-150) without
__global__ void __launch_bounds__(256) k_mn_exclude(int *__restrict__ mask, const int *__restrict__ excl, int halves, int noiseOnly, size_t N)
{
    XH_GRID_LOOP(n, N) {
        int m = mask[n];
        if (excl) {
            if (halves) {
                if (noiseOnly) {
                    if (m == 1) { if (excl[n] == 1) m = -1; }
                    else m = -1;
                }
            } else if (m == 1 && excl[n] == 1) m = -1;
        } else if (halves && noiseOnly && m < 1) m = -1;
        mask[n] = m;
    }
}

// ---------------------------------------------------------------- the amplitude of one frequency
// amplitudeMonoSig3D_LPF :295-373 (BAND) and monogenicAmplitude_3D_Fourier :591-648: F -> F4 = [V, Rx, Ry, Rz]
template <bool BAND>
__global__ void __launch_bounds__(256)
k_mn_split(const xh_cd *__restrict__ F, xh_cd *__restrict__ F4, size_t NF, XhDims d, double freq, double freqH, double ideltal)
{
    XH_GRID_LOOP(e, NF) {
        int k, i, j;
        xh_kij(e, d, k, i, j);
        const double iun = mn_iu(k, i, j, d);
        xh_cd f = xh_cd{0.0, 0.0}, aux = xh_cd{0.0, 0.0};
        bool in = true;
        if (BAND) {
            const double un = 1.0 / iun;
            if (freqH <= un && un <= freq) {
                f = F[e];
                const double H = 0.5 * (1 + cos((un - freq) * ideltal));
                f.x *= H; f.y *= H;
            } else if (un > freq) f = F[e];
            else in = false;
        } else f = F[e];
        if (in) { aux.x = f.y * iun; aux.y = (-f.x) * iun; }       // -J f iu
        const double ux = mn_axis(j, d.X), uy = mn_axis(i, d.Y), uz = mn_axis(k, d.Z);
        F4[e] = f;
        F4[NF + e] = xh_cd{ux * aux.x, ux * aux.y};
        F4[2 * NF + e] = xh_cd{uy * aux.x, uy * aux.y};
        F4[3 * NF + e] = xh_cd{uz * aux.x, uz * aux.y};
    }
}

// the x lines of the four inverse transforms and the amplitude (:330-386; :606-660 with SWEEP false). rpb rows per workgroup, two
// complex lines of M elements per row in LDS
template <bool SWEEP>
__global__ void __launch_bounds__(256)
k_mn_rows_amp(const xh_cd *__restrict__ F4, double *__restrict__ amp, XhPlan<double> plan, size_t nrows, size_t NF, int X, int xh, int rpb)
{
    extern __shared__ __align__(16) unsigned char mn_smem[];
    xh_cd *s = reinterpret_cast<xh_cd *>(mn_smem);
    const int M = 1 << plan.logM;
    const int tid = threadIdx.x, nth = blockDim.x;
    const size_t row0 = (size_t)blockIdx.x * rpb;
    const int nr = (int)min((size_t)rpb, nrows - row0);
    for (int q = tid; q < rpb * 2 * X; q += nth) {
        const int l = q / X, e = q - l * X, r = l >> 1, p = l & 1;
        xh_cd v = xh_cd{0.0, 0.0};
        if (r < nr) {
            const int src = e < xh ? e : X - e;
            const size_t at = (row0 + r) * xh + src;
            xh_cd a = F4[(size_t)(2 * p) * NF + at], b = F4[(size_t)(2 * p + 1) * NF + at];
            if (src == 0 || 2 * src == X) { a.y = 0.0; b.y = 0.0; }
            if (e >= xh) { a.y = -a.y; b.y = -b.y; }
            v = xh_cd{a.x - b.y, a.y + b.x};
        }
        s[l * M + xh_plan_pos(plan, e)] = v;
    }
    __syncthreads();
    xh_plan_exec<double, true>(s, plan, 2 * rpb, tid, nth);
    for (int q = tid; q < nr * X; q += nth) {
        const int r = q / X, e = q - r * X;
        const xh_cd c0 = s[(2 * r) * M + e], c1 = s[(2 * r + 1) * M + e];
        const double v = c0.x, rx = c0.y, ry = c1.x, rz = c1.y;
        double a = v * v;
        a += rx * rx;
        if (SWEEP) { a += rz * rz; a += ry * ry; }
        else { a += ry * ry; a += rz * rz; }
        amp[(row0 + r) * X + e] = sqrt(a);
    }
}

// the low-pass tail (:390-406)
__global__ void __launch_bounds__(256) k_mn_lowpass(xh_cd *__restrict__ F, size_t NF, XhDims d, double freq, double freqL)
{
    const double raised_w = 3.14159265358979323846 / (freqL - freq);
    XH_GRID_LOOP(e, NF) {
        int k, i, j;
        xh_kij(e, d, k, i, j);
        const double un = 1.0 / mn_iu(k, i, j, d);
        if (freqL >= un && un >= freq) {
            if (freqL != freq) {
                const double H = 0.5 * (1 + cos(raised_w * (un - freq)));
                F[e].x *= H; F[e].y *= H;
            }
        } else if (un > freqL) F[e] = xh_cd{0.0, 0.0};
    }
}

// realGaussianFilter's mask (data/fourier_filter.cpp :438 through generateMask :664-676)
__global__ void __launch_bounds__(256) k_mn_gauss(xh_cd *__restrict__ F, size_t NF, XhDims d, double sigma)
{
    const double PI = 3.14159265358979323846;
    XH_GRID_LOOP(e, NF) {
        int k, i, j;
        xh_kij(e, d, k, i, j);
        const double wx = d_digfreq(j, d.X), wy = d_digfreq(i, d.Y), wz = d_digfreq(k, d.Z);
        double sum = wx * wx;
        sum += wy * wy;
        sum += wz * wz;
        const double absw = sqrt(sum);
        const double g = exp(-PI * PI * absw * absw * sigma * sigma);
        F[e].x *= g; F[e].y *= g;
    }
}

// ---------------------------------------------------------------- statistics, select, assign
// statisticsInBinaryMask2 (:424-462, halves) / statisticsInOutBinaryMask2 (:470-508): NS, sumS, sumS2, NN, sumN, sumN2
__global__ void __launch_bounds__(256)
k_mn_stats(const double *__restrict__ ampS, const double *__restrict__ ampN, const int *__restrict__ mask, size_t N, int halves, double *__restrict__ partials)
{
    double acc[6] = {0, 0, 0, 0, 0, 0};
    XH_GRID_LOOP(n, N) {
        const int m = mask[n];
        if (m >= 1) {
            const double a = ampS[n];
            acc[0] += 1; acc[1] += a; acc[2] += a * a;
        }
        if (halves ? m >= 0 : m == 0) {
            const double a = ampN[n];
            acc[3] += 1; acc[4] += a; acc[5] += a * a;
        }
    }
    xh_block_partials(acc, partials);
}

__device__ __forceinline__ bool mn_in_set(int mode, const int *__restrict__ mask, size_t n, double v, double t)
{
    switch (mode) {
        case MN_SET_MASK_EQ0: return mask[n] == 0;
        case MN_SET_MASK_GE0: return mask[n] >= 0;
        case MN_SET_VAL_GT: return v > t;
        default: return !mask || mask[n] != 0;
    }
}

// a double's bits as an unsigned key of the same order (negative values: all bits flipped; others: the sign bit set)
__device__ __forceinline__ unsigned long long mn_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double mn_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// rank: size_t(count * frac) with the count read on the device (d_count), or `rank` itself (d_count null); minus `less`, clamped: see
// the median of post-processing
__global__ void __launch_bounds__(256) k_mn_sel_init(MnSel *sel, const double *d_count, double frac, unsigned long long rank)
{
    for (int i = threadIdx.x; i < MN_BINS; i += 256) sel->hist[i] = 0;
    if (threadIdx.x == 0) {
        sel->prefix = 0;
        sel->bad = 0;
        sel->value = 0;
        if (d_count) {
            const double c = *d_count;
            if (!(c > 0)) sel->bad = 1;
            rank = (unsigned long long)(c * frac);
        }
        sel->krem = rank;
    }
}

// histogram of the w bits below the b resolved ones over the members of the set whose top b bits equal the prefix. A thread counts runs
// of equal digits before it touches LDS: the top digits of an amplitude map are nearly all the same
__global__ void __launch_bounds__(256)
k_mn_sel_pass(const double *__restrict__ vals, const int *__restrict__ mask, size_t N, int mode, double t, int b, int w, MnSel *sel)
{
    __shared__ unsigned int h[MN_BINS];
    for (int i = threadIdx.x; i < MN_BINS; i += 256) h[i] = 0;
    __syncthreads();
    const unsigned long long prefix = sel->prefix;
    const unsigned dmask = (1u << w) - 1;
    unsigned last = 0, cnt = 0;
    XH_GRID_LOOP(n, N) {
        const double v = vals[n];
        if (!mn_in_set(mode, mask, n, v, t)) continue;
        const unsigned long long key = mn_key(v);
        if (b > 0 && (key >> (64 - b)) != prefix) continue;
        const unsigned dg = (unsigned)(key >> (64 - b - w)) & dmask;
        if (cnt && dg == last) ++cnt;
        else {
            if (cnt) atomicAdd(&h[last], cnt);
            last = dg; cnt = 1;
        }
    }
    if (cnt) atomicAdd(&h[last], cnt);
    __syncthreads();
    for (int i = threadIdx.x; i < MN_BINS; i += 256)
        if (h[i]) atomicAdd(&sel->hist[i], h[i]);
}

// one workgroup: the digit the remaining rank falls in extends the prefix; the histogram is left zeroed
__global__ void __launch_bounds__(256) k_mn_sel_step(MnSel *sel, int w)
{
    __shared__ unsigned long long part[256];
    __shared__ int chosen;
    const int t = threadIdx.x, T = 1 << w, per = MN_BINS / 256;
    unsigned long long s = 0;
    for (int i = t * per; i < (t + 1) * per; ++i)
        if (i < T) s += sel->hist[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        unsigned long long krem = sel->krem, acc = 0;
        int c = 0;
        while (c < 256 && acc + part[c] <= krem) acc += part[c++];
        if (c == 256) { sel->bad = 1; chosen = 0; }
        else {
            int i = c * per;
            while (acc + sel->hist[i] <= krem) acc += sel->hist[i++];
            chosen = i;
            sel->krem = krem - acc;
        }
        sel->prefix = (sel->prefix << w) | (unsigned long long)chosen;
    }
    __syncthreads();
    for (int i = t; i < MN_BINS; i += 256) sel->hist[i] = 0;
}

__global__ void k_mn_sel_finish(MnSel *sel) { sel->value = mn_unkey(sel->prefix); }

// setLocalResolutionMap / setLocalResolutionHalfMaps (:518-569): drop is -1 / 0
__global__ void __launch_bounds__(256)
k_mn_assign(const double *__restrict__ amp, int *__restrict__ mask, double *__restrict__ res, size_t N, double thr, double resolution, double resolution_2, int drop)
{
    XH_GRID_LOOP(n, N) {
        int m = mask[n];
        if (m >= 1) {
            if (amp[n] > thr) {
                m = 1;
                res[n] = resolution;
            } else {
                m += 1;
                if (m > 2) {
                    m = drop;
                    res[n] = resolution_2;
                }
            }
            mask[n] = m;
        }
    }
}

// refiningMask :241-255; out[0] counts the voxels kept
__global__ void __launch_bounds__(256) k_mn_refine(const double *__restrict__ amp, int *__restrict__ mask, size_t N, double thr, unsigned long long *__restrict__ out)
{
    unsigned long long c = 0;
    XH_GRID_LOOP(n, N) {
        if (mask[n] >= 1) {
            if (amp[n] < thr) mask[n] = 0;
            else ++c;
        }
    }
    if (c) atomicAdd(out, c);
}

// run :466-475 / :541-550
__global__ void __launch_bounds__(256) k_mn_relabel(const double *__restrict__ res, int *__restrict__ mask, size_t N)
{
    XH_GRID_LOOP(n, N) mask[n] = res[n] == 0 ? 0 : 1;
}

// postProcessingLocalResolutions :270-274 and the values copied at :280-282: out[0] counts >= bound, out[1] counts > bound
__global__ void __launch_bounds__(256) k_mn_post_count(const double *__restrict__ filt, size_t N, double bound, unsigned long long *__restrict__ out)
{
    unsigned long long ge = 0, gt = 0;
    XH_GRID_LOOP(n, N) {
        const double v = filt[n];
        if (v >= bound) ++ge;
        if (v > bound) ++gt;
    }
    if (ge) atomicAdd(out, ge);
    if (gt) atomicAdd(out + 1, gt);
}

// :290-299
__global__ void __launch_bounds__(256) k_mn_post_fill(double *__restrict__ filt, int *__restrict__ mask, size_t N, double last_res, double filling)
{
    XH_GRID_LOOP(n, N) {
        if (filt[n] < last_res) { filt[n] = filling; mask[n] = 0; }
        else mask[n] = 1;
    }
}

// :310-321 into chimera, :327-331 into resmap
__global__ void __launch_bounds__(256)
k_mn_post_out(const double *__restrict__ filt, const double *__restrict__ res, const int *__restrict__ mask, size_t N, double nyquist, double *__restrict__ chimera,
              double *__restrict__ resmap)
{
    XH_GRID_LOOP(n, N) {
        double v = filt[n];
        const int m = mask[n];
        if (m > 0) {
            const double valFilt = v, valRes = res[n];
            if (valFilt > valRes) v = valRes;
            if (valFilt < nyquist) v = valRes;
        }
        chimera[n] = v;
        resmap[n] = m == 0 ? 0.0 : v;
    }
}

double mn_round_idx(double x) { return x > 0 ? (double)(int)(x + 0.5) : (double)(int)(x - 0.5); }

// DIGFREQ2FFT_IDX / FFT_IDX2DIGFREQ (xmippCore xmipp_fft.h)
int mn_freq2idx(double freq, int size)
{
    int idx = (int)mn_round_idx((double)size * freq);
    if (idx < 0) idx += size;
    return idx;
}
double mn_idx2freq(int idx, int size) { return size <= 1 ? 0.0 : (double)(idx <= (size >> 1) ? idx : idx - size) / (double)size; }

}  // namespace

struct xh_mono : XhVolume {
    unsigned grid = 0;
    int nshell = 0, rpb = 1;
    XhBuf FV, FN, F4, V, Nz, ampS, ampN, mask, res, filt, shellPart, shellOut, partials, result, sel, counts;
    XhPinned host;                               // 6 sums, the select's record, 2 counters
    XhEvent ev[2][5], evs[6];
    bool timing = false;
    double ms[MN_NT] = {};
    int32_t radius = 0, radiuslimit = 0;
    int64_t nvox = 0;
    ~xh_mono() { finish(); }
};

namespace {

MnSel *selp(xh_mono *h) { return (MnSel *)h->sel.p; }

// the monogenic amplitude of spectrum F into d_amp: the sweep's form (band, low-pass tail) or monogenicAmplitude_3D_Fourier's. tslot:
// which event row records the stages when timing is on
int mn_amplitude(xh_mono *h, const xh_cd *F, double freq, double freqH, double freqL, bool banded, double *d_amp, int tslot)
{
    hipStream_t st = h->ctx->stream;
    const bool tm = h->timing && tslot >= 0;
    XhEvent *ev = h->ev[tslot < 0 ? 0 : tslot];
    if (tm) XH_HIP(hipEventRecord(ev[0], st));
    if (banded) XH_LAUNCH256(h->ctx, k_mn_split<true>, h->grid, F, cp(h->F4), h->NF, h->d, freq, freqH, 3.14159265358979323846 / (freq - freqH));
    else XH_LAUNCH256(h->ctx, k_mn_split<false>, h->grid, F, cp(h->F4), h->NF, h->d, 0.0, 0.0, 0.0);
    if (tm) XH_HIP(hipEventRecord(ev[1], st));
    XH_TRY(fft3d_yz<true>(h->ctx, cp(h->F4), h->d.Z, h->d.Y, h->d.xh, h->fft.py.plan, h->fft.pz.plan, 4));
    if (tm) XH_HIP(hipEventRecord(ev[2], st));
    {
        const size_t nrows = (size_t)h->d.Z * h->d.Y;
        const size_t smem = ((size_t)h->rpb * 2 * sizeof(xh_cd)) << h->fft.px.plan.logM;
        const unsigned g = (unsigned)((nrows + h->rpb - 1) / h->rpb);
        if (banded)
            hipLaunchKernelGGL(k_mn_rows_amp<true>, dim3(g), dim3(256), smem, st, (const xh_cd *)h->F4.p, d_amp, h->fft.px.plan, nrows, h->NF, h->d.X, h->d.xh, h->rpb);
        else
            hipLaunchKernelGGL(k_mn_rows_amp<false>, dim3(g), dim3(256), smem, st, (const xh_cd *)h->F4.p, d_amp, h->fft.px.plan, nrows, h->NF, h->d.X, h->d.xh, h->rpb);
        XH_LAUNCH_CHECK();
    }
    if (tm) XH_HIP(hipEventRecord(ev[3], st));
    if (banded) {
        XH_TRY(h->fft.r2c(d_amp, cp(h->F4), 1.0 / (double)h->N));
        XH_LAUNCH256(h->ctx, k_mn_lowpass, h->grid, cp(h->F4), h->NF, h->d, freq, freqL);
        XH_TRY(h->fft.c2r(cp(h->F4), d_amp, 1.0));
    }
    if (tm) XH_HIP(hipEventRecord(ev[4], st));
    return XH_OK;
}

int mn_gauss(xh_mono *h, double *d_v, double sigma)
{
    XH_TRY(h->fft.r2c(d_v, cp(h->F4), 1.0 / (double)h->N));
    XH_LAUNCH256(h->ctx, k_mn_gauss, h->grid, cp(h->F4), h->NF, h->d, sigma);
    return h->fft.c2r(cp(h->F4), d_v, 1.0);
}

// the statistics of n values, launched only: result [6] stays on the device
int mn_stats_launch(xh_mono *h, const double *ampS, const double *ampN, const int *mask, size_t n, int halves)
{
    XH_LAUNCH256(h->ctx, k_mn_stats, h->grid, ampS, ampN, mask, n, halves, dp(h->partials));
    XH_LAUNCH256(h->ctx, xh_k_reduce_final, 1, (const double *)h->partials.p, (int)h->grid, 6, dp(h->result));
    return XH_OK;
}

// the select, launched only: d_count (a device double) times frac, or rank
int mn_select_launch(xh_mono *h, const double *vals, const int *mask, size_t n, int mode, double t, const double *d_count, double frac, unsigned long long rank)
{
    MnSel *sel = selp(h);
    XH_LAUNCH256(h->ctx, k_mn_sel_init, 1, sel, d_count, frac, rank);
    for (int b = 0; b < 64;) {
        const int w = std::min(MN_W, 64 - b);
        XH_LAUNCH256(h->ctx, k_mn_sel_pass, h->grid, vals, mask, n, mode, t, b, w, sel);
        XH_LAUNCH256(h->ctx, k_mn_sel_step, 1, sel, w);
        b += w;
    }
    hipLaunchKernelGGL(k_mn_sel_finish, dim3(1), dim3(1), 0, h->ctx->stream, sel);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

// the one wait: sums [6] and the select's record to the host
int mn_fetch(xh_mono *h, double *sums, double *value, bool *bad)
{
    double *hp = h->host.f64();
    XH_HIP(hipMemcpyAsync(hp, h->result.p, sizeof(double) * 6, hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipMemcpyAsync(hp + 8, h->sel.p, offsetof(MnSel, hist), hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    for (int i = 0; i < 6; ++i) sums[i] = hp[i];
    const MnSel *s = (const MnSel *)(hp + 8);
    *value = s->value;
    *bad = s->bad != 0;
    return XH_OK;
}

int mn_counts(xh_mono *h, unsigned long long *out, int n)
{
    unsigned long long *hp = (unsigned long long *)(h->host.f64() + 8 + 8);
    XH_HIP(hipMemcpyAsync(hp, h->counts.p, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    for (int i = 0; i < n; ++i) out[i] = hp[i];
    return XH_OK;
}

void mn_record(const double *s, double thr95, xh_mono_stats *o)
{
    o->NS = s[0]; o->NN = s[3];
    o->sumS = s[1]; o->sumS2 = s[2]; o->sumN = s[4]; o->sumN2 = s[5];
    o->meanS = s[1] / s[0];
    o->meanN = s[4] / s[3];
    o->sdS2 = s[2] / s[0] - o->meanS * o->meanS;
    o->sdN2 = s[5] / s[3] - o->meanN * o->meanN;
    o->thr95 = thr95;
}

int mn_shells(xh_mono *h, const double *d_vol)
{
    XH_LAUNCH256(h->ctx, k_mn_shell_planes, (unsigned)h->d.Z, d_vol, h->d, h->nshell, dp(h->shellPart));
    XH_LAUNCH256(h->ctx, k_mn_shell_final, (unsigned)((3 * h->nshell + 255) / 256), (const double *)h->shellPart.p, h->d.Z, h->nshell, dp(h->shellOut));
    return XH_OK;
}

int mn_time_add(xh_mono *h, hipEvent_t a, hipEvent_t b, int stage)
{
    float ms = 0;
    XH_HIP(hipEventElapsedTime(&ms, a, b));
    h->ms[stage] += ms;
    return XH_OK;
}

}  // namespace

extern "C" {

int xh_mono_icdf_gauss(double p, double *out)
{
    XH_CHECK(out && p > 0 && p < 1, XH_ERR_ARG, "xh_mono_icdf_gauss: p = %g is not inside (0, 1)", p);
    const double q = p < 0.5 ? p : 1 - p;
    const double t = std::sqrt(-2 * std::log(q));
    const double x = t - ((0.010328 * t + 0.802853) * t + 2.515517) / (((0.001308 * t + 0.189269) * t + 1.432788) * t + 1);
    *out = p < 0.5 ? -x : x;
    return XH_OK;
}

int xh_mono_resolution2eval(int32_t *count_res, double step, double *resolution, double *last_resolution, double *freq, double *freqL, int32_t *last_fourier_idx,
                            int32_t volsize, int32_t *continueIter, int32_t *breakIter, double sampling, double maxRes)
{
    XH_CHECK(count_res && resolution && last_resolution && freq && freqL && last_fourier_idx && continueIter && breakIter, XH_ERR_ARG,
             "xh_mono_resolution2eval: null argument");
    *continueIter = 0;
    *breakIter = 0;
    *resolution = maxRes - *count_res * step;
    if (!(*resolution > 0)) {       // deviation: the reference divides by it
        ++*count_res;
        *breakIter = 1;
        return XH_OK;
    }
    *freq = sampling / *resolution;
    ++*count_res;
    const double Nyquist = 2 * sampling;
    const int fourier_idx = mn_freq2idx(*freq, volsize);
    const double aux_frequency = mn_idx2freq(fourier_idx, volsize);
    *freq = aux_frequency;
    if (fourier_idx == *last_fourier_idx) {
        *continueIter = 1;
        return XH_OK;
    }
    *last_fourier_idx = fourier_idx;
    *resolution = sampling / aux_frequency;
    if (*count_res == 0) *last_resolution = *resolution;
    if (*resolution < Nyquist) {
        *breakIter = 1;
        return XH_OK;
    }
    *freqL = sampling / (*resolution + step);
    const int fourier_idx_2 = mn_freq2idx(*freqL, volsize);
    if (fourier_idx_2 == fourier_idx) {
        if (fourier_idx > 0) *freqL = mn_idx2freq(fourier_idx - 1, volsize);
        else *freqL = sampling / (*resolution + step);
    }
    return XH_OK;
}

int xh_mono_cliff_radius(const double *h_sum, const double *h_sum2, const double *h_N, int32_t nshell, int32_t radius, int32_t X, int32_t *radiuslimit)
{
    XH_CHECK(h_sum && h_sum2 && h_N && radiuslimit && nshell >= 1, XH_ERR_ARG, "xh_mono_cliff_radius: bad argument");
    int limit = X / 2;
    double last_std2 = 1e-38;
    for (int rad = radius; rad < limit; rad++) {
        XH_CHECK(rad >= 0 && rad < nshell, XH_ERR_ARG, "xh_mono_cliff_radius: shell %d of %d", rad, nshell);
        const double mean = h_sum[rad] / h_N[rad];
        const double std2 = h_sum2[rad] / h_N[rad] - mean * mean;
        if (std2 / last_std2 < 0.01) {
            limit = rad - 1;
            break;
        }
        last_std2 = std2;
    }
    *radiuslimit = limit;
    return XH_OK;
}

int xh_mono_num_shells(int32_t Z, int32_t Y, int32_t X, int32_t *nshell)
{
    XH_CHECK(nshell && Z >= 1 && Y >= 1 && X >= 1, XH_ERR_ARG, "xh_mono_num_shells: bad argument");
    const long long a = Z / 2, b = Y / 2, c = X / 2;
    *nshell = (int32_t)std::sqrt((double)(a * a + b * b + c * c)) + 2;
    return XH_OK;
}

void xh_mono_defaults(xh_mono_params *p)
{
    if (!p) return;
    p->sampling = 1; p->minRes = 30; p->maxRes = 1; p->freq_step = 0.25; p->significance = 0.95;
    p->gaussian = 0; p->noise_only_in_halves = 0;
}

int xh_mono_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, xh_mono **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_mono_create: null argument");
    XH_CHECK(Z >= 2 && Y >= 2 && X >= 2, XH_ERR_ARG, "xh_mono_create: bad size %d x %d x %d", Z, Y, X);
    XH_CHECK(Z <= 1024 && Y <= 1024 && X <= 1024, XH_ERR_UNSUPPORTED, "xh_mono_create: sizes above 1024 are not supported (%d x %d x %d)", Z, Y, X);
    std::unique_ptr<xh_mono> h(new xh_mono);
    XH_TRY(h->init(ctx, Z, Y, X));
    h->grid = xh_grid256(h->NF, ctx->num_cus, 4);
    const size_t rowBytes = (2 * sizeof(xh_cd)) << h->fft.px.plan.logM;     // the two complex lines of a row
    XH_CHECK(rowBytes <= 64 * 1024, XH_ERR_UNSUPPORTED, "xh_mono_create: a row of %d points does not fit the LDS of the amplitude kernel", X);
    h->rpb = (int)std::max<size_t>(1, std::min<size_t>(8, 32 * 1024 / rowBytes));
    XH_TRY(xh_mono_num_shells(Z, Y, X, &h->nshell));
    const size_t vb = sizeof(double) * h->N, fb = sizeof(xh_cd) * h->NF;
    for (XhBuf *b : {&h->V, &h->Nz, &h->ampS, &h->ampN, &h->res, &h->filt}) XH_TRY(xh_buf_alloc(ctx, *b, vb));
    XH_TRY(xh_buf_alloc(ctx, h->mask, sizeof(int) * h->N));
    XH_TRY(xh_buf_alloc(ctx, h->FV, fb));
    XH_TRY(xh_buf_alloc(ctx, h->FN, fb));
    XH_TRY(xh_buf_alloc(ctx, h->F4, 4 * fb));
    XH_TRY(xh_buf_alloc(ctx, h->shellPart, sizeof(double) * 3 * h->nshell * Z));
    XH_TRY(xh_buf_alloc(ctx, h->shellOut, sizeof(double) * 3 * h->nshell));
    XH_TRY(xh_buf_alloc(ctx, h->partials, sizeof(double) * 6 * h->grid));
    XH_TRY(xh_buf_alloc(ctx, h->result, sizeof(double) * 6));
    XH_TRY(xh_buf_alloc(ctx, h->sel, sizeof(MnSel)));
    XH_TRY(xh_buf_alloc(ctx, h->counts, sizeof(unsigned long long) * 2));
    XH_TRY(xh_pinned_alloc(ctx, h->host, sizeof(double) * 32));
    for (auto &r : h->ev) for (XhEvent &x : r) XH_TRY(xh_event_create(x));
    for (XhEvent &x : h->evs) XH_TRY(xh_event_create(x));
    *out = h.release();
    return XH_OK;
}

int xh_mono_destroy(xh_mono *h)
{
    delete h;
    return XH_OK;
}

int xh_mono_shell_sums(xh_mono *h, const double *d_vol, double *h_sum, double *h_sum2, double *h_N)
{
    XH_CHECK(h && d_vol && h_sum && h_sum2 && h_N, XH_ERR_ARG, "xh_mono_shell_sums: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_TRY(mn_shells(h, d_vol));
    std::vector<double> o(3 * (size_t)h->nshell);
    XH_HIP(hipMemcpyAsync(o.data(), h->shellOut.p, sizeof(double) * o.size(), hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    for (int r = 0; r < h->nshell; ++r) { h_sum[r] = o[r]; h_sum2[r] = o[h->nshell + r]; h_N[r] = o[2 * h->nshell + r]; }
    return XH_OK;
}

int xh_mono_amplitude(xh_mono *h, const double *d_vol, double freq, double freqH, double freqL, int32_t banded, double *d_out)
{
    XH_CHECK(h && d_vol && d_out, XH_ERR_ARG, "xh_mono_amplitude: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_TRY(h->fft.r2c(d_vol, cp(h->FV), 1.0 / (double)h->N));
    XH_TRY(mn_amplitude(h, (const xh_cd *)h->FV.p, freq, freqH, freqL, banded != 0, dp(h->ampS), -1));
    XH_HIP(hipMemcpyAsync(d_out, h->ampS.p, h->ampS.bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
    return XH_OK;
}

int xh_mono_gaussian(xh_mono *h, double *d_vol, double sigma)
{
    XH_CHECK(h && d_vol, XH_ERR_ARG, "xh_mono_gaussian: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    return mn_gauss(h, d_vol, sigma);
}

int xh_mono_statistics(xh_mono *h, const double *d_ampS, const double *d_ampN, const int32_t *d_mask, double significance, xh_mono_stats *out)
{
    XH_CHECK(h && d_ampS && d_mask && out, XH_ERR_ARG, "xh_mono_statistics: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    const int halves = d_ampN ? 1 : 0;
    const double *ampN = d_ampN ? d_ampN : d_ampS;
    XH_TRY(mn_stats_launch(h, d_ampS, ampN, d_mask, h->N, halves));
    XH_TRY(mn_select_launch(h, ampN, d_mask, h->N, halves ? MN_SET_MASK_GE0 : MN_SET_MASK_EQ0, 0.0, dp(h->result) + 3, significance, 0));
    double s[6], thr;
    bool bad;
    XH_TRY(mn_fetch(h, s, &thr, &bad));
    XH_CHECK(s[3] > 0, XH_ERR_ARG, "xh_mono_statistics: the noise set is empty (NN = 0)");
    XH_CHECK(!bad, XH_ERR_ARG, "xh_mono_statistics: rank %g is beyond the noise set of %g voxels", std::floor(s[3] * significance), s[3]);
    mn_record(s, thr, out);
    return XH_OK;
}

int xh_mono_select(xh_mono *h, const double *d_vals, const int32_t *d_mask, size_t n, size_t rank, double *out)
{
    XH_CHECK(h && d_vals && out, XH_ERR_ARG, "xh_mono_select: null argument");
    XH_CHECK(n >= 1 && n <= h->N, XH_ERR_ARG, "xh_mono_select: %zu values (1 .. %zu)", n, h->N);
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_TRY(mn_select_launch(h, d_vals, d_mask, n, MN_SET_ALL, 0.0, nullptr, 0.0, (unsigned long long)rank));
    double *hp = h->host.f64();
    XH_HIP(hipMemcpyAsync(hp + 8, h->sel.p, offsetof(MnSel, hist), hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    const MnSel *s = (const MnSel *)(hp + 8);
    XH_CHECK(!s->bad, XH_ERR_ARG, "xh_mono_select: rank %zu is beyond the set", rank);
    *out = s->value;
    return XH_OK;
}

int xh_mono_assign(xh_mono *h, const double *d_amp, int32_t *d_mask, double *d_res, size_t n, double threshold, double resolution, double resolution_2, int32_t halves)
{
    XH_CHECK(h && d_amp && d_mask && d_res, XH_ERR_ARG, "xh_mono_assign: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_LAUNCH256(h->ctx, k_mn_assign, h->grid, d_amp, (int *)d_mask, d_res, n, threshold, resolution, resolution_2, halves ? 0 : -1);
    return XH_OK;
}

int xh_mono_set_timing(xh_mono *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_mono_set_timing: null handle");
    h->timing = on != 0;
    return XH_OK;
}

int xh_mono_stage_ms(const xh_mono *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_mono_stage_ms: null argument");
    for (int i = 0; i < MN_NT; ++i) h_ms[i] = h->ms[i];
    return XH_OK;
}

int xh_mono_info(const xh_mono *h, int32_t *radius, int32_t *radiuslimit, int64_t *nvoxels, int32_t *nshell)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_mono_info: null handle");
    if (radius) *radius = h->radius;
    if (radiuslimit) *radiuslimit = h->radiuslimit;
    if (nvoxels) *nvoxels = h->nvox;
    if (nshell) *nshell = h->nshell;
    return XH_OK;
}

int xh_mono_run(xh_mono *h, const double *d_vol, const double *d_vol2, const int32_t *d_mask, const int32_t *d_mask_excl, const xh_mono_params *prm,
                xh_mono_step *h_steps, int32_t max_steps, int32_t *n_steps, int32_t *stop, double *d_mean, int32_t *d_refined, double *d_chimera, double *d_resmap)
{
    XH_CHECK(h && d_vol && d_mask && prm && n_steps && stop && d_refined && d_chimera && d_resmap, XH_ERR_ARG, "xh_mono_run: null argument");
    XH_CHECK(!h_steps || max_steps >= 0, XH_ERR_ARG, "xh_mono_run: bad record capacity");
    XH_CHECK(prm->sampling > 0, XH_ERR_ARG, "xh_mono_run: sampling rate %g", prm->sampling);
    XH_CHECK(prm->significance > 0 && prm->significance < 1, XH_ERR_ARG, "xh_mono_run: significance %g is not inside (0, 1)", prm->significance);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const bool halves = d_vol2 != nullptr, noiseOnly = prm->noise_only_in_halves != 0;
    const size_t N = h->N;
    const double invN = 1.0 / (double)N;
    *n_steps = 0;
    *stop = 0;
    for (double &t : h->ms) t = 0;

    // ---- produceSideInfo
    if (halves) {
        XH_LAUNCH256(h->ctx, k_mn_mean_diff, h->grid, d_vol, d_vol2, dp(h->V), dp(h->Nz), N);
        if (d_mean) XH_HIP(hipMemcpyAsync(d_mean, h->V.p, h->V.bytes, hipMemcpyDeviceToDevice, st));
        XH_TRY(h->fft.r2c(dp(h->Nz), cp(h->FN), invN));
    } else XH_HIP(hipMemcpyAsync(h->V.p, d_vol, h->V.bytes, hipMemcpyDeviceToDevice, st));
    XH_HIP(hipMemcpyAsync(h->mask.p, d_mask, h->mask.bytes, hipMemcpyDeviceToDevice, st));
    XH_HIP(hipMemsetAsync(h->counts.p, 0, h->counts.bytes, st));
    XH_LAUNCH256(h->ctx, k_mn_radius, h->grid, (const int *)h->mask.p, h->d, (unsigned long long *)h->counts.p);
    unsigned long long cnt[2];
    XH_TRY(mn_counts(h, cnt, 2));
    XH_CHECK(cnt[1] > 0, XH_ERR_ARG, "xh_mono_run: the mask has no voxel equal to 1");
    h->radius = (int32_t)std::sqrt((double)cnt[0]);
    double NVoxelsOriginalMask = (double)cnt[1];
    {
        XH_TRY(mn_shells(h, dp(h->V)));
        std::vector<double> o(3 * (size_t)h->nshell);
        XH_HIP(hipMemcpyAsync(o.data(), h->shellOut.p, sizeof(double) * o.size(), hipMemcpyDeviceToHost, st));
        XH_HIP(hipStreamSynchronize(st));
        XH_TRY(xh_mono_cliff_radius(o.data(), o.data() + h->nshell, o.data() + 2 * h->nshell, h->nshell, h->radius, h->d.X, &h->radiuslimit));
        double raux = (double)h->radiuslimit - 0.0;      // smoothparam = 0 (:129)
        raux *= raux;
        XH_LAUNCH256(h->ctx, k_mn_cliff_mask, h->grid, ip(h->mask), h->d, raux);
    }
    if (d_mask_excl || (halves && noiseOnly)) XH_LAUNCH256(h->ctx, k_mn_exclude, h->grid, ip(h->mask), (const int *)d_mask_excl, halves ? 1 : 0, noiseOnly ? 1 : 0, N);
    XH_TRY(h->fft.r2c(dp(h->V), cp(h->FV), invN));
    const double freq_step = prm->freq_step < 0.25 ? 0.25 : prm->freq_step;

    // ---- run
    double criticalZ;
    XH_TRY(xh_mono_icdf_gauss(prm->significance, &criticalZ));
    const double maxRes = prm->maxRes, sampling = prm->sampling;
    const double minRes = 2 * sampling;
    double resolution = 0, resolution_2 = 0, last_resolution = maxRes, freq = 0, freqH = 0, freqL = 0;
    double max_meanS = -DBL_MIN;
    const double cut_value = 0.025;
    int32_t count_res = 0, last_fourier_idx = -1;

    if (!noiseOnly) {      // refiningMask
        XH_TRY(mn_amplitude(h, (const xh_cd *)h->FV.p, 0, 0, 0, false, dp(h->ampS), -1));
        XH_TRY(mn_gauss(h, dp(h->ampS), 4));
        XH_TRY(mn_stats_launch(h, dp(h->ampS), dp(h->ampS), ip(h->mask), N, 0));
        XH_TRY(mn_select_launch(h, dp(h->ampS), ip(h->mask), N, MN_SET_MASK_EQ0, 0.0, dp(h->result) + 3, 0.95, 0));
        double s[6], thr;
        bool bad;
        XH_TRY(mn_fetch(h, s, &thr, &bad));
        XH_CHECK(s[3] > 0 && !bad, XH_ERR_ARG, "xh_mono_run: refiningMask: the noise set (mask == 0 inside the noise radius of %d px) is empty", h->radiuslimit);
        XH_HIP(hipMemsetAsync(h->counts.p, 0, h->counts.bytes, st));
        XH_LAUNCH256(h->ctx, k_mn_refine, h->grid, (const double *)h->ampS.p, ip(h->mask), N, thr, (unsigned long long *)h->counts.p);
        XH_TRY(mn_counts(h, cnt, 1));
        XH_CHECK(cnt[0] > 0, XH_ERR_ARG, "xh_mono_run: refiningMask left no voxel in the mask");
        NVoxelsOriginalMask = (double)cnt[0];
    }
    h->nvox = (int64_t)NVoxelsOriginalMask;

    const int32_t volsize = h->d.X;
    std::vector<double> list;
    int iter = 0;
    bool doNextIteration = true;
    XH_HIP(hipMemsetAsync(h->res.p, 0, h->res.bytes, st));
    do {
        int32_t continueIter = 0, breakIter = 0;
        XH_TRY(xh_mono_resolution2eval(&count_res, freq_step, &resolution, &last_resolution, &freq, &freqH, &last_fourier_idx, volsize, &continueIter, &breakIter,
                                       sampling, maxRes));
        if (continueIter) continue;
        if (breakIter) { *stop = XH_MONO_STOP_RANGE; break; }
        list.push_back(resolution);
        resolution_2 = iter < 2 ? list[0] : list[iter - 2];
        freqL = freq + 0.02;
        freqH = freq - 0.02;
        if (freqL >= 0.5) freqL = 0.5;
        if (freqH <= 0.0) freqH = 0.0;
        XH_TRY(mn_amplitude(h, (const xh_cd *)h->FV.p, freq, freqH, freqL, true, dp(h->ampS), 0));
        if (halves) XH_TRY(mn_amplitude(h, (const xh_cd *)h->FN.p, freq, freqH, freqL, true, dp(h->ampN), 1));
        const double *ampN = halves ? dp(h->ampN) : dp(h->ampS);
        if (h->timing) XH_HIP(hipEventRecord(h->evs[0], st));
        XH_TRY(mn_stats_launch(h, dp(h->ampS), ampN, ip(h->mask), N, halves ? 1 : 0));
        if (h->timing) XH_HIP(hipEventRecord(h->evs[1], st));
        XH_TRY(mn_select_launch(h, ampN, ip(h->mask), N, halves ? MN_SET_MASK_GE0 : MN_SET_MASK_EQ0, 0.0, dp(h->result) + 3, prm->significance, 0));
        if (h->timing) XH_HIP(hipEventRecord(h->evs[2], st));
        double s[6], thr95;
        bool bad;
        XH_TRY(mn_fetch(h, s, &thr95, &bad));
        XH_CHECK(s[3] > 0 && !bad, XH_ERR_ARG, "xh_mono_run: the noise set is empty (NN = 0) at resolution %g", resolution);
        xh_mono_step rec;
        std::memset(&rec, 0, sizeof(rec));
        mn_record(s, thr95, &rec.stats);
        rec.resolution = resolution; rec.freq = freq; rec.freqH = freqH; rec.freqL = freqL;
        const double NS = s[0], NN = s[3], meanS = rec.stats.meanS, meanN = rec.stats.meanN, sdS2 = rec.stats.sdS2, sdN2 = rec.stats.sdN2;
        bool leave = false, assigned = false;
        if ((NS / NVoxelsOriginalMask) < cut_value) {
            *stop = XH_MONO_STOP_MASK_DONE;
            doNextIteration = false;
        } else {
            if (NS == 0) { *stop = XH_MONO_STOP_NO_POINTS; leave = true; }
            else {
                const double thresholdNoise = prm->gaussian ? meanN + criticalZ * std::sqrt(sdN2) : thr95;
                rec.threshold = thresholdNoise;
                if (meanS > max_meanS) max_meanS = meanS;
                if (meanS < 0.001 * max_meanS) { *stop = XH_MONO_STOP_LOW_SIGNAL; leave = true; }
                else {
                    if (h->timing) XH_HIP(hipEventRecord(h->evs[3], st));
                    XH_LAUNCH256(h->ctx, k_mn_assign, h->grid, (const double *)h->ampS.p, ip(h->mask), dp(h->res), N, thresholdNoise, resolution, resolution_2,
                                 halves ? 0 : -1);
                    if (h->timing) XH_HIP(hipEventRecord(h->evs[4], st));
                    assigned = true;
                    const double z = (meanS - meanN) / std::sqrt(sdS2 / NS + sdN2 / NN);
                    rec.z = z;
                    if (z < criticalZ) { *stop = XH_MONO_STOP_ZTEST; doNextIteration = false; }
                    if (doNextIteration && resolution < minRes) { *stop = XH_MONO_STOP_MIN_RES; doNextIteration = false; }
                }
            }
        }
        rec.max_meanS = max_meanS;
        rec.assigned = assigned ? 1 : 0;
        if (h_steps && *n_steps < max_steps) h_steps[*n_steps] = rec;
        ++*n_steps;
        if (h->timing) {
            XH_HIP(hipEventSynchronize(assigned ? h->evs[4] : h->evs[2]));
            for (int m = 0; m < (halves ? 2 : 1); ++m)
                for (int q = 0; q < 4; ++q) XH_TRY(mn_time_add(h, h->ev[m][q], h->ev[m][q + 1], MN_T_SPLIT + q));
            XH_TRY(mn_time_add(h, h->evs[0], h->evs[1], MN_T_STATS));
            XH_TRY(mn_time_add(h, h->evs[1], h->evs[2], MN_T_SELECT));
            if (assigned) XH_TRY(mn_time_add(h, h->evs[3], h->evs[4], MN_T_ASSIGN));
        }
        if (leave) break;
        iter++;
        last_resolution = resolution;
    } while (doNextIteration);
    XH_LAUNCH256(h->ctx, k_mn_relabel, h->grid, (const double *)h->res.p, ip(h->mask), N);

    // ---- postProcessingLocalResolutions
    XH_CHECK(!list.empty(), XH_ERR_STATE, "xh_mono_run: no frequency was evaluated (maxRes %g, sampling %g)", maxRes, sampling);
    XH_HIP(hipMemcpyAsync(h->filt.p, h->res.p, h->res.bytes, hipMemcpyDeviceToDevice, st));
    double last_res = list[list.size() - 1];
    last_res = last_res - 0.001;
    const double Nyquist = 2 * sampling;
    XH_HIP(hipMemsetAsync(h->counts.p, 0, h->counts.bytes, st));
    XH_LAUNCH256(h->ctx, k_mn_post_count, h->grid, (const double *)h->filt.p, N, last_res, (unsigned long long *)h->counts.p);
    XH_TRY(mn_counts(h, cnt, 2));
    XH_CHECK(cnt[0] > 0, XH_ERR_STATE, "xh_mono_run: no voxel has a resolution at or above %g", last_res);
    double filling_value = 0;
    {
        const unsigned long long rank = (unsigned long long)(int)(0.5 * (double)cnt[0]), zeros = cnt[0] - cnt[1];
        if (rank >= zeros) {
            XH_TRY(mn_select_launch(h, (const double *)h->filt.p, nullptr, N, MN_SET_VAL_GT, last_res, nullptr, 0.0, rank - zeros));
            double s[6];
            bool bad;
            XH_TRY(mn_fetch(h, s, &filling_value, &bad));
            XH_CHECK(!bad, XH_ERR_STATE, "xh_mono_run: the median's rank is beyond its set");
        }
    }
    last_res = list[list.size() - 1];
    XH_LAUNCH256(h->ctx, k_mn_post_fill, h->grid, dp(h->filt), ip(h->mask), N, last_res, filling_value);
    XH_HIP(hipMemcpyAsync(d_refined, h->mask.p, h->mask.bytes, hipMemcpyDeviceToDevice, st));
    XH_TRY(mn_gauss(h, dp(h->filt), 3));
    XH_LAUNCH256(h->ctx, k_mn_post_out, h->grid, (const double *)h->filt.p, (const double *)h->res.p, (const int *)h->mask.p, N, Nyquist, d_chimera, d_resmap);
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

}  // extern "C"
