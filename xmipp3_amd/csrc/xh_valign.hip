// xh_valign.hip -- the device side of xmipp_volume_align (reconstruction/volume_align_prog.cpp, ProgAlignVolumes; the reference runs one
// fitness per trial on the CPU, serially: applyGeometry(LINEAR) of V2 into Vaux, then correlationIndex or rms against V1), fp64, no FMA
// contraction: the source coordinates feed comparisons (the wrap / outside thresholds, the (int) of the taps).
//
//   the fit      a workgroup owns an 8 x 8 x 4 brick of voxels and a tile of VA_TILE trials of the batch. It loads its V1 and mask values
//                once; for every trial it forms the source point Ainv (x, y, z, 1) directly, tests it per axis (xh_applygeo.h), interpolates
//                V2 by the trilinear rule, applies y greyScale + greyShift where the reference does, and over the masked voxels adds
//                COVARIANCE: sum y, sum y^2, sum (x - mean_x) y; LEAST_SQUARES: sum (x - y)^2. The workgroup's sums go through the fixed
//                tree (xh_reduce.h) to partials [trial][brick][k]. No Vaux volume exists.
//   the finish   one workgroup per trial: thread t adds the partials of bricks t, t + 256, .. in increasing order, the tree adds the 256
//                sums, thread 0 finishes: COVARIANCE -(Sxy - mean_y S0) / ((stddev_x stddev_y) n), 0 where a deviation is below 1e-6;
//                LEAST_SQUARES sqrt(sum / n), 0 for n = 0. mean_x, stddev_x, n and S0 = sum (x - mean_x) are formed once by set_volumes
//                on the host in raster order (compensated sums), with computeAvgStdev's integer N / (N - 1); xh_corr.h.
//   the choice   the first minimum in trial order (strict <, volume_align_prog.cpp:388), carried from batch to batch on the device.
//   apply        the materialised applyTransformation of V2 (:56-97) for --apply.
//
// Nothing above depends on how the trials are cut into batches: a trial's partials depend on the brick grid alone, its finish on the
// number of bricks alone, and the choice takes the lower index among equal fits: any capacity gives the same bytes.
// The reference makes two passes over Vaux (mean_y first, then sum (x - mean_x)(y - mean_y)); this file uses
// sum (x - mean_x)(y - mean_y) = sum (x - mean_x) y - mean_y sum (x - mean_x) and sum (y - mean_y)^2 = sum y^2 - n mean_y^2 in one pass
// (the second is computeAvgStdev's own form). The rounding difference is what the tests' bound is derived from.
#include "xh_applygeo.h"
#include "xh_corr.h"
#include "xh_reduce.h"
#include <cmath>
#include <memory>
#include <vector>

namespace {

constexpr int VA_TILE = 8;                       // trials of one workgroup
constexpr size_t VA_PARTIAL_BYTES = (size_t)1 << 29;   // the partial sums of one batch hold at most this much
enum { VA_COVARIANCE = 1, VA_LEAST_SQUARES = 2 };      // the reference's #defines
enum { VA_T_GATHER = 0, VA_T_FINISH, VA_T_SELECT, VA_NT };

// what the kernels read of a trial: rows (x', y', z') of the inverse of A with its translation, the grey values, isIdentity
struct VaTrial { double a[12]; double greyScale, greyShift, ident, pad; };
typedef XhCorrStats VaStats;                     // n, mean_x, stddev_x, S0 (xh_corr.h, shared with xh_fsym.hip)
struct VaBest { double fit; long long index; };

// Vaux at voxel n = (k, i, j) of trial T: applyGeometry(LINEAR, Vaux, V2, A, IS_NOT_INV, wrap) with outside value 0, then the grey values
template <bool WRAP>
__device__ __forceinline__ double va_sample(const double *__restrict__ V2, XhDims d, const VaTrial &T, double x, double y, double z, size_t n)
{
    double v;
    if (T.ident != 0) v = V2[n];
    else {
        double xp = x * T.a[0] + y * T.a[1] + z * T.a[2] + T.a[3];
        double yp = x * T.a[4] + y * T.a[5] + z * T.a[6] + T.a[7];
        double zp = x * T.a[8] + y * T.a[9] + z * T.a[10] + T.a[11];
        bool outsideHit = sy_axis<WRAP>(xp, d.X);
        outsideHit = sy_axis<WRAP>(yp, d.Y) || outsideHit;
        outsideHit = sy_axis<WRAP>(zp, d.Z) || outsideHit;
        v = outsideHit ? 0.0 : sy_interp3<1, WRAP>(V2, d, xp, yp, zp);
    }
    if (T.greyScale != 1 || T.greyShift != 0) v = v * T.greyScale + T.greyShift;
    return v;
}

// grid (bricks, tiles of trials). NK sums per trial: 3 (COVARIANCE) or 1 (LEAST_SQUARES); partials [m][nbricks][NK]
template <int NK, bool WRAP>
__global__ void __launch_bounds__(256)
k_va_fit(const double *__restrict__ V1, const double *__restrict__ V2, const int *__restrict__ mask, const VaTrial *__restrict__ trials, int m,
         XhDims d, int nbx, int nby, double mean_x, double *__restrict__ partials)
{
    __shared__ double red[NK][256];
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int j = bx * 8 + (threadIdx.x & 7), i = by * 8 + ((threadIdx.x >> 3) & 7), k = bz * 4 + (threadIdx.x >> 6);
    const bool inside = j < d.X && i < d.Y && k < d.Z;
    const size_t n = inside ? ((size_t)k * d.Y + i) * d.X + j : 0;
    const bool live = inside && (mask == nullptr || mask[n] != 0);
    const double x1 = live ? V1[n] : 0.0;
    const double x = j - d.X / 2, y = i - d.Y / 2, z = k - d.Z / 2;
    const int t0 = blockIdx.y * VA_TILE, t1 = min(t0 + VA_TILE, m);
    for (int t = t0; t < t1; ++t) {
        double v[NK];
        for (int c = 0; c < NK; ++c) v[c] = 0.0;
        if (live) {
            const double yv = va_sample<WRAP>(V2, d, trials[t], x, y, z, n);
            if constexpr (NK == 3) {
                v[0] = yv;
                v[1] = yv * yv;
                v[2] = (x1 - mean_x) * yv;
            } else {
                const double diff = x1 - yv;
                v[0] = diff * diff;
            }
        }
        xh_tree256(red, v);               // its first barrier comes after every thread's read of red[c][0] below: thread 0 alone reads it
        if (threadIdx.x == 0) {
            double *o = partials + ((size_t)t * gridDim.x + b) * NK;
            for (int c = 0; c < NK; ++c) o[c] = red[c][0];
        }
    }
}

// one workgroup per trial: partials [m][nbricks][NK] -> fit [m]
template <int NK>
__global__ void __launch_bounds__(256) k_va_finish(const double *__restrict__ partials, int nbricks, VaStats S, double *__restrict__ fit)
{
    __shared__ double red[NK][256];
    xh_brick_totals<NK>(partials + (size_t)blockIdx.x * nbricks * NK, nbricks, red);
    if (threadIdx.x != 0) return;
    double f = 0.0;
    if constexpr (NK == 3) {
        f = -xh_corr_index(red[0][0], red[1][0], red[2][0], S);
    } else
        f = S.n != 0 ? sqrt(red[0][0] / S.n) : 0.0;
    fit[blockIdx.x] = f;
}

// one workgroup: the first minimum of fit [m] (trial base + t), against the best of the batches before unless first
__global__ void __launch_bounds__(256) k_va_select(const double *__restrict__ fit, int m, long long base, int first, VaBest *__restrict__ best)
{
    __shared__ double sf[256];
    __shared__ int si[256];
    const int per = (m + 255) / 256, a = threadIdx.x * per, e = min(a + per, m);
    double bf = 0;
    int bi = -1;
    for (int t = a; t < e; ++t)
        if (bi < 0 || fit[t] < bf) { bf = fit[t]; bi = t; }
    sf[threadIdx.x] = bf;
    si[threadIdx.x] = bi;
    __syncthreads();
    // the chunks are in trial order: the lower thread keeps its own on a tie
    for (int s = 1; s < 256; s <<= 1) {
        if ((threadIdx.x & (2 * s - 1)) == 0) {
            const int o = threadIdx.x + s;
            if (si[o] >= 0 && (si[threadIdx.x] < 0 || sf[o] < sf[threadIdx.x])) { sf[threadIdx.x] = sf[o]; si[threadIdx.x] = si[o]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && si[0] >= 0 && (first || sf[0] < best->fit)) {
        best->fit = sf[0];
        best->index = base + si[0];
    }
}

template <bool WRAP>
__global__ void __launch_bounds__(256)
k_va_apply(const double *__restrict__ V2, const VaTrial *__restrict__ trial, XhDims d, int nbx, int nby, double *__restrict__ out)
{
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int j = bx * 8 + (threadIdx.x & 7), i = by * 8 + ((threadIdx.x >> 3) & 7), k = bz * 4 + (threadIdx.x >> 6);
    if (j >= d.X || i >= d.Y || k >= d.Z) return;
    const size_t n = ((size_t)k * d.Y + i) * d.X + j;
    out[n] = va_sample<WRAP>(V2, d, trial[0], (double)(j - d.X / 2), (double)(i - d.Y / 2), (double)(k - d.Z / 2), n);
}

// ---------------------------------------------------------------------------------------------------------------- host helpers
// C = A B for 4 x 4, every entry summed from 0 over k in order (xmippCore's Matrix2D product)
void va_mul4(const double *A, const double *B, double *C)
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += A[i * 4 + k] * B[k * 4 + j];
            C[i * 4 + j] = s;
        }
}

// applyTransformation's A (volume_align_prog.cpp:61-91), its inverse and isIdentity. The inverse of the affine 4 x 4: the cofactor inverse
// of the 3 x 3 block, -Rinv t, the last row kept (xmippCore's own 4 x 4 inv() is not in the reference tree: INTEGRATION.md)
void va_matrix(const double *p, double *A, double *Ainv, bool *ident)
{
    const double flip = p[0], rot = p[3], tilt = p[4], psi = p[5], scale = p[6];
    double rz = p[7];
    const double ry = p[8], rx = p[9];
    if (flip < 0) {
        rz *= -1;
        rz += 1;
    }
    double E[9];
    xh_fp_euler(rot, tilt, psi, E);
    double M[16] = {E[0], E[1], E[2], 0, E[3], E[4], E[5], 0, E[6], E[7], E[8], 0, 0, 0, 0, 1};
    for (int i = 0; i < 4; ++i) M[i * 4 + 2] *= flip;
    const double T[16] = {1, 0, 0, rx, 0, 1, 0, ry, 0, 0, 1, rz, 0, 0, 0, 1};
    const double S[16] = {scale, 0, 0, 0, 0, scale, 0, 0, 0, 0, scale, 0, 0, 0, 0, 1};
    double MT[16];
    va_mul4(M, T, MT);
    va_mul4(MT, S, A);
    bool id = true;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            if (std::fabs(A[r * 4 + c] - (r == c ? 1.0 : 0.0)) > SY_ACC) id = false;
    *ident = id;
    const double R[9] = {A[0], A[1], A[2], A[4], A[5], A[6], A[8], A[9], A[10]};
    double Ri[9];
    sy_inv3x3(R, Ri);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Ainv[r * 4 + c] = Ri[r * 3 + c];
        Ainv[r * 4 + 3] = -(Ri[r * 3 + 0] * A[3] + Ri[r * 3 + 1] * A[7] + Ri[r * 3 + 2] * A[11]);
    }
    Ainv[12] = 0; Ainv[13] = 0; Ainv[14] = 0; Ainv[15] = 1;
}

int va_make_trial(const char *who, const double *p, VaTrial &T)
{
    for (int c = 0; c < 10; ++c) XH_CHECK(std::isfinite(p[c]), XH_ERR_ARG, "%s: entry %d of a trial is not finite", who, c);
    double A[16], Ai[16];
    bool ident;
    va_matrix(p, A, Ai, &ident);
    for (int c = 0; c < 12; ++c) {
        XH_CHECK(std::isfinite(Ai[c]) && std::fabs(Ai[c]) <= 1e6, XH_ERR_ARG, "%s: the matrix of a trial is singular (scale %g, flip %g; inverse entry %g)", who, p[6], p[0], Ai[c]);
        T.a[c] = Ai[c];
    }
    T.greyScale = p[1];
    T.greyShift = p[2];
    T.ident = ident ? 1.0 : 0.0;
    T.pad = 0;
    return XH_OK;
}

}  // namespace

struct xh_valign {
    xh_ctx *ctx = nullptr;
    XhDims d = {};
    size_t N = 0;
    int nbx = 0, nby = 0, nbz = 0, nbricks = 0, capacity = 0, batch = 0;
    bool loaded = false, masked = false;
    VaStats stats = {};
    XhBuf V1, V2, mask, trials, partials, fit, best, one;
    XhLapTimer<VA_NT> tm;
    void finish()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    ~xh_valign() { finish(); }
};

namespace {

template <int NK, bool WRAP> int va_launch(xh_valign *h, int m)
{
    const dim3 grid((unsigned)h->nbricks, (unsigned)((m + VA_TILE - 1) / VA_TILE));
    hipLaunchKernelGGL((k_va_fit<NK, WRAP>), grid, dim3(256), 0, h->ctx->stream, (const double *)h->V1.p, (const double *)h->V2.p,
                       h->masked ? (const int *)h->mask.p : (const int *)nullptr, (const VaTrial *)h->trials.p, m, h->d, h->nbx, h->nby, h->stats.mean_x,
                       dp(h->partials));
    XH_LAUNCH_CHECK();
    XH_TRY(h->tm.lap(VA_T_GATHER));
    XH_LAUNCH256(h->ctx, (k_va_finish<NK>), (unsigned)m, (const double *)h->partials.p, h->nbricks, h->stats, dp(h->fit));
    return h->tm.lap(VA_T_FINISH);
}

// the fits of all m trials, batch by batch; select: the running first minimum in h->best
int va_run(xh_valign *h, const char *who, const double *h_p, int64_t m, int method, bool wrap, bool select, double *h_fit)
{
    XH_CHECK(h->loaded, XH_ERR_STATE, "%s: no volumes (xh_valign_set_volumes comes first)", who);
    XH_CHECK(method == VA_COVARIANCE || method == VA_LEAST_SQUARES, XH_ERR_ARG, "%s: method %d (1 covariance, 2 least squares)", who, method);
    XH_CHECK(m >= 0 && m <= ((int64_t)1 << 40), XH_ERR_ARG, "%s: %lld trials", who, (long long)m);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    std::vector<VaTrial> T((size_t)std::min<int64_t>(m, h->batch));
    for (int64_t t0 = 0; t0 < m; t0 += h->batch) {
        const int mb = (int)std::min<int64_t>(h->batch, m - t0);
        for (int t = 0; t < mb; ++t) XH_TRY(va_make_trial(who, h_p + 10 * (size_t)(t0 + t), T[t]));
        XH_HIP(hipMemcpyAsync(h->trials.p, T.data(), sizeof(VaTrial) * mb, hipMemcpyHostToDevice, st));
        XH_HIP(hipStreamSynchronize(st));                 // T is reused by the next batch
        XH_TRY(h->tm.start());
        if (method == VA_COVARIANCE) XH_TRY(wrap ? (va_launch<3, true>(h, mb)) : (va_launch<3, false>(h, mb)));
        else XH_TRY(wrap ? (va_launch<1, true>(h, mb)) : (va_launch<1, false>(h, mb)));
        if (select) {
            XH_LAUNCH256(h->ctx, k_va_select, 1, (const double *)h->fit.p, mb, (long long)t0, t0 == 0 ? 1 : 0, (VaBest *)h->best.p);
            XH_TRY(h->tm.lap(VA_T_SELECT));
        }
        if (h_fit) XH_HIP(hipMemcpyAsync(h_fit + t0, h->fit.p, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
    }
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

}  // namespace

extern "C" {

int xh_valign_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t capacity, xh_valign **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_valign_create: null argument");
    XH_CHECK(Z >= 2 && Y >= 2 && X >= 2, XH_ERR_ARG, "xh_valign_create: bad size %d x %d x %d", Z, Y, X);
    XH_CHECK(Z <= 1024 && Y <= 1024 && X <= 1024, XH_ERR_UNSUPPORTED, "xh_valign_create: sizes above 1024 are not supported (%d x %d x %d)", Z, Y, X);
    XH_CHECK(capacity >= 1 && capacity <= (1 << 20), XH_ERR_ARG, "xh_valign_create: capacity %d (1 .. %d)", capacity, 1 << 20);
    std::unique_ptr<xh_valign> h(new xh_valign);
    XH_HIP(hipSetDevice(ctx->device));
    h->ctx = ctx;
    h->d = XhDims{Z, Y, X, X / 2 + 1};
    h->N = (size_t)Z * Y * X;
    h->nbx = (X + 7) / 8;
    h->nby = (Y + 7) / 8;
    h->nbz = (Z + 3) / 4;
    h->nbricks = h->nbx * h->nby * h->nbz;
    h->capacity = capacity;
    // trials of one launch: the capacity, less where their partial sums would pass VA_PARTIAL_BYTES (the results do not depend on it);
    // 65535 tiles is the grid's y limit
    const size_t perTrial = sizeof(double) * 3 * (size_t)h->nbricks;
    h->batch = (int)std::max<size_t>(1, std::min<size_t>({(size_t)capacity, VA_PARTIAL_BYTES / perTrial, (size_t)65535 * VA_TILE}));
    XH_TRY(xh_buf_alloc(ctx, h->V1, sizeof(double) * h->N));
    XH_TRY(xh_buf_alloc(ctx, h->V2, sizeof(double) * h->N));
    XH_TRY(xh_buf_alloc(ctx, h->trials, sizeof(VaTrial) * h->batch));
    XH_TRY(xh_buf_alloc(ctx, h->one, sizeof(VaTrial)));
    XH_TRY(xh_buf_alloc(ctx, h->partials, perTrial * h->batch));
    XH_TRY(xh_buf_alloc(ctx, h->fit, sizeof(double) * h->batch));
    XH_TRY(xh_buf_alloc(ctx, h->best, sizeof(VaBest)));
    XH_TRY(h->tm.create(ctx));
    *out = h.release();
    return XH_OK;
}

int xh_valign_destroy(xh_valign *h)
{
    delete h;
    return XH_OK;
}

int xh_valign_set_volumes(xh_valign *h, const double *h_V1, const double *h_V2, const int32_t *h_mask)
{
    XH_CHECK(h && h_V1 && h_V2, XH_ERR_ARG, "xh_valign_set_volumes: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    h->loaded = false;
    // what does not depend on the trial, in raster order: computeAvgStdev within the mask, then sum (x - mean_x)
    VaStats S;
    XH_TRY(xh_corr_stats("xh_valign_set_volumes", "the first volume", h_V1, h_mask, h->N, S));
    h->stats = S;
    XH_HIP(hipMemcpyAsync(h->V1.p, h_V1, sizeof(double) * h->N, hipMemcpyHostToDevice, st));
    XH_HIP(hipMemcpyAsync(h->V2.p, h_V2, sizeof(double) * h->N, hipMemcpyHostToDevice, st));
    h->masked = h_mask != nullptr;
    if (h_mask) {
        XH_TRY(xh_buf_reserve(h->ctx, h->mask, sizeof(int32_t) * h->N));
        XH_HIP(hipMemcpyAsync(h->mask.p, h_mask, sizeof(int32_t) * h->N, hipMemcpyHostToDevice, st));
    }
    XH_HIP(hipStreamSynchronize(st));
    h->loaded = true;
    return XH_OK;
}

int xh_valign_stats(const xh_valign *h, double *h_stats)
{
    XH_CHECK(h && h_stats, XH_ERR_ARG, "xh_valign_stats: null argument");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_valign_stats: no volumes");
    h_stats[0] = h->stats.n; h_stats[1] = h->stats.mean_x; h_stats[2] = h->stats.stddev_x; h_stats[3] = h->stats.S0;
    return XH_OK;
}

int xh_valign_matrix(const double *h_p, double *h_A, double *h_Ainv, int32_t *ident)
{
    XH_CHECK(h_p && h_A && h_Ainv && ident, XH_ERR_ARG, "xh_valign_matrix: null argument");
    bool id;
    va_matrix(h_p, h_A, h_Ainv, &id);
    *ident = id ? 1 : 0;
    return XH_OK;
}

int xh_valign_trials(const double *h_ranges, int32_t consider_mirror, int64_t limit, double *h_p, int64_t *count, int64_t *times)
{
    XH_CHECK(h_ranges && count, XH_ERR_ARG, "xh_valign_trials: null argument");
    // grey_scale, grey_shift, rot, tilt, psi, scale, z, y, x: (first, last, step), a zero step set to 1 (readParams :257-274)
    double lo[9], hi[9], step[9];
    for (int a = 0; a < 9; ++a) {
        lo[a] = h_ranges[3 * a];
        hi[a] = h_ranges[3 * a + 1];
        step[a] = h_ranges[3 * a + 2] == 0 ? 1 : h_ranges[3 * a + 2];
        XH_CHECK(std::isfinite(lo[a]) && std::isfinite(hi[a]) && std::isfinite(step[a]), XH_ERR_ARG, "xh_valign_trials: range %d is not finite", a);
        // the reference's loop `v <= last; v += step` never ends for these
        XH_CHECK(!(lo[a] <= hi[a] && (step[a] < 0 || lo[a] + step[a] == lo[a] || hi[a] + step[a] == hi[a])), XH_ERR_ARG,
                 "xh_valign_trials: range %d (%g .. %g by %g) never ends", a, lo[a], hi[a], step[a]);
    }
    if (times) {
        // the progress bar's count (:330-352), which is not the loops' trip count
        int64_t t = consider_mirror ? 2 : 1;
        for (int a = 0; a < 9; ++a)
            if (lo[a] != hi[a]) t = (int32_t)(t * (int64_t)std::floor(1 + std::fmin(std::fmax((hi[a] - lo[a]) / step[a], -1e9), 1e9)));   // an int in the reference
        *times = t;
    }
    int64_t c = 0;
    double v[9];
    for (int mirror = 0; mirror <= (consider_mirror ? 1 : 0); ++mirror)
        for (v[0] = lo[0]; v[0] <= hi[0]; v[0] += step[0])
            for (v[1] = lo[1]; v[1] <= hi[1]; v[1] += step[1])
                for (v[2] = lo[2]; v[2] <= hi[2]; v[2] += step[2])
                    for (v[3] = lo[3]; v[3] <= hi[3]; v[3] += step[3])
                        for (v[4] = lo[4]; v[4] <= hi[4]; v[4] += step[4])
                            for (v[5] = lo[5]; v[5] <= hi[5]; v[5] += step[5])
                                for (v[6] = lo[6]; v[6] <= hi[6]; v[6] += step[6])
                                    for (v[7] = lo[7]; v[7] <= hi[7]; v[7] += step[7])
                                        for (v[8] = lo[8]; v[8] <= hi[8]; v[8] += step[8]) {
                                            XH_CHECK(c < limit, XH_ERR_UNSUPPORTED, "xh_valign_trials: more than %lld trials", (long long)limit);
                                            if (h_p) {
                                                double *p = h_p + 10 * (size_t)c;
                                                p[0] = mirror ? -1.0 : 1.0;
                                                for (int a = 0; a < 9; ++a) p[1 + a] = v[a];
                                            }
                                            ++c;
                                        }
    *count = c;
    return XH_OK;
}

int xh_valign_fit(xh_valign *h, const double *h_p, int64_t m, int32_t method, int32_t wrap, double *h_fit)
{
    XH_CHECK(h && (h_p || m == 0) && (h_fit || m == 0), XH_ERR_ARG, "xh_valign_fit: null argument");
    return va_run(h, "xh_valign_fit", h_p, m, method, wrap != 0, false, h_fit);
}

int xh_valign_search(xh_valign *h, const double *h_p, int64_t m, int32_t method, int32_t wrap, int64_t *best_index, double *best_fit, double *h_fit)
{
    XH_CHECK(h && h_p && best_index && best_fit, XH_ERR_ARG, "xh_valign_search: null argument");
    XH_CHECK(m >= 1, XH_ERR_ARG, "xh_valign_search: no trials");
    XH_TRY(va_run(h, "xh_valign_search", h_p, m, method, wrap != 0, true, h_fit));
    VaBest b;
    XH_HIP(hipMemcpy(&b, h->best.p, sizeof(VaBest), hipMemcpyDeviceToHost));
    *best_index = b.index;
    *best_fit = b.fit;
    return XH_OK;
}

int xh_valign_apply(xh_valign *h, const double *h_p, int32_t wrap, double *d_out)
{
    XH_CHECK(h && h_p && d_out, XH_ERR_ARG, "xh_valign_apply: null argument");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_valign_apply: no volumes (xh_valign_set_volumes comes first)");
    XH_CHECK(d_out != h->V2.p && d_out != h->V1.p, XH_ERR_ARG, "xh_valign_apply: the output may not be a volume of the handle");
    VaTrial T;
    XH_TRY(va_make_trial("xh_valign_apply", h_p, T));
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(h->one.p, &T, sizeof(VaTrial), hipMemcpyHostToDevice, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    if (wrap) XH_LAUNCH256(h->ctx, (k_va_apply<true>), (unsigned)h->nbricks, (const double *)h->V2.p, (const VaTrial *)h->one.p, h->d, h->nbx, h->nby, d_out);
    else XH_LAUNCH256(h->ctx, (k_va_apply<false>), (unsigned)h->nbricks, (const double *)h->V2.p, (const VaTrial *)h->one.p, h->d, h->nbx, h->nby, d_out);
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

int xh_valign_set_timing(xh_valign *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_valign_set_timing: null handle");
    h->tm.set(on != 0);
    return XH_OK;
}

int xh_valign_stage_ms(const xh_valign *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_valign_stage_ms: null argument");
    h->tm.read(h_ms);
    return XH_OK;
}

}  // extern "C"
