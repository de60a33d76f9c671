// xh_fsym.hip -- the device side of xmipp_volume_find_symmetry (reconstruction/volume_find_symmetry.cpp, ProgVolumeFindSymmetry; the
// reference runs one evaluateSymmetry per trial on CPU threads and allocates two volumes for each: volume_sym and volume_aux), fp64, no FMA
// contraction: the source coordinates feed comparisons (the outside thresholds, the (int), floor and ceil of the taps, kp against zFirst /
// zLast).
//
//   the axis fit     --sym rot <n> (:364-391). A workgroup owns an 8 x 8 x 4 brick of voxels and a tile of FS_TILE trials of the batch. A
//                    thread reads its voxel of V and its mask value once; for every trial it forms
//                    y = V + sum_{n = 1}^{rot_sym - 1} applyGeometry(V, rotation3DMatrix(360.0 / rot_sym * n, axis)) in a register, in
//                    that order, with the per-voxel applyGeometry of xh_applygeo.h (LINEAR from V, BSPLINE3 from the coefficients,
//                    DONT_WRAP, outside value 0), and over the masked voxels adds sum y, sum y^2, sum (x - mean_x) y through the fixed
//                    tree (xh_reduce.h) to partials [trial][brick][3]. The rot_sym - 1 inverse matrices of a trial are read with an
//                    index that is uniform over the workgroup, so they arrive through the scalar cache, not per lane.
//   the helical fit  --sym helical | helicalDihedral (:392-417). Same ownership. rot = atan2(i, j) and rho of a voxel are formed once and
//                    serve every trial; per trial the loop of symmetry_Helical runs as written (xh_helix.h: l0, Llength + 1 terms, the
//                    edge weights with zHelical2, the Cn copies, the dihedral copies at (jp, -ip, -kp), finalValue / L). A voxel outside
//                    the mask contributes nothing: the reference leaves Vout 0 there and correlationIndex skips it.
//   the finish       one workgroup per trial: the bricks' partials to totals in the order xh_valign.hip uses (xh_corr.h), then
//                    correlationIndex in its one-pass form. What depends on V alone (n, mean, deviation, sum (x - mean_x)) is formed once
//                    on the host by set_volume, for the helix again under the mask clipped to [zFirst, zLast] (:280-288).
//   the choice       the first correlation strictly above the running best in trial order, the best started at 0 (:167, :188), carried
//                    from launch to launch on the device. With no correlation above 0 there is no winner: the caller answers 0, 0.
//   No volume_sym or volume_aux is stored; xh_fsym_axis_volume and xh_fsym_helical_volume materialise one trial's for the tests.
//
// Nothing depends on how the trials are cut into launches: a trial's partials depend on the brick grid alone, its finish on the number of
// bricks alone, and the choice takes the lower index among equal correlations: any capacity gives the same bytes.
// Kept as written: the 0 start of the best and corr > best; the gate's 1e38 (a correlation of -1e38 in the map, set on the host without a
// launch, never chosen); Llength + 1 terms and the edge weights; finalValue / L even where L is 0 (a NaN, which compares false and never
// wins); the (int) truncation of the linear taps.
// Deviations: a source coordinate is x A00 + y A01 + z A02, not A00 added along the row (the one DESIGN 5p, 5q, 5r have). A corner of
// the helix's interpolation whose weight is exactly 0 is not evaluated (xh_helix.h); the reference evaluates it and multiplies by 0.
// Not in the reference tree (xmippCore), restated here: rotation3DMatrix(ang, axis) as the rotation by ang about the unit axis with the
// sense of rotation3DMatrix(ang, 'Z') (for the axis z: [c s 0; -s c 0; 0 0 1]). The sense cannot change a correlation beyond rounding:
// n and rot_sym - n are inverse rotations, so the set of copies is the same either way. applyGeometry's isIdentity shortcut cannot
// trigger: the smallest angle is 360 / 99 degrees. correlationIndex and applyGeometry are the forms of xh_corr.h and xh_applygeo.h.
// Refused: rot_sym outside 2 .. 99, Cn outside 1 .. 99, entries that are not finite, and an ungated helical trial for which
// xh_fsym_helical_depth gives -1 (zHelical <= 0, where the reference divides by zero; heightFraction outside (0, 1]; the dihedral copies
// over an even Z covered entirely with zHelical < 1 or > Z, where the reference's recursion never ends: DESIGN 5s).
#include "xh_applygeo.h"
#include "xh_corr.h"
#include "xh_helix.h"
#include "xh_reduce.h"
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace {

constexpr double FS_PI = 3.14159265358979323846;
constexpr int FS_TILE = 8;                               // trials of one workgroup
constexpr size_t FS_PARTIAL_BYTES = (size_t)1 << 29;     // the partial sums of one launch hold at most this much
constexpr size_t FS_MATRIX_BYTES = (size_t)1 << 28;      // and its matrices this much
constexpr int FS_MAX_ORDER = 99;
constexpr double FS_GATED = -1e38;                        // minus the gate's 1e38 (:396-399)
enum { FS_T_GATHER = 0, FS_T_FINISH, FS_T_SELECT, FS_NT };

struct FsBest { double corr; long long index; };

// volume_sym at the voxel (x, y, z) of one trial: v0 + sum_n applyGeometry(src, A_n); Ainv [nmat][9], rows (x', y', z')
template <int DEG>
__device__ __forceinline__ double fs_axis_value(const double *__restrict__ src, XhDims d, const double *__restrict__ Ainv, int nmat, double x, double y, double z, double v0)
{
    double acc = v0;
    for (int n = 0; n < nmat; ++n) {
        const double *a = Ainv + 9 * n;
        double xp = x * a[0] + y * a[1] + z * a[2];
        double yp = x * a[3] + y * a[4] + z * a[5];
        double zp = x * a[6] + y * a[7] + z * a[8];
        bool outsideHit = sy_axis<false>(xp, d.X);
        outsideHit = sy_axis<false>(yp, d.Y) || outsideHit;
        outsideHit = sy_axis<false>(zp, d.Z) || outsideHit;
        const double aux = outsideHit ? 0.0 : sy_interp3<DEG, false>(src, d, xp, yp, zp);
        acc = acc + aux;
    }
    return acc;
}

// the three sums of a trial's y over the workgroup's masked voxels -> partials [trial][brick][3]
__device__ __forceinline__ void fs_brick_sums(double (&red)[3][256], bool live, double yv, double x1, double mean_x, int t, int b, double *__restrict__ partials)
{
    double v[3] = {0.0, 0.0, 0.0};
    if (live) {
        v[0] = yv;
        v[1] = yv * yv;
        v[2] = (x1 - mean_x) * yv;
    }
    xh_tree256(red, v);               // its first barrier comes after every thread's read of red[c][0] below: thread 0 alone reads it
    if (threadIdx.x == 0) {
        double *o = partials + ((size_t)t * gridDim.x + b) * 3;
        for (int c = 0; c < 3; ++c) o[c] = red[c][0];
    }
}

// grid (bricks, tiles of trials); src: V (DEG 1) or its coefficients (DEG 3); mats [m][nmat][9]
template <int DEG>
__global__ void __launch_bounds__(256)
k_fs_axis(const double *__restrict__ src, const double *__restrict__ V, const int *__restrict__ mask, const double *__restrict__ mats, int nmat, int m, XhDims d,
          int nbx, int nby, double mean_x, double *__restrict__ partials)
{
    __shared__ double red[3][256];
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int j = bx * 8 + (threadIdx.x & 7), i = by * 8 + ((threadIdx.x >> 3) & 7), k = bz * 4 + (threadIdx.x >> 6);
    const bool inside = j < d.X && i < d.Y && k < d.Z;
    const size_t n = inside ? ((size_t)k * d.Y + i) * d.X + j : 0;
    const bool live = inside && (mask == nullptr || mask[n] != 0);
    const double x1 = live ? V[n] : 0.0;
    const double x = j - d.X / 2, y = i - d.Y / 2, z = k - d.Z / 2;
    const int t0 = blockIdx.y * FS_TILE, t1 = min(t0 + FS_TILE, m);
    for (int t = t0; t < t1; ++t) {
        const double yv = live ? fs_axis_value<DEG>(src, d, mats + (size_t)t * nmat * 9, nmat, x, y, z, x1) : 0.0;
        fs_brick_sums(red, live, yv, x1, mean_x, t, b, partials);
    }
}

// grid (bricks, tiles of trials); helices [m]; cn: sinCn [Cn] then cosCn [Cn]; the mask is the clipped one and never null
__global__ void __launch_bounds__(256)
k_fs_helical(const double *__restrict__ V, const int *__restrict__ mask, const SyHelix *__restrict__ helices, const double *__restrict__ cn, int Cn, int m,
             XhDims d, int nbx, int nby, double mean_x, double *__restrict__ partials)
{
    __shared__ double red[3][256];
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int jj = bx * 8 + (threadIdx.x & 7), ii = by * 8 + ((threadIdx.x >> 3) & 7), kk = bz * 4 + (threadIdx.x >> 6);
    const bool inside = jj < d.X && ii < d.Y && kk < d.Z;
    const size_t n = inside ? ((size_t)kk * d.Y + ii) * d.X + jj : 0;
    const bool live = inside && mask[n] != 0;
    const double x1 = live ? V[n] : 0.0;
    const int i = ii - d.Y / 2, j = jj - d.X / 2, k = kk - d.Z / 2;
    const double rot = atan2((double)i, (double)j);
    const double rho = sqrt((double)i * i + (double)j * j);
    const int t0 = blockIdx.y * FS_TILE, t1 = min(t0 + FS_TILE, m);
    for (int t = t0; t < t1; ++t) {
        const SyHelix &H = helices[t];
        const double yv = live ? sy_helical_value(V, d, H, cn, cn + Cn, k, rot + H.rot0, rho) : 0.0;
        fs_brick_sums(red, live, yv, x1, mean_x, t, b, partials);
    }
}

// one workgroup per trial: partials [m][nbricks][3] -> corr [m]
__global__ void __launch_bounds__(256) k_fs_finish(const double *__restrict__ partials, int nbricks, XhCorrStats S, double *__restrict__ corr)
{
    __shared__ double red[3][256];
    xh_brick_totals<3>(partials + (size_t)blockIdx.x * nbricks * 3, nbricks, red);
    if (threadIdx.x == 0) corr[blockIdx.x] = xh_corr_index(red[0][0], red[1][0], red[2][0], S);
}

// one workgroup: the first of corr [m] (trial base + t) strictly above the running best, which starts at 0 with no winner when first.
// A NaN compares false and is never taken
__global__ void __launch_bounds__(256) k_fs_select(const double *__restrict__ corr, int m, long long base, int first, FsBest *__restrict__ best)
{
    __shared__ double sf[256];
    __shared__ int si[256];
    const double running = first ? 0.0 : best->corr;
    const int per = (m + 255) / 256, a = threadIdx.x * per, e = min(a + per, m);
    double bf = running;
    int bi = -1;
    for (int t = a; t < e; ++t)
        if (corr[t] > bf) { bf = corr[t]; bi = t; }
    sf[threadIdx.x] = bf;
    si[threadIdx.x] = bi;
    __syncthreads();
    // the chunks are in trial order: the lower thread keeps its own on a tie
    for (int s = 1; s < 256; s <<= 1) {
        if ((threadIdx.x & (2 * s - 1)) == 0) {
            const int o = threadIdx.x + s;
            if (si[o] >= 0 && sf[o] > sf[threadIdx.x]) { sf[threadIdx.x] = sf[o]; si[threadIdx.x] = si[o]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (first) { best->corr = 0.0; best->index = -1; }
        if (si[0] >= 0) { best->corr = sf[0]; best->index = base + si[0]; }
    }
}

// the materialised volume_sym of one trial, every voxel (the reference forms it everywhere)
template <int DEG>
__global__ void __launch_bounds__(256)
k_fs_axis_volume(const double *__restrict__ src, const double *__restrict__ V, const double *__restrict__ mats, int nmat, XhDims d, int nbx, int nby, double *__restrict__ out)
{
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int j = bx * 8 + (threadIdx.x & 7), i = by * 8 + ((threadIdx.x >> 3) & 7), k = bz * 4 + (threadIdx.x >> 6);
    if (j >= d.X || i >= d.Y || k >= d.Z) return;
    const size_t n = ((size_t)k * d.Y + i) * d.X + j;
    out[n] = fs_axis_value<DEG>(src, d, mats, nmat, (double)(j - d.X / 2), (double)(i - d.Y / 2), (double)(k - d.Z / 2), V[n]);
}

// symmetry_Helical's Vout with the mask: 0 outside it
__global__ void __launch_bounds__(256)
k_fs_helical_volume(const double *__restrict__ V, const int *__restrict__ mask, const SyHelix *__restrict__ helix, const double *__restrict__ cn, int Cn, XhDims d,
                    int nbx, int nby, double *__restrict__ out)
{
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int jj = bx * 8 + (threadIdx.x & 7), ii = by * 8 + ((threadIdx.x >> 3) & 7), kk = bz * 4 + (threadIdx.x >> 6);
    if (jj >= d.X || ii >= d.Y || kk >= d.Z) return;
    const size_t n = ((size_t)kk * d.Y + ii) * d.X + jj;
    const int i = ii - d.Y / 2, j = jj - d.X / 2, k = kk - d.Z / 2;
    const SyHelix &H = helix[0];
    double v = 0.0;
    if (mask[n] != 0) v = sy_helical_value(V, d, H, cn, cn + Cn, k, atan2((double)i, (double)j) + H.rot0, sqrt((double)i * i + (double)j * j));
    out[n] = v;
}

// ---------------------------------------------------------------------------------------------------------------- host helpers
// rotation3DMatrix(ang, axis): the rotation by ang degrees about the unit vector along axis, in the sense of rotation3DMatrix(ang, 'Z')
void fs_rotation_about(double ang, const double *axis, double *A)
{
    double x = axis[0], y = axis[1], z = axis[2];
    const double n = std::sqrt(x * x + y * y + z * z);
    x /= n; y /= n; z /= n;
    const double a = ang * FS_PI / 180.0, c = std::cos(a), s = std::sin(a), t = 1 - c;
    A[0] = t * x * x + c;     A[1] = t * x * y + s * z; A[2] = t * x * z - s * y;
    A[3] = t * x * y - s * z; A[4] = t * y * y + c;     A[5] = t * y * z + s * x;
    A[6] = t * x * z + s * y; A[7] = t * y * z - s * x; A[8] = t * z * z + c;
}

// the rot_sym - 1 matrices of a trial (:373-381) and their cofactor inverses; either output may be null
void fs_axis_matrices(double rot, double tilt, int rot_sym, double *A, double *Ainv)
{
    double E[9], M[9], Mi[9];
    xh_fp_euler(rot, tilt, 0.0, E);
    for (int n = 1; n < rot_sym; ++n) {
        fs_rotation_about(360.0 / rot_sym * n, E + 6, M);
        sy_inv3x3(M, Mi);
        if (A) std::copy_n(M, 9, A + 9 * (size_t)(n - 1));
        if (Ainv) std::copy_n(Mi, 9, Ainv + 9 * (size_t)(n - 1));
    }
}

// :396-399
bool fs_gated(int Z, double zHelical, double rotHelical, const double *box)
{
    if (zHelical < 0 || zHelical > Z * 0.4) return true;
    if (box && (zHelical < box[0] || zHelical > box[1] || rotHelical < box[2] || rotHelical > box[3])) return true;
    return false;
}

// The depth of interpolatedElement3DHelical's recursion for the sample points of the masked symmetry_Helical, or -1 where it has no bound
// (DESIGN 5s). With n = round(heightFraction Z) <= Z every kp lies in [zFirst, zLast] inside [STARTINGZ, FINISHINGZ], and so do floor(kp)
// and, where kp is not an integer, floor(kp) + 1: depth 0 for any zHelical > 0. The dihedral copies sit at -kp in [-zLast, -zFirst];
// -zFirst = n / 2 passes FINISHINGZ = Z - 1 - Z / 2 only for n == Z even, by exactly one plane. The corner FINISHINGZ + 1 is sent to
// z' = FINISHINGZ + 1 - zHelical, whose corners of weight != 0 lie inside z if and only if 1 <= zHelical <= Z: at zHelical == 1 z' is
// FINISHINGZ itself and the plane above it has weight 0; below 1 the plane FINISHINGZ + 1 comes back with a weight, and is sent to the
// same z' without end.
int fs_helical_depth(int Z, double zHelical, double heightFraction, bool dihedral)
{
    if (!(zHelical > 0.0) || !std::isfinite(zHelical)) return -1;
    if (!(heightFraction > 0.0 && heightFraction <= 1.0)) return -1;
    const long n = std::lround(heightFraction * Z);
    if (n < 1 || n > Z) return -1;
    if (dihedral && Z % 2 == 0 && n == Z) return zHelical >= 1.0 && zHelical <= (double)Z ? 1 : -1;
    return 0;
}

}  // namespace

struct xh_fsym {
    xh_ctx *ctx = nullptr;
    XhDims d = {};
    size_t N = 0;
    int nbx = 0, nby = 0, nbz = 0, nbricks = 0, capacity = 0, batch = 0;
    bool loaded = false, masked = false, splines = false, clipped = false;
    double clippedFor = 0;                     // the heightFraction the clipped mask and its statistics were made for
    XhCorrStats stats = {}, hstats = {};
    std::vector<double> hV;
    std::vector<int32_t> hMask;
    xh_sym *sym = nullptr;                     // for the coefficients (xh_sym_coefficients)
    XhBuf V, coef, mask, hmask, mats, helices, cn, partials, corr, best, one;
    XhLapTimer<FS_NT> tm;
    void finish()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    ~xh_fsym()
    {
        finish();
        if (sym) xh_sym_destroy(sym);
    }
};

namespace {

int fs_finish_and_select(xh_fsym *h, const XhCorrStats &S, int mb, int64_t base, bool first, bool select)
{
    XH_TRY(h->tm.lap(FS_T_GATHER));
    XH_LAUNCH256(h->ctx, k_fs_finish, (unsigned)mb, (const double *)h->partials.p, h->nbricks, S, dp(h->corr));
    XH_TRY(h->tm.lap(FS_T_FINISH));
    if (select) {
        XH_LAUNCH256(h->ctx, k_fs_select, 1, (const double *)h->corr.p, mb, (long long)base, first ? 1 : 0, (FsBest *)h->best.p);
        XH_TRY(h->tm.lap(FS_T_SELECT));
    }
    return XH_OK;
}

int fs_read_best(xh_fsym *h, int64_t *best_index, double *best_corr)
{
    FsBest b;
    XH_HIP(hipMemcpy(&b, h->best.p, sizeof(FsBest), hipMemcpyDeviceToHost));
    *best_index = b.index;
    *best_corr = b.corr;
    return XH_OK;
}

int fs_check_order(const char *who, int rot_sym)
{
    XH_CHECK(rot_sym >= 2 && rot_sym <= FS_MAX_ORDER, XH_ERR_ARG, "%s: rot_sym %d (2 .. %d)", who, rot_sym, FS_MAX_ORDER);
    return XH_OK;
}

// the correlations of all m axis trials, launch by launch; select: the running best in h->best
int fs_axis_run(xh_fsym *h, const char *who, const double *h_rt, int64_t m, int rot_sym, bool select, double *h_corr)
{
    XH_CHECK(h->loaded, XH_ERR_STATE, "%s: no volume (xh_fsym_set_volume comes first)", who);
    XH_TRY(fs_check_order(who, rot_sym));
    XH_CHECK(m >= 0 && m <= ((int64_t)1 << 40), XH_ERR_ARG, "%s: %lld trials", who, (long long)m);
    for (int64_t t = 0; t < 2 * m; ++t) XH_CHECK(std::isfinite(h_rt[t]), XH_ERR_ARG, "%s: entry %d of trial %lld is not finite", who, (int)(t & 1), (long long)(t / 2));
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int nmat = rot_sym - 1;
    const int batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)h->batch, FS_MATRIX_BYTES / (sizeof(double) * 9 * nmat)));
    const int mfirst = (int)std::min<int64_t>(m, batch);
    XH_TRY(xh_buf_reserve(h->ctx, h->mats, sizeof(double) * 9 * nmat * (size_t)std::max(mfirst, 1)));
    std::vector<double> M((size_t)mfirst * nmat * 9);
    for (int64_t t0 = 0; t0 < m; t0 += batch) {
        const int mb = (int)std::min<int64_t>(batch, m - t0);
        for (int t = 0; t < mb; ++t) fs_axis_matrices(h_rt[2 * (t0 + t)], h_rt[2 * (t0 + t) + 1], rot_sym, nullptr, M.data() + (size_t)t * nmat * 9);
        XH_HIP(hipMemcpyAsync(h->mats.p, M.data(), sizeof(double) * 9 * nmat * (size_t)mb, hipMemcpyHostToDevice, st));
        XH_HIP(hipStreamSynchronize(st));                 // M is reused by the next launch
        XH_TRY(h->tm.start());
        const dim3 grid((unsigned)h->nbricks, (unsigned)((mb + FS_TILE - 1) / FS_TILE));
        const int *mask = h->masked ? (const int *)h->mask.p : (const int *)nullptr;
        if (h->splines)
            hipLaunchKernelGGL((k_fs_axis<3>), grid, dim3(256), 0, st, (const double *)h->coef.p, (const double *)h->V.p, mask, (const double *)h->mats.p, nmat, mb, h->d,
                               h->nbx, h->nby, h->stats.mean_x, dp(h->partials));
        else
            hipLaunchKernelGGL((k_fs_axis<1>), grid, dim3(256), 0, st, (const double *)h->V.p, (const double *)h->V.p, mask, (const double *)h->mats.p, nmat, mb, h->d,
                               h->nbx, h->nby, h->stats.mean_x, dp(h->partials));
        XH_LAUNCH_CHECK();
        XH_TRY(fs_finish_and_select(h, h->stats, mb, t0, t0 == 0, select));
        if (h_corr) XH_HIP(hipMemcpyAsync(h_corr + t0, h->corr.p, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
    }
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

// the mask clipped to [zFirst, zLast] (:280-288) on a copy, and the statistics of V under it
int fs_clip_mask(xh_fsym *h, const char *who, double heightFraction)
{
    if (h->clipped && h->clippedFor == heightFraction) return XH_OK;
    const XhDims d = h->d;
    const long n = std::lround(heightFraction * d.Z);
    const int zFirst = -(int)(n / 2), zLast = zFirst + (int)n - 1;
    std::vector<int32_t> m(h->N);
    const size_t plane = (size_t)d.Y * d.X;
    for (int kk = 0; kk < d.Z; ++kk) {
        const int k = kk - d.Z / 2;
        const bool in = k >= zFirst && k <= zLast;
        for (size_t e = 0; e < plane; ++e) m[kk * plane + e] = in ? (h->masked ? h->hMask[kk * plane + e] : 1) : 0;
    }
    XH_TRY(xh_corr_stats(who, "the volume", h->hV.data(), m.data(), h->N, h->hstats));
    XH_TRY(xh_buf_reserve(h->ctx, h->hmask, sizeof(int32_t) * h->N));
    XH_HIP(hipMemcpyAsync(h->hmask.p, m.data(), sizeof(int32_t) * h->N, hipMemcpyHostToDevice, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    h->clipped = true;
    h->clippedFor = heightFraction;
    return XH_OK;
}

int fs_check_helical(xh_fsym *h, const char *who, int Cn)
{
    XH_CHECK(h->loaded, XH_ERR_STATE, "%s: no volume (xh_fsym_set_volume comes first)", who);
    XH_CHECK(Cn >= 1 && Cn <= FS_MAX_ORDER, XH_ERR_ARG, "%s: Cn = %d (1 .. %d)", who, Cn, FS_MAX_ORDER);
    return XH_OK;
}

int fs_check_depth(const char *who, int Z, double zHelical, double heightFraction, bool dihedral)
{
    XH_CHECK(fs_helical_depth(Z, zHelical, heightFraction, dihedral) >= 0, XH_ERR_UNSUPPORTED,
             "%s: zHelical %g voxels, heightFraction %g%s on Z = %d: the helical interpolation's recursion has no bound (zHelical must be above 0, heightFraction in "
             "(0, 1], and the dihedral copies over an even Z covered entirely need 1 <= zHelical <= Z)", who, zHelical, heightFraction, dihedral ? ", dihedral" : "", Z);
    return XH_OK;
}

int fs_upload_cn(xh_fsym *h, int Cn)
{
    std::vector<double> cs(2 * (size_t)Cn);
    sy_cn_table(Cn, cs.data());
    XH_HIP(hipMemcpyAsync(h->cn.p, cs.data(), sizeof(double) * cs.size(), hipMemcpyHostToDevice, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

// the correlations of all m helical trials (rot in degrees, z in voxels); the gated ones get -1e38 without a launch
int fs_helical_run(xh_fsym *h, const char *who, const double *h_rz, int64_t m, const double *h_box, bool dihedral, double heightFraction, int Cn, bool select,
                   int64_t *best_index, double *best_corr, double *h_corr)
{
    XH_TRY(fs_check_helical(h, who, Cn));
    XH_CHECK(m >= 0 && m <= ((int64_t)1 << 40), XH_ERR_ARG, "%s: %lld trials", who, (long long)m);
    XH_CHECK(std::isfinite(heightFraction), XH_ERR_ARG, "%s: heightFraction is not finite", who);
    for (int64_t t = 0; t < 2 * m; ++t) XH_CHECK(std::isfinite(h_rz[t]), XH_ERR_ARG, "%s: entry %d of trial %lld is not finite", who, (int)(t & 1), (long long)(t / 2));
    if (h_box)
        for (int c = 0; c < 4; ++c) XH_CHECK(std::isfinite(h_box[c]), XH_ERR_ARG, "%s: entry %d of the search box is not finite", who, c);
    const XhDims d = h->d;
    std::vector<int64_t> live;
    for (int64_t t = 0; t < m; ++t) {
        if (fs_gated(d.Z, h_rz[2 * t + 1], h_rz[2 * t], h_box)) {
            if (h_corr) h_corr[t] = FS_GATED;
            continue;
        }
        XH_TRY(fs_check_depth(who, d.Z, h_rz[2 * t + 1], heightFraction, dihedral));
        live.push_back(t);
    }
    if (select) { *best_index = -1; *best_corr = 0.0; }
    if (live.empty()) return XH_OK;
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    XH_TRY(fs_clip_mask(h, who, heightFraction));
    XH_TRY(fs_upload_cn(h, Cn));
    const int64_t ml = (int64_t)live.size();
    std::vector<SyHelix> H((size_t)std::min<int64_t>(ml, h->batch));
    std::vector<double> got(h_corr ? (size_t)ml : 0);
    for (int64_t t0 = 0; t0 < ml; t0 += h->batch) {
        const int mb = (int)std::min<int64_t>(h->batch, ml - t0);
        for (int t = 0; t < mb; ++t) {
            const double *p = h_rz + 2 * live[t0 + t];
            H[t] = sy_make_helix(d.Z, p[1], p[0] * FS_PI / 180.0, 0.0, heightFraction, Cn, dihedral);      // DEG2RAD(rotHelical), rot0 = 0 (:400)
        }
        XH_HIP(hipMemcpyAsync(h->helices.p, H.data(), sizeof(SyHelix) * mb, hipMemcpyHostToDevice, st));
        XH_HIP(hipStreamSynchronize(st));                 // H is reused by the next launch
        XH_TRY(h->tm.start());
        const dim3 grid((unsigned)h->nbricks, (unsigned)((mb + FS_TILE - 1) / FS_TILE));
        hipLaunchKernelGGL(k_fs_helical, grid, dim3(256), 0, st, (const double *)h->V.p, (const int *)h->hmask.p, (const SyHelix *)h->helices.p, (const double *)h->cn.p, Cn,
                           mb, d, h->nbx, h->nby, h->hstats.mean_x, dp(h->partials));
        XH_LAUNCH_CHECK();
        XH_TRY(fs_finish_and_select(h, h->hstats, mb, t0, t0 == 0, select));
        if (h_corr) XH_HIP(hipMemcpyAsync(got.data() + t0, h->corr.p, sizeof(double) * mb, hipMemcpyDeviceToHost, st));
    }
    XH_HIP(hipStreamSynchronize(st));
    if (h_corr)
        for (int64_t t = 0; t < ml; ++t) h_corr[live[t]] = got[t];
    if (select) {
        XH_TRY(fs_read_best(h, best_index, best_corr));
        if (*best_index >= 0) *best_index = live[*best_index];        // the index among the trials that ran -> the caller's
    }
    return XH_OK;
}

}  // namespace

extern "C" {

int xh_fsym_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t capacity, xh_fsym **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_fsym_create: null argument");
    XH_CHECK(Z >= 2 && Y >= 2 && X >= 2, XH_ERR_ARG, "xh_fsym_create: bad size %d x %d x %d", Z, Y, X);
    XH_CHECK(Z <= 1024 && Y <= 1024 && X <= 1024, XH_ERR_UNSUPPORTED, "xh_fsym_create: sizes above 1024 are not supported (%d x %d x %d)", Z, Y, X);
    XH_CHECK(capacity >= 1 && capacity <= (1 << 20), XH_ERR_ARG, "xh_fsym_create: capacity %d (1 .. %d)", capacity, 1 << 20);
    std::unique_ptr<xh_fsym> h(new xh_fsym);
    XH_HIP(hipSetDevice(ctx->device));
    h->ctx = ctx;
    h->d = XhDims{Z, Y, X, X / 2 + 1};
    h->N = (size_t)Z * Y * X;
    h->nbx = (X + 7) / 8;
    h->nby = (Y + 7) / 8;
    h->nbz = (Z + 3) / 4;
    h->nbricks = h->nbx * h->nby * h->nbz;
    h->capacity = capacity;
    // trials of one launch: the capacity, less where their partial sums would pass FS_PARTIAL_BYTES (the results do not depend on it);
    // 65535 tiles is the grid's y limit
    const size_t perTrial = sizeof(double) * 3 * (size_t)h->nbricks;
    h->batch = (int)std::max<size_t>(1, std::min<size_t>({(size_t)capacity, FS_PARTIAL_BYTES / perTrial, (size_t)65535 * FS_TILE}));
    XH_TRY(xh_buf_alloc(ctx, h->V, sizeof(double) * h->N));
    XH_TRY(xh_buf_alloc(ctx, h->helices, sizeof(SyHelix) * h->batch));
    XH_TRY(xh_buf_alloc(ctx, h->one, std::max(sizeof(SyHelix), sizeof(double) * 9 * (FS_MAX_ORDER - 1))));
    XH_TRY(xh_buf_alloc(ctx, h->cn, sizeof(double) * 2 * (FS_MAX_ORDER + 1)));
    XH_TRY(xh_buf_alloc(ctx, h->partials, perTrial * h->batch));
    XH_TRY(xh_buf_alloc(ctx, h->corr, sizeof(double) * h->batch));
    XH_TRY(xh_buf_alloc(ctx, h->best, sizeof(FsBest)));
    XH_TRY(h->tm.create(ctx));
    *out = h.release();
    return XH_OK;
}

int xh_fsym_destroy(xh_fsym *h)
{
    delete h;
    return XH_OK;
}

int xh_fsym_set_volume(xh_fsym *h, const double *h_V, const int32_t *h_mask, int32_t splines)
{
    XH_CHECK(h && h_V, XH_ERR_ARG, "xh_fsym_set_volume: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    h->loaded = false;
    h->clipped = false;
    XH_TRY(xh_corr_stats("xh_fsym_set_volume", "the volume", h_V, h_mask, h->N, h->stats));
    h->hV.assign(h_V, h_V + h->N);
    h->masked = h_mask != nullptr;
    if (h_mask) h->hMask.assign(h_mask, h_mask + h->N);
    else h->hMask.clear();
    XH_HIP(hipMemcpyAsync(h->V.p, h->hV.data(), sizeof(double) * h->N, hipMemcpyHostToDevice, st));
    if (h_mask) {
        XH_TRY(xh_buf_reserve(h->ctx, h->mask, sizeof(int32_t) * h->N));
        XH_HIP(hipMemcpyAsync(h->mask.p, h->hMask.data(), sizeof(int32_t) * h->N, hipMemcpyHostToDevice, st));
    }
    h->splines = splines != 0;
    if (h->splines) {
        if (!h->sym) XH_TRY(xh_sym_create(h->ctx, h->d.Z, h->d.Y, h->d.X, &h->sym));
        XH_TRY(xh_buf_reserve(h->ctx, h->coef, sizeof(double) * h->N));
        XH_TRY(xh_sym_coefficients(h->sym, (const double *)h->V.p, dp(h->coef)));
    }
    XH_HIP(hipStreamSynchronize(st));
    h->loaded = true;
    return XH_OK;
}

int xh_fsym_stats(const xh_fsym *h, int32_t clipped, double *h_stats)
{
    XH_CHECK(h && h_stats, XH_ERR_ARG, "xh_fsym_stats: null argument");
    XH_CHECK(h->loaded && (!clipped || h->clipped), XH_ERR_STATE, "xh_fsym_stats: no volume, or no helical fit yet");
    const XhCorrStats &S = clipped ? h->hstats : h->stats;
    h_stats[0] = S.n; h_stats[1] = S.mean_x; h_stats[2] = S.stddev_x; h_stats[3] = S.S0;
    return XH_OK;
}

int xh_fsym_axis_matrices(double rot, double tilt, int32_t rot_sym, double *h_A, double *h_Ainv)
{
    XH_CHECK(h_A || h_Ainv, XH_ERR_ARG, "xh_fsym_axis_matrices: null argument");
    XH_TRY(fs_check_order("xh_fsym_axis_matrices", rot_sym));
    XH_CHECK(std::isfinite(rot) && std::isfinite(tilt), XH_ERR_ARG, "xh_fsym_axis_matrices: an angle is not finite");
    fs_axis_matrices(rot, tilt, rot_sym, h_A, h_Ainv);
    return XH_OK;
}

int xh_fsym_grid(double first0, double last0, double step0, double first1, double last1, double step1, int64_t limit, double *h_p, int64_t *count, int64_t *n_outer,
                 int64_t *n_inner)
{
    XH_CHECK(count, XH_ERR_ARG, "xh_fsym_grid: null argument");
    const double lo[2] = {first0, first1}, hi[2] = {last0, last1}, step[2] = {step0, step1};
    for (int a = 0; a < 2; ++a) {
        XH_CHECK(std::isfinite(lo[a]) && std::isfinite(hi[a]) && std::isfinite(step[a]), XH_ERR_ARG, "xh_fsym_grid: range %d is not finite", a);
        // the reference's loop `v <= last; v += step` never ends for these
        XH_CHECK(!(lo[a] <= hi[a] && (step[a] <= 0 || lo[a] + step[a] == lo[a] || hi[a] + step[a] == hi[a])), XH_ERR_ARG,
                 "xh_fsym_grid: range %d (%g .. %g by %g) never ends", a, lo[a], hi[a], step[a]);
    }
    int64_t c = 0, outer = 0, inner = 0;
    for (double u = lo[0]; u <= hi[0]; u += step[0]) {
        ++outer;
        for (double v = lo[1]; v <= hi[1]; v += step[1]) {
            XH_CHECK(c < limit, XH_ERR_UNSUPPORTED, "xh_fsym_grid: more than %lld trials", (long long)limit);
            if (outer == 1) ++inner;
            if (h_p) {
                h_p[2 * (size_t)c] = u;
                h_p[2 * (size_t)c + 1] = v;
            }
            ++c;
        }
    }
    *count = c;
    if (n_outer) *n_outer = outer;
    if (n_inner) *n_inner = inner;
    return XH_OK;
}

int xh_fsym_helical_gate(int32_t Z, double zHelical, double rotHelical, double z0, double zF, double rot0, double rotF, int32_t *gated)
{
    XH_CHECK(gated, XH_ERR_ARG, "xh_fsym_helical_gate: null argument");
    const double box[4] = {z0, zF, rot0, rotF};
    *gated = fs_gated(Z, zHelical, rotHelical, box) ? 1 : 0;
    return XH_OK;
}

int xh_fsym_helical_depth(int32_t Z, double zHelical, double heightFraction, int32_t dihedral, int32_t *depth)
{
    XH_CHECK(depth, XH_ERR_ARG, "xh_fsym_helical_depth: null argument");
    XH_CHECK(Z >= 2, XH_ERR_ARG, "xh_fsym_helical_depth: Z = %d", Z);
    *depth = fs_helical_depth(Z, zHelical, heightFraction, dihedral != 0);
    return XH_OK;
}

int xh_fsym_axis_fit(xh_fsym *h, const double *h_rot_tilt, int64_t m, int32_t rot_sym, double *h_corr)
{
    XH_CHECK(h && (h_rot_tilt || m == 0) && (h_corr || m == 0), XH_ERR_ARG, "xh_fsym_axis_fit: null argument");
    return fs_axis_run(h, "xh_fsym_axis_fit", h_rot_tilt, m, rot_sym, false, h_corr);
}

int xh_fsym_axis_search(xh_fsym *h, const double *h_rot_tilt, int64_t m, int32_t rot_sym, int64_t *best_index, double *best_corr, double *h_corr)
{
    XH_CHECK(h && h_rot_tilt && best_index && best_corr, XH_ERR_ARG, "xh_fsym_axis_search: null argument");
    XH_CHECK(m >= 1, XH_ERR_ARG, "xh_fsym_axis_search: no trials");
    XH_TRY(fs_axis_run(h, "xh_fsym_axis_search", h_rot_tilt, m, rot_sym, true, h_corr));
    return fs_read_best(h, best_index, best_corr);
}

int xh_fsym_helical_fit(xh_fsym *h, const double *h_rot_z, int64_t m, const double *h_box, int32_t dihedral, double heightFraction, int32_t Cn, double *h_corr)
{
    XH_CHECK(h && (h_rot_z || m == 0) && (h_corr || m == 0), XH_ERR_ARG, "xh_fsym_helical_fit: null argument");
    return fs_helical_run(h, "xh_fsym_helical_fit", h_rot_z, m, h_box, dihedral != 0, heightFraction, Cn, false, nullptr, nullptr, h_corr);
}

int xh_fsym_helical_search(xh_fsym *h, const double *h_rot_z, int64_t m, const double *h_box, int32_t dihedral, double heightFraction, int32_t Cn, int64_t *best_index,
                           double *best_corr, double *h_corr)
{
    XH_CHECK(h && h_rot_z && best_index && best_corr, XH_ERR_ARG, "xh_fsym_helical_search: null argument");
    XH_CHECK(m >= 1, XH_ERR_ARG, "xh_fsym_helical_search: no trials");
    return fs_helical_run(h, "xh_fsym_helical_search", h_rot_z, m, h_box, dihedral != 0, heightFraction, Cn, true, best_index, best_corr, h_corr);
}

int xh_fsym_axis_volume(xh_fsym *h, double rot, double tilt, int32_t rot_sym, double *d_out)
{
    XH_CHECK(h && d_out, XH_ERR_ARG, "xh_fsym_axis_volume: null argument");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_fsym_axis_volume: no volume (xh_fsym_set_volume comes first)");
    XH_CHECK(d_out != h->V.p && d_out != h->coef.p, XH_ERR_ARG, "xh_fsym_axis_volume: the output may not be a volume of the handle");
    XH_TRY(fs_check_order("xh_fsym_axis_volume", rot_sym));
    XH_CHECK(std::isfinite(rot) && std::isfinite(tilt), XH_ERR_ARG, "xh_fsym_axis_volume: an angle is not finite");
    const int nmat = rot_sym - 1;
    std::vector<double> M((size_t)nmat * 9);
    fs_axis_matrices(rot, tilt, rot_sym, nullptr, M.data());
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(h->one.p, M.data(), sizeof(double) * M.size(), hipMemcpyHostToDevice, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    if (h->splines) XH_LAUNCH256(h->ctx, (k_fs_axis_volume<3>), (unsigned)h->nbricks, (const double *)h->coef.p, (const double *)h->V.p, (const double *)h->one.p, nmat, h->d, h->nbx, h->nby, d_out);
    else XH_LAUNCH256(h->ctx, (k_fs_axis_volume<1>), (unsigned)h->nbricks, (const double *)h->V.p, (const double *)h->V.p, (const double *)h->one.p, nmat, h->d, h->nbx, h->nby, d_out);
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

int xh_fsym_helical_volume(xh_fsym *h, double rotHelical, double zHelical, int32_t dihedral, double heightFraction, int32_t Cn, double *d_out)
{
    XH_CHECK(h && d_out, XH_ERR_ARG, "xh_fsym_helical_volume: null argument");
    XH_TRY(fs_check_helical(h, "xh_fsym_helical_volume", Cn));
    XH_CHECK(d_out != h->V.p, XH_ERR_ARG, "xh_fsym_helical_volume: the output may not be a volume of the handle");
    XH_CHECK(std::isfinite(rotHelical) && std::isfinite(zHelical) && std::isfinite(heightFraction), XH_ERR_ARG, "xh_fsym_helical_volume: a parameter is not finite");
    XH_TRY(fs_check_depth("xh_fsym_helical_volume", h->d.Z, zHelical, heightFraction, dihedral != 0));
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_TRY(fs_clip_mask(h, "xh_fsym_helical_volume", heightFraction));
    XH_TRY(fs_upload_cn(h, Cn));
    const SyHelix H = sy_make_helix(h->d.Z, zHelical, rotHelical * FS_PI / 180.0, 0.0, heightFraction, Cn, dihedral != 0);
    XH_HIP(hipMemcpyAsync(h->one.p, &H, sizeof(SyHelix), hipMemcpyHostToDevice, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    XH_LAUNCH256(h->ctx, k_fs_helical_volume, (unsigned)h->nbricks, (const double *)h->V.p, (const int *)h->hmask.p, (const SyHelix *)h->one.p, (const double *)h->cn.p, Cn, h->d,
                 h->nbx, h->nby, d_out);
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

int xh_fsym_set_timing(xh_fsym *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_fsym_set_timing: null handle");
    h->tm.set(on != 0);
    return XH_OK;
}

int xh_fsym_stage_ms(const xh_fsym *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_fsym_stage_ms: null argument");
    h->tm.read(h_ms);
    return XH_OK;
}

}  // extern "C"
