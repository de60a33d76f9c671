// xh_sym.hip -- the device side of xmipp_transform_symmetrize (reconstruction/symmetrize.{h,cpp}, ProgSymmetrize; data/symmetries.cpp
// :1574-1705 for the helix; the reference runs all of it on the CPU in one serial loop), fp64, no FMA contraction: the source
// coordinates feed comparisons (the wrap / outside thresholds, the (int) and ceil of the taps, kp against zFirst / zLast).
//
//   coefficients    produceSplineCoefficients(BSPLINE3) of a Z x Y x X box: the recursive filter of d_prefilter_line (xh_bspline.h) along
//                   x, then y, then z. The x pass stages whole rows in LDS (a thread walks its row there, not in HBM); the y and z passes
//                   give a thread one line, neighbouring threads neighbouring x (coalesced).
//   outside mean    the mean of the input over r^2 >= (min(dims) / 2)^2 (BinaryCircularMask OUTSIDE_MASK, mask.cpp:193-217, with the integer
//                   division of symmetrize.cpp:133-135), sum and count through the fixed tree (xh_reduce.h): two runs give the same bytes.
//   the pass        for every output voxel and every matrix of the list the source point Ainv (x, y, z), wrapped (realWRAP) or given the
//                   outside value per axis, interpolated (LINEAR: eight neighbours; BSPLINE3: 4 x 4 x 4 mirrored taps), added to V_in in
//                   the list's order in a register, times 1 / (n + 1) unless sum. No V_aux volume exists. A workgroup owns an 8 x 8 x 4
//                   brick of the output. LINEAR gathers from global memory (k_sy_pass); BSPLINE3 stages the brick's source box of
//                   coefficients in LDS for every matrix whose box lies inside the volume and gathers otherwise (k_sy_pass_staged): the
//                   same bits either way, 1.01 to 1.32 times the gather's rate.
//   images          symmetrizeImage (:187-214) for a whole stack in one launch: I + sum_i rotate(I, 360 i / order), times 1 / order.
//   helix           symmetry_Helical (symmetries.cpp:1632-1705) as written; interpolatedElement3DHelical's recursion (:1577-1630) is at
//                   most one level deep for the parameters the entry point accepts (sy_helical_depth) and is written as two
//                   nested levels. helicalDihedral: the pass with one matrix (180 degrees about X, WRAP), (V_out + Vrotated) * 0.5.
//
// The per-voxel applyGeometry (range test per axis, linear and cubic taps) and the cofactor inverse are in xh_applygeo.h, shared with xh_valign.hip
// and xh_fsym.hip; the helix's per-voxel sum and its interpolation are in xh_helix.h, shared with xh_fsym.hip.
// xmippCore is not in the reference tree: applyGeometry's 3-D branch is its 2-D branch, as k_rs_apply of xh_rsig.hip has it,
// with a z axis added. The one deviation: a source coordinate is x A00 + y A01 + z A02, not A00 added along the row.
// Reference behaviours kept as written: the (int) truncation of the linear taps (a coordinate in (-1, 0) extrapolates from taps 0 and 1),
// m2 >= dim -> 0 under wrap, the w != 0 && m2 < dim guards, one mirror per spline tap, 1.0 / (n + 1.0f), Llength + 1 terms of the helix
// and its edge weights.
#include "xh_applygeo.h"
#include "xh_helix.h"
#include "xh_reduce.h"
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace {

constexpr double SY_PI = 3.14159265358979323846;
constexpr int SY_MAX_MATRICES = 1024;
constexpr int SY_MAX_CN = 99;          // "n must be an integer number with no more than 2 digits"
enum { SY_T_COEFFS = 0, SY_T_OUTSIDE, SY_T_PASS, SY_NT };

// the inverse of a list entry, rows (x', y', z'); ident: applyGeometry's isIdentity shortcut (a copy)
struct SyMat { double a[9]; double ident; };

// ---------------------------------------------------------------------------------------------------------------- coefficients
// x pass: rows [r0, r0 + TR) of the nrows = (Z Y) rows of length X through LDS, thread <-> row. in -> out; they may be the same memory
// (every load of a workgroup's rows comes before the barrier, every store after it), so neither is restrict. TR is 64 up to X = 95 and
// falls to 5 at X = 1024 (48 KB of LDS): on large boxes most of a workgroup's 64 threads only copy, which is correct and slow; the
// pass is 0.2 of 0.7 ms at 256^3, against 4 to 66 ms of the symmetry pass behind it
__global__ void __launch_bounds__(64) k_sy_prefilter_x(const double *in, double *out, int X, size_t nrows, int TR)
{
    extern __shared__ __align__(16) unsigned char sy_smem[];
    double *s = reinterpret_cast<double *>(sy_smem);
    const size_t r0 = (size_t)blockIdx.x * TR;
    if (r0 >= nrows) return;
    const int nrow = nrows - r0 < (size_t)TR ? (int)(nrows - r0) : TR;
    const int ld = X | 1;                              // odd: the threads' rows start on different banks
    const double *src = in + r0 * X;
    for (int e = threadIdx.x; e < nrow * X; e += 64) {
        const int r = e / X, c = e - r * X;
        s[r * ld + c] = src[e];
    }
    __syncthreads();
    if ((int)threadIdx.x < nrow) d_prefilter_line(s + threadIdx.x * ld, X, 1);
    __syncthreads();
    double *dst = out + r0 * X;
    for (int e = threadIdx.x; e < nrow * X; e += 64) {
        const int r = e / X, c = e - r * X;
        dst[e] = s[r * ld + c];
    }
}

// y pass: thread <-> (slice, x); z pass: thread <-> (y, x). In place
__global__ void __launch_bounds__(256) k_sy_prefilter_y(double *__restrict__ c, int nslices, int Y, int X)
{
    XH_GRID_LOOP(t, (size_t)nslices * X) {
        const size_t k = t / X;
        const int x = (int)(t - k * X);
        d_prefilter_line(c + k * Y * X + x, Y, X);
    }
}

__global__ void __launch_bounds__(256) k_sy_prefilter_z(double *__restrict__ c, int Z, int Y, int X)
{
    XH_GRID_LOOP(t, (size_t)Y * X) d_prefilter_line(c + t, Z, Y * X);
}

// ---------------------------------------------------------------------------------------------------------------- outside mean
// one volume: (sum, count) over r2 >= rad2 to partials [2][gridDim.x]
__global__ void __launch_bounds__(256) k_sy_outside(const double *__restrict__ v, XhDims d, double rad2, double *__restrict__ partials)
{
    double a[2] = {0.0, 0.0};
    const int cz = d.Z / 2, cy = d.Y / 2, cx = d.X / 2;
    XH_GRID_LOOP(n, (size_t)d.Z * d.Y * d.X) {
        const int j = (int)(n % d.X);
        const size_t r = n / d.X;
        const int i = (int)(r % d.Y), k = (int)(r / d.Y);
        double diff = k - cz;
        const double z2 = diff * diff;
        diff = i - cy;
        const double z2y2 = z2 + diff * diff;
        diff = j - cx;
        if (z2y2 + diff * diff >= rad2) { a[0] += v[n]; a[1] += 1.0; }
    }
    xh_block_partials<2>(a, partials);
}

// a stack: one workgroup per image (grid-strided), avg [img]
__global__ void __launch_bounds__(256) k_sy_outside_images(const double *__restrict__ imgs, int nimg, int Y, int X, double rad2, double *__restrict__ avg)
{
    __shared__ double red[2][256];
    const int cy = Y / 2, cx = X / 2;
    for (int img = blockIdx.x; img < nimg; img += gridDim.x) {
        const double *v = imgs + (size_t)img * Y * X;
        double a[2] = {0.0, 0.0};
        for (int n = threadIdx.x; n < Y * X; n += 256) {
            const int i = n / X, j = n - i * X;
            double diff = i - cy;
            const double y2 = diff * diff;
            diff = j - cx;
            if (y2 + diff * diff >= rad2) { a[0] += v[n]; a[1] += 1.0; }
        }
        __syncthreads();
        xh_tree256(red, a);
        if (threadIdx.x == 0) avg[img] = red[0][0] / red[1][0];
    }
}

// the pass: out = (vin + sum_m aux_m) * scale, aux_m = applyGeometry of src by matrix m. vin null: the sum alone (0.0 + aux is aux).
// src: the volume (DEG 1) or its coefficients (DEG 3); vsrc: the volume itself, for an identity entry
template <int DEG, bool WRAP>
__global__ void __launch_bounds__(256)
k_sy_pass(const double *__restrict__ src, const double *__restrict__ vsrc, const double *__restrict__ vin, const SyMat *__restrict__ mats, int nmat,
          XhDims d, int nbx, int nby, double outside, double scale, double *__restrict__ out)
{
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int j = bx * 8 + (threadIdx.x & 7), i = by * 8 + ((threadIdx.x >> 3) & 7), k = bz * 4 + (threadIdx.x >> 6);
    if (j >= d.X || i >= d.Y || k >= d.Z) return;
    const size_t n = ((size_t)k * d.Y + i) * d.X + j;
    const double x = j - d.X / 2, y = i - d.Y / 2, z = k - d.Z / 2;
    double acc = vin ? vin[n] : 0.0;
    for (int m = 0; m < nmat; ++m) {
        const SyMat &A = mats[m];
        double aux;
        if (A.ident != 0) aux = vsrc[n];
        else {
            double xp = x * A.a[0] + y * A.a[1] + z * A.a[2];
            double yp = x * A.a[3] + y * A.a[4] + z * A.a[5];
            double zp = x * A.a[6] + y * A.a[7] + z * A.a[8];
            bool outsideHit = sy_axis<WRAP>(xp, d.X);
            outsideHit = sy_axis<WRAP>(yp, d.Y) || outsideHit;
            outsideHit = sy_axis<WRAP>(zp, d.Z) || outsideHit;
            aux = outsideHit ? outside : sy_interp3<DEG, WRAP>(src, d, xp, yp, zp);
        }
        acc = acc + aux;
    }
    out[n] = acc * scale;
}

// The same pass for cubic splines with the source box of a brick staged in LDS. Per matrix the workgroup bounds the brick's source
// points (a sum of per-term minima and maxima, with a margin) and adds the spline support; where that box lies inside the volume no
// coordinate is outside the range and no tap is mirrored, so the box (SY_BOX doubles at the most) is loaded once and the 64 taps of every
// voxel come from LDS with the weights, order and values of sy_interp3: the result has the same bits as k_sy_pass's. A brick at the border,
// or a box that does not fit, gathers from global memory exactly as k_sy_pass does. The decision is the same for the whole workgroup.
constexpr int SY_BOX = 18 * 18 * 18;
template <bool WRAP>
__global__ void __launch_bounds__(256)
k_sy_pass_staged(const double *__restrict__ src, const double *__restrict__ vsrc, const double *__restrict__ vin, const SyMat *__restrict__ mats, int nmat,
                 XhDims d, int nbx, int nby, double outside, double scale, double *__restrict__ out)
{
    __shared__ double box[SY_BOX];
    const int b = blockIdx.x;
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int j = bx * 8 + (threadIdx.x & 7), i = by * 8 + ((threadIdx.x >> 3) & 7), k = bz * 4 + (threadIdx.x >> 6);
    const bool live = j < d.X && i < d.Y && k < d.Z;
    const size_t n = live ? ((size_t)k * d.Y + i) * d.X + j : 0;
    const double x = j - d.X / 2, y = i - d.Y / 2, z = k - d.Z / 2;
    // the brick's logical corners
    const double p0[3] = {(double)(bx * 8 - d.X / 2), (double)(by * 8 - d.Y / 2), (double)(bz * 4 - d.Z / 2)};
    const double p1[3] = {(double)(min(bx * 8 + 7, d.X - 1) - d.X / 2), (double)(min(by * 8 + 7, d.Y - 1) - d.Y / 2), (double)(min(bz * 4 + 3, d.Z - 1) - d.Z / 2)};
    const int dim[3] = {d.X, d.Y, d.Z};
    double acc = live && vin ? vin[n] : 0.0;
    for (int m = 0; m < nmat; ++m) {
        const SyMat &A = mats[m];
        int lo[3], nb[3];
        bool staged = A.ident == 0;
        for (int r = 0; r < 3; ++r) {
            double cmin = 0, cmax = 0;
            for (int c = 0; c < 3; ++c) {
                const double u = A.a[3 * r + c] * p0[c], v = A.a[3 * r + c] * p1[c];
                cmin += fmin(u, v);
                cmax += fmax(u, v);
            }
            const int ilo = (int)floor(cmin + dim[r] / 2 - 2.0 - 1e-3), ihi = (int)floor(cmax + dim[r] / 2 + 2.0 + 1e-3);
            staged = staged && ilo >= 0 && ihi <= dim[r] - 1;
            lo[r] = ilo;
            nb[r] = ihi - ilo + 1;
        }
        staged = staged && nb[0] * nb[1] * nb[2] <= SY_BOX;
        double aux = 0;
        if (staged) {
            __syncthreads();                                   // the taps of the matrix before have been read
            const int nxy = nb[0] * nb[1], tot = nxy * nb[2];
            for (int e = threadIdx.x; e < tot; e += 256) {
                const int ez = e / nxy, r2 = e - ez * nxy, ey = r2 / nb[0], ex = r2 - ey * nb[0];
                box[e] = src[((size_t)(lo[2] + ez) * d.Y + (lo[1] + ey)) * d.X + (lo[0] + ex)];
            }
            __syncthreads();
            if (live) {
                const double xp = x * A.a[0] + y * A.a[1] + z * A.a[2];
                const double yp = x * A.a[3] + y * A.a[4] + z * A.a[5];
                const double zp = x * A.a[6] + y * A.a[7] + z * A.a[8];
                const double xx = xp + d.X / 2, yy = yp + d.Y / 2, zz = zp + d.Z / 2;
                const int l1 = (int)ceil(xx - 2), m1 = (int)ceil(yy - 2), n1 = (int)ceil(zz - 2);
                double wx[4], wy[4], wz[4];
                d_bspline03_w4<double>(xx, l1, wx);
                d_bspline03_w4<double>(yy, m1, wy);
                d_bspline03_w4<double>(zz, n1, wz);
                // inside the box by construction; the clamps keep a stray index inside LDS
                const int ox = sy_clamp(l1 - lo[0], nb[0] - 3), oy = sy_clamp(m1 - lo[1], nb[1] - 3), oz = sy_clamp(n1 - lo[2], nb[2] - 3);
                double slices = 0;
#pragma unroll
                for (int tz = 0; tz < 4; ++tz) {
                    double columns = 0;
#pragma unroll
                    for (int ty = 0; ty < 4; ++ty) {
                        const double *ref = box + (oz + tz) * nxy + (oy + ty) * nb[0] + ox;
                        double rows = 0;
#pragma unroll
                        for (int u = 0; u < 4; ++u) rows += ref[u] * wx[u];
                        columns += rows * wy[ty];
                    }
                    slices += columns * wz[tz];
                }
                aux = slices;
            }
        } else if (live) {
            if (A.ident != 0) aux = vsrc[n];
            else {
                double xp = x * A.a[0] + y * A.a[1] + z * A.a[2];
                double yp = x * A.a[3] + y * A.a[4] + z * A.a[5];
                double zp = x * A.a[6] + y * A.a[7] + z * A.a[8];
                bool outsideHit = sy_axis<WRAP>(xp, d.X);
                outsideHit = sy_axis<WRAP>(yp, d.Y) || outsideHit;
                outsideHit = sy_axis<WRAP>(zp, d.Z) || outsideHit;
                aux = outsideHit ? outside : sy_interp3<3, WRAP>(src, d, xp, yp, zp);
            }
        }
        acc = acc + aux;
    }
    if (live) out[n] = acc * scale;
}

// symmetrizeImage for a stack [nimg][Y][X]: src the images (DEG 1) or their 2-D coefficients (DEG 3); mats: the order - 1 inverses of
// rotation2DMatrix(360 i / order); avg [img] the outside value (null: 0)
template <int DEG, bool WRAP>
__global__ void __launch_bounds__(256)
k_sy_images(const double *__restrict__ src, const double *__restrict__ imgs, const SyMat *__restrict__ mats, int nmat, int nimg, int Y, int X,
            const double *__restrict__ avg, double scale, double *__restrict__ out)
{
    const size_t per = (size_t)Y * X;
    XH_GRID_LOOP(n, per * nimg) {
        const size_t img = n / per;
        const int p = (int)(n - img * per), i = p / X, j = p - i * X;
        const double *s = src + img * per;
        const double x = j - X / 2, y = i - Y / 2;
        const double outside = avg ? avg[img] : 0.0;
        double acc = imgs[n];
        for (int m = 0; m < nmat; ++m) {
            const SyMat &A = mats[m];
            double aux;
            if (A.ident != 0) aux = imgs[n];
            else {
                double xp = x * A.a[0] + y * A.a[1] + A.a[2];
                double yp = x * A.a[3] + y * A.a[4] + A.a[5];
                bool outsideHit = sy_axis<WRAP>(xp, X);
                outsideHit = sy_axis<WRAP>(yp, Y) || outsideHit;
                if (outsideHit) aux = outside;
                else if (DEG == 1) {
                    double wx = xp + X / 2;
                    int m1 = (int)wx;
                    wx = wx - m1;
                    int m2 = m1 + 1;
                    double wy = yp + Y / 2;
                    int n1 = (int)wy;
                    wy = wy - n1;
                    int n2 = n1 + 1;
                    if (WRAP) {
                        if (m2 >= X) m2 = 0;
                        if (n2 >= Y) n2 = 0;
                    }
                    m1 = sy_clamp(m1, X); n1 = sy_clamp(n1, Y);
                    m2 = max(m2, 0); n2 = max(n2, 0);
                    const double wx_1 = 1 - wx, wy_1 = 1 - wy;
                    double aux2 = wy_1 * wx_1;
                    double tmp = aux2 * s[n1 * X + m1];
                    if (wx != 0 && m2 < X) tmp += (wy_1 - aux2) * s[n1 * X + m2];
                    if (wy != 0 && n2 < Y) {
                        aux2 = wy * wx_1;
                        tmp += aux2 * s[n2 * X + m1];
                        if (wx != 0 && m2 < X) tmp += (wy - aux2) * s[n2 * X + m2];
                    }
                    aux = tmp;
                } else {
                    const double xx = xp + X / 2, yy = yp + Y / 2;
                    const int l1 = (int)ceil(xx - 2), q1 = (int)ceil(yy - 2);
                    double wx[4], wy[4];
                    d_bspline03_w4<double>(xx, l1, wx);
                    d_bspline03_w4<double>(yy, q1, wy);
                    double columns = 0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const double *ref = s + (size_t)sy_mirror(q1 + t, Y) * X;
                        double rows = 0;
#pragma unroll
                        for (int u = 0; u < 4; ++u) rows += ref[sy_mirror(l1 + u, X)] * wx[u];
                        columns += rows * wy[t];
                    }
                    aux = columns;
                }
            }
            acc = acc + aux;
        }
        out[n] = acc * scale;
    }
}

// ---------------------------------------------------------------------------------------------------------------- helix
// symmetry_Helical (:1632-1705), mask == nullptr; sinCn / cosCn [Cn] from the host. The voxel's sum and the interpolation are in xh_helix.h
__global__ void __launch_bounds__(256)
k_sy_helical(const double *__restrict__ vin, XhDims d, SyHelix H, const double *__restrict__ sinCn, const double *__restrict__ cosCn, double *__restrict__ out)
{
    XH_GRID_LOOP(n, (size_t)d.Z * d.Y * d.X) {
        const int jj = (int)(n % d.X);
        const size_t r = n / d.X;
        const int i = (int)(r % d.Y) - d.Y / 2, k = (int)(r / d.Y) - d.Z / 2, j = jj - d.X / 2;
        const double rot = atan2((double)i, (double)j) + H.rot0;
        const double rho = sqrt((double)i * i + (double)j * j);
        out[n] = sy_helical_value(vin, d, H, sinCn, cosCn, k, rot, rho);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host helpers
// A (IS_NOT_INV) -> the record the kernels read
int sy_make_mat(const char *who, const double *A, SyMat &M)
{
    bool ident = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            XH_CHECK(std::isfinite(A[r * 3 + c]), XH_ERR_ARG, "%s: a matrix entry is not finite", who);
            if (std::fabs(A[r * 3 + c] - (r == c ? 1.0 : 0.0)) > SY_ACC) ident = false;
        }
    sy_inv3x3(A, M.a);
    M.ident = ident ? 1.0 : 0.0;
    for (double v : M.a) XH_CHECK(std::isfinite(v) && std::fabs(v) <= 1e3, XH_ERR_ARG, "%s: a matrix is singular or scales by more than 1000 (inverse entry %g)", who, v);
    return XH_OK;
}

// The depth of interpolatedElement3DHelical's recursion for symmetry_Helical's sample points, or -1 where it has no bound.
// With n = round(heightFraction Z) <= Z every kp lies in [zFirst, zLast] inside [STARTINGZ, FINISHINGZ]: no corner of weight != 0 is
// outside z, depth 0. The dihedral copies sit at -kp in [-zLast, -zFirst]; -zFirst = n / 2 passes FINISHINGZ = Z - 1 - Z / 2 only for
// n == Z even, by exactly one plane: the corner FINISHINGZ + 1 is sent to z' = FINISHINGZ + 1 - zHelical, whose corners floor(z') and
// floor(z') + 1 lie inside z if and only if 1 < zHelical <= Z (zHelical == 1 lands on FINISHINGZ with weight 0 above it, which the
// entry point still refuses with the rest of zHelical <= 1: there z' > FINISHINGZ is sent back to the same point without end).
int sy_helical_depth(int Z, double zHelical, double heightFraction, bool dihedral)
{
    if (!(zHelical > 1.0 && zHelical <= (double)Z)) return -1;
    if (!(heightFraction > 0.0 && heightFraction <= 1.0)) return -1;
    const long n = std::lround(heightFraction * Z);
    if (n < 1 || n > Z) return -1;
    return dihedral && Z % 2 == 0 && n == Z ? 1 : 0;
}

}  // namespace

struct xh_sym {
    xh_ctx *ctx = nullptr;
    XhDims d = {};
    size_t N = 0;
    unsigned grid = 0;
    int nmat = 0;
    XhBuf coef, mats, one, partials, result, helix, cn, stack, avg;
    XhPinned host;
    XhLapTimer<SY_NT> tm;
    void finish()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    ~xh_sym() { finish(); }
};

namespace {

// coefficients of nslices slices (a volume: all three passes; a stack: x and y only). d_in -> d_out, may alias
int sy_coefficients(xh_sym *h, const double *d_in, double *d_out, int nslices, bool volume)
{
    const int X = h->d.X, Y = h->d.Y;
    const size_t nrows = (size_t)nslices * Y;
    const int ld = X | 1;
    const int TR = std::max(1, std::min(64, (int)(48 * 1024 / (sizeof(double) * ld))));
    const size_t blocks = (nrows + TR - 1) / TR;
    hipLaunchKernelGGL(k_sy_prefilter_x, dim3((unsigned)blocks), dim3(64), sizeof(double) * (size_t)TR * ld, h->ctx->stream, d_in, d_out, X, nrows, TR);
    XH_LAUNCH_CHECK();
    XH_LAUNCH256(h->ctx, k_sy_prefilter_y, xh_grid256((size_t)nslices * X, h->ctx->num_cus, 8), d_out, nslices, Y, X);
    if (volume) XH_LAUNCH256(h->ctx, k_sy_prefilter_z, xh_grid256((size_t)Y * X, h->ctx->num_cus, 8), d_out, nslices, Y, X);
    return XH_OK;
}

int sy_outside_mean(xh_sym *h, const double *d_in, double *mean)
{
    const XhDims d = h->d;
    const int rad = std::min(d.X, std::min(d.Y, d.Z)) / 2;
    XH_LAUNCH256(h->ctx, k_sy_outside, h->grid, d_in, d, (double)rad * rad, dp(h->partials));
    double *hp = h->host.f64();
    XH_TRY(xh_reduce_finish(h->ctx, (const double *)h->partials.p, (int)h->grid, 2, dp(h->result), hp));
    *mean = hp[0] / hp[1];
    return XH_OK;
}

template <int DEG, bool WRAP>
int sy_launch_pass(xh_sym *h, const double *src, const double *vsrc, const double *vin, const SyMat *mats, int nmat, double outside, double scale, double *out)
{
    const XhDims d = h->d;
    const int nbx = (d.X + 7) / 8, nby = (d.Y + 7) / 8, nbz = (d.Z + 3) / 4;
    if (DEG == 3) XH_LAUNCH256(h->ctx, (k_sy_pass_staged<WRAP>), (unsigned)(nbx * nby * nbz), src, vsrc, vin, mats, nmat, d, nbx, nby, outside, scale, out);
    else XH_LAUNCH256(h->ctx, (k_sy_pass<DEG, WRAP>), (unsigned)(nbx * nby * nbz), src, vsrc, vin, mats, nmat, d, nbx, nby, outside, scale, out);
    return XH_OK;
}

// d_out = (vin + sum over the matrices of applyGeometry(d_src)) * scale; d_out is none of the inputs
int sy_pass(xh_sym *h, const double *d_src, const double *vin, const SyMat *mats, int nmat, int degree, bool wrap, double outside, double scale, double *d_out)
{
    const double *src = d_src;
    XH_TRY(h->tm.start());
    if (degree == 3) {
        XH_TRY(sy_coefficients(h, d_src, dp(h->coef), h->d.Z, true));
        src = dp(h->coef);
    }
    XH_TRY(h->tm.lap(SY_T_COEFFS));
    if (degree == 3) return wrap ? sy_launch_pass<3, true>(h, src, d_src, vin, mats, nmat, outside, scale, d_out) : sy_launch_pass<3, false>(h, src, d_src, vin, mats, nmat, outside, scale, d_out);
    return wrap ? sy_launch_pass<1, true>(h, src, d_src, vin, mats, nmat, outside, scale, d_out) : sy_launch_pass<1, false>(h, src, d_src, vin, mats, nmat, outside, scale, d_out);
}

int sy_check_volume(const xh_sym *h, const char *who)
{
    XH_CHECK(h->d.Z >= 2, XH_ERR_STATE, "%s: the handle was made for images (Z = 1)", who);
    return XH_OK;
}

int sy_check_degree(const char *who, int degree)
{
    XH_CHECK(degree == 1 || degree == 3, XH_ERR_UNSUPPORTED, "%s: spline order %d (1 and 3 are supported)", who, degree);
    return XH_OK;
}

}  // namespace

extern "C" {

int xh_sym_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, xh_sym **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_sym_create: null argument");
    XH_CHECK(Z >= 1 && Y >= 2 && X >= 2, XH_ERR_ARG, "xh_sym_create: bad size %d x %d x %d", Z, Y, X);
    XH_CHECK(Z <= 1024 && Y <= 1024 && X <= 1024, XH_ERR_UNSUPPORTED, "xh_sym_create: sizes above 1024 are not supported (%d x %d x %d)", Z, Y, X);
    std::unique_ptr<xh_sym> h(new xh_sym);
    XH_HIP(hipSetDevice(ctx->device));
    h->ctx = ctx;
    h->d = XhDims{Z, Y, X, X / 2 + 1};
    h->N = (size_t)Z * Y * X;
    h->grid = xh_grid256(h->N, ctx->num_cus, 4);
    if (Z >= 2) XH_TRY(xh_buf_alloc(ctx, h->coef, sizeof(double) * h->N));
    XH_TRY(xh_buf_alloc(ctx, h->mats, sizeof(SyMat) * SY_MAX_MATRICES));
    XH_TRY(xh_buf_alloc(ctx, h->one, sizeof(SyMat)));
    XH_TRY(xh_buf_alloc(ctx, h->cn, sizeof(double) * 2 * (SY_MAX_CN + 1)));
    XH_TRY(xh_buf_alloc(ctx, h->partials, sizeof(double) * 2 * h->grid));
    XH_TRY(xh_buf_alloc(ctx, h->result, sizeof(double) * 2));
    XH_TRY(xh_pinned_alloc(ctx, h->host, sizeof(double) * 2));
    XH_TRY(h->tm.create(ctx));
    *out = h.release();
    return XH_OK;
}

int xh_sym_destroy(xh_sym *h)
{
    delete h;
    return XH_OK;
}

int xh_sym_set_matrices(xh_sym *h, const double *h_R, int32_t n)
{
    XH_CHECK(h && (h_R || n == 0), XH_ERR_ARG, "xh_sym_set_matrices: null argument");
    XH_CHECK(n >= 0 && n <= SY_MAX_MATRICES, XH_ERR_ARG, "xh_sym_set_matrices: %d matrices (0 .. %d)", n, SY_MAX_MATRICES);
    std::vector<SyMat> M((size_t)n);
    for (int m = 0; m < n; ++m) {
        const double *R = h_R + 9 * (size_t)m;
        const double At[9] = {R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]};     // R.transpose(), symmetrize.cpp:159
        XH_TRY(sy_make_mat("xh_sym_set_matrices", At, M[m]));
    }
    XH_HIP(hipSetDevice(h->ctx->device));
    if (n) XH_HIP(hipMemcpyAsync(h->mats.p, M.data(), sizeof(SyMat) * n, hipMemcpyHostToDevice, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    h->nmat = n;
    return XH_OK;
}

int xh_sym_coefficients(xh_sym *h, const double *d_in, double *d_out)
{
    XH_CHECK(h && d_in && d_out, XH_ERR_ARG, "xh_sym_coefficients: null argument");
    XH_TRY(sy_check_volume(h, "xh_sym_coefficients"));
    XH_HIP(hipSetDevice(h->ctx->device));
    return sy_coefficients(h, d_in, d_out, h->d.Z, true);
}

int xh_sym_outside_mean(xh_sym *h, const double *d_in, double *h_mean)
{
    XH_CHECK(h && d_in && h_mean, XH_ERR_ARG, "xh_sym_outside_mean: null argument");
    XH_TRY(sy_check_volume(h, "xh_sym_outside_mean"));
    XH_HIP(hipSetDevice(h->ctx->device));
    return sy_outside_mean(h, d_in, h_mean);
}

int xh_sym_apply_geometry3d(xh_sym *h, const double *d_in, const double *h_A, int32_t degree, int32_t wrap, double outside, double *d_out)
{
    XH_CHECK(h && d_in && h_A && d_out, XH_ERR_ARG, "xh_sym_apply_geometry3d: null argument");
    XH_CHECK(d_in != d_out, XH_ERR_ARG, "xh_sym_apply_geometry3d: the output may not be the input");
    XH_TRY(sy_check_volume(h, "xh_sym_apply_geometry3d"));
    XH_TRY(sy_check_degree("xh_sym_apply_geometry3d", degree));
    SyMat M;
    XH_TRY(sy_make_mat("xh_sym_apply_geometry3d", h_A, M));
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(h->one.p, &M, sizeof(SyMat), hipMemcpyHostToDevice, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return sy_pass(h, d_in, nullptr, (const SyMat *)h->one.p, 1, degree, wrap != 0, outside, 1.0, d_out);
}

int xh_sym_symmetrize(xh_sym *h, const double *d_in, int32_t degree, int32_t wrap, int32_t sum, double *d_out)
{
    XH_CHECK(h && d_in && d_out, XH_ERR_ARG, "xh_sym_symmetrize: null argument");
    XH_CHECK(d_in != d_out, XH_ERR_ARG, "xh_sym_symmetrize: the output may not be the input");
    XH_TRY(sy_check_volume(h, "xh_sym_symmetrize"));
    XH_TRY(sy_check_degree("xh_sym_symmetrize", degree));
    XH_HIP(hipSetDevice(h->ctx->device));
    double avg = 0.0;
    XH_TRY(h->tm.start());
    if (!wrap) XH_TRY(sy_outside_mean(h, d_in, &avg));
    XH_TRY(h->tm.lap(SY_T_OUTSIDE));
    const double scale = sum ? 1.0 : 1.0 / (h->nmat + 1.0f);
    XH_TRY(sy_pass(h, d_in, d_in, (const SyMat *)h->mats.p, h->nmat, degree, wrap != 0, avg, scale, d_out));
    return h->tm.lap(SY_T_PASS);
}

int xh_sym_symmetrize_images(xh_sym *h, const double *d_in, int32_t n, int32_t order, int32_t degree, int32_t wrap, int32_t sum, double *d_out)
{
    XH_CHECK(h && d_in && d_out, XH_ERR_ARG, "xh_sym_symmetrize_images: null argument");
    XH_CHECK(d_in != d_out, XH_ERR_ARG, "xh_sym_symmetrize_images: the output may not be the input");
    XH_CHECK(h->d.Z == 1, XH_ERR_STATE, "xh_sym_symmetrize_images: the handle was made for volumes (Z = %d)", h->d.Z);
    XH_CHECK(n >= 1 && (size_t)n * h->N <= ((size_t)1 << 31), XH_ERR_ARG, "xh_sym_symmetrize_images: %d images", n);
    XH_CHECK(order >= 1 && order <= SY_MAX_MATRICES, XH_ERR_ARG, "xh_sym_symmetrize_images: order %d (1 .. %d)", order, SY_MAX_MATRICES);
    XH_TRY(sy_check_degree("xh_sym_symmetrize_images", degree));
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int Y = h->d.Y, X = h->d.X;
    // rotate (:209): rotation2DMatrix(360.0 / symorder * i), IS_NOT_INV
    std::vector<SyMat> M((size_t)order - 1);
    for (int i = 1; i < order; ++i) {
        const double a = (360.0 / order * i) * SY_PI / 180.0;
        const double c = std::cos(a), s = std::sin(a);
        const double A[9] = {c, s, 0, -s, c, 0, 0, 0, 1};
        XH_TRY(sy_make_mat("xh_sym_symmetrize_images", A, M[i - 1]));
    }
    if (order > 1) XH_HIP(hipMemcpyAsync(h->mats.p, M.data(), sizeof(SyMat) * M.size(), hipMemcpyHostToDevice, st));
    XH_HIP(hipStreamSynchronize(st));
    h->nmat = 0;                                          // the list of a volume is gone
    XH_TRY(h->tm.start());
    const double *src = d_in;
    if (degree == 3) {
        XH_TRY(xh_buf_reserve(h->ctx, h->stack, sizeof(double) * h->N * n));
        XH_TRY(sy_coefficients(h, d_in, dp(h->stack), n, false));
        src = dp(h->stack);
    }
    XH_TRY(h->tm.lap(SY_T_COEFFS));
    const double *avg = nullptr;
    if (!wrap) {
        XH_TRY(xh_buf_reserve(h->ctx, h->avg, sizeof(double) * n));
        const int rad = std::min(X, Y) / 2;
        XH_LAUNCH256(h->ctx, k_sy_outside_images, (unsigned)std::min(n, 65535), d_in, n, Y, X, (double)rad * rad, dp(h->avg));
        avg = dp(h->avg);
    }
    XH_TRY(h->tm.lap(SY_T_OUTSIDE));
    const double scale = sum ? 1.0 : 1.0 / order;
    const unsigned grid = xh_grid256(h->N * n, h->ctx->num_cus, 16);
    const SyMat *mats = (const SyMat *)h->mats.p;
    if (degree == 3) {
        if (wrap) XH_LAUNCH256(h->ctx, (k_sy_images<3, true>), grid, src, d_in, mats, order - 1, n, Y, X, avg, scale, d_out);
        else XH_LAUNCH256(h->ctx, (k_sy_images<3, false>), grid, src, d_in, mats, order - 1, n, Y, X, avg, scale, d_out);
    } else {
        if (wrap) XH_LAUNCH256(h->ctx, (k_sy_images<1, true>), grid, src, d_in, mats, order - 1, n, Y, X, avg, scale, d_out);
        else XH_LAUNCH256(h->ctx, (k_sy_images<1, false>), grid, src, d_in, mats, order - 1, n, Y, X, avg, scale, d_out);
    }
    return h->tm.lap(SY_T_PASS);
}

int xh_sym_helical_depth(int32_t Z, double zHelical, double heightFraction, int32_t dihedral, int32_t *depth)
{
    XH_CHECK(depth, XH_ERR_ARG, "xh_sym_helical_depth: null argument");
    XH_CHECK(Z >= 2, XH_ERR_ARG, "xh_sym_helical_depth: Z = %d", Z);
    *depth = sy_helical_depth(Z, zHelical, heightFraction, dihedral != 0);
    return XH_OK;
}

int xh_sym_helical(xh_sym *h, const double *d_in, double zHelical, double rotHelical, double rotPhaseHelical, int32_t Cn, int32_t dihedral, double heightFraction,
                   int32_t degree, double *d_out)
{
    XH_CHECK(h && d_in && d_out, XH_ERR_ARG, "xh_sym_helical: null argument");
    XH_CHECK(d_in != d_out, XH_ERR_ARG, "xh_sym_helical: the output may not be the input");
    XH_TRY(sy_check_volume(h, "xh_sym_helical"));
    XH_TRY(sy_check_degree("xh_sym_helical", degree));
    XH_CHECK(Cn >= 1 && Cn <= SY_MAX_CN, XH_ERR_ARG, "xh_sym_helical: Cn = %d (1 .. %d)", Cn, SY_MAX_CN);
    XH_CHECK(std::isfinite(rotHelical) && std::isfinite(rotPhaseHelical), XH_ERR_ARG, "xh_sym_helical: the rotation is not finite");
    const XhDims d = h->d;
    XH_CHECK(sy_helical_depth(d.Z, zHelical, heightFraction, dihedral != 0) >= 0, XH_ERR_UNSUPPORTED,
             "xh_sym_helical: zHelical %g voxels, heightFraction %g on Z = %d: the helical interpolation's recursion is bounded only for 1 < zHelical <= Z and "
             "0 < heightFraction <= 1 (at zHelical <= 1 the reference never terminates)", zHelical, heightFraction, d.Z);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const SyHelix H = sy_make_helix(d.Z, zHelical, rotHelical, rotPhaseHelical, heightFraction, Cn, dihedral != 0);
    std::vector<double> cs(2 * (size_t)Cn);
    sy_cn_table(Cn, cs.data());
    XH_HIP(hipMemcpyAsync(h->cn.p, cs.data(), sizeof(double) * cs.size(), hipMemcpyHostToDevice, st));
    XH_HIP(hipStreamSynchronize(st));
    XH_TRY(h->tm.start());
    double *hel = d_out;
    if (dihedral) {
        XH_TRY(xh_buf_reserve(h->ctx, h->helix, sizeof(double) * h->N));
        hel = dp(h->helix);
    }
    XH_LAUNCH256(h->ctx, k_sy_helical, xh_grid256(h->N, h->ctx->num_cus, 16), d_in, d, H, (const double *)h->cn.p, (const double *)h->cn.p + Cn, hel);
    XH_TRY(h->tm.lap(SY_T_PASS));
    if (!dihedral) return XH_OK;
    // rotate(spline, Vrotated, V_out, 180.0, 'X', WRAP); V_out += Vrotated; V_out *= 0.5 (symmetrize.cpp:175-178)
    const double a = 180.0 * SY_PI / 180.0, c = std::cos(a), s = std::sin(a);
    const double A[9] = {1, 0, 0, 0, c, -s, 0, s, c};
    SyMat M;
    XH_TRY(sy_make_mat("xh_sym_helical", A, M));
    XH_HIP(hipMemcpyAsync(h->one.p, &M, sizeof(SyMat), hipMemcpyHostToDevice, st));
    XH_HIP(hipStreamSynchronize(st));
    XH_TRY(sy_pass(h, hel, hel, (const SyMat *)h->one.p, 1, degree, true, 0.0, 0.5, d_out));
    return h->tm.lap(SY_T_PASS);
}

int xh_sym_set_timing(xh_sym *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_sym_set_timing: null handle");
    h->tm.set(on != 0);
    return XH_OK;
}

int xh_sym_stage_ms(const xh_sym *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_sym_stage_ms: null argument");
    h->tm.read(h_ms);
    return XH_OK;
}

}  // extern "C"
