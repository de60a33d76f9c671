// xh_wbp.hip -- the device side of xmipp_reconstruct_wbp (reconstruction/reconstruct_wbp.cpp, ProgRecWbp: weighted back-projection with
// Radermacher's arbitrary-geometry filter; the reference runs one image at a time on the CPU, with an MPI farm beside it), fp64, no FMA
// contraction: the filter's table index is the (int) of a quotient, the back-projection's taps the (int) of a coordinate, and both feed
// comparisons (the threshold, the sphere and image cuts).
//
//   prepare      apply2DFilterArbitraryGeometry :552-557: the matrix of getTransformationMatrix(A, true) (shifts and flip), and where it is
//                not the identity selfApplyGeometry(BSPLINE3, ., A, IS_INV, WRAP) from the image's spline coefficients (xh_bspline.h's
//                prefilter, xh_applygeo.h's range test); then the image times its weight. Written as the real parts of the transform's input.
//   transform    FourierTransform (:448): the complete D x D transform, times 1 / D^2. CenterFFT (:449, :490) moves nothing here: the filter
//                reads the uncentred array and forms the centred logical index of each cell itself.
//   k_wbp_filter filterOneImage :451-487. mat_f[k] of the image from mat_g (:458-462) goes through LDS in tiles of WB_TILE directions; a
//                thread owns one cell of the half plane (columns 0 .. D / 2), adds count_k * TSINC(x f_kx + y f_ky) over k = 0 .. no_mats - 1
//                in that order in one register, and divides by weight * diameter, or by SGN(weight) * threshold * diameter where
//                |weight| < threshold. weight(-i, -j) = weight(i, j) bit for bit (negation is exact, the index is the abs of a truncation
//                toward zero), so a thresholded cell with a partner outside the half plane counts twice; the cells of an even D's row
//                -D / 2 that have no partner and lie outside the half plane are evaluated for the count alone. count_thr is an integer
//                sum: one vector atomic per workgroup, the order cannot matter.
//   inverse      InverseFourierTransform (:491) reads the half plane only (setFromCompleteFourier) and runs a complex-to-real transform:
//                the filter writes the conjugate of each cell of columns 1 .. (D - 1) / 2 to its mirror cell, and the real part of the
//                complete inverse transform is that transform.
//   k_wbp_backproject  simpleBackprojection :362-434. A thread owns WB_SEG consecutive voxels of a row, loops over the batch's images in list
//                order and adds the bilinear sample to each voxel's value in a register; a batch continues from the stored volume, so the
//                sum has the reference's order for any capacity. No atomics. xp is carried along the row (xp += a00) as the reference
//                carries it: the thread first adds a00 once for every voxel of the row before its segment.
//   finish       with symmetry symmetrizeVolume at its defaults (BSPLINE3, WRAP, no outside average, no sum; xh_sym.hip), then the inner
//                sphere r^2 <= (diameter / 2.)^2 (:566-579).
//
// Nothing above depends on the capacity: an image's prepare, transform and filter see that image alone, count_thr is an integer sum, and a
// voxel adds the images in list order whatever the batches are.
//
// Behaviours kept as written:
//   - the three -tilt conventions: the directions are row 2 of Euler_angles2matrix(rot, -tilt, psi) (:327), the filter's matrix is
//     Euler_angles2matrix(-rot, tilt, -psi) (:447), the back-projection's the inverse of Euler_angles2matrix(rot, -tilt, psi) (:373-374).
//     The caller forms all of them: this file reads matrices and direction lists, never angles.
//   - mat_g[].count = (int) count_imgs[i] in sampled mode (:276): weights are truncated. The caller's business as well.
//   - simpleBackprojection tests yp and takes l = (int) yp and scaley ONCE PER ROW, at x = -dim2 (:406-412); yp += a01 along the row is
//     never read again. Every voxel of a row therefore interpolates between the same two image rows.
//   - dim2 = dim / 2 by integer division, z = -i + dim2, the cuts z^2 > r^2, z^2 + y^2 > r^2, x^2 + (z^2 + y^2) > r^2,
//     yp >= D - 1 || yp < 0, xp >= D - 1 || xp < 0.
//   - getTransformationMatrix and selfApplyGeometry: the matrix readApplyGeo applies as IS_NOT_INV is applied here as IS_INV, as :554 says.
// One deviation, as in xh_sym.hip and xh_rsig.hip: the source coordinates of selfApplyGeometry and of symmetrizeVolume are formed directly
// (x A00 + y A01 + A02), not by adding A00 along the row. The back-projection's xp is NOT formed directly: the direct form moves the
// volume by up to 2.9e-14 of its largest value, past the bound the tests derive.
// The table index is formed as (int)(argum / 0.0001) like TSINCVALUE; the division runs only where argum * 10000 lies within 1e-14 relative
// of an integer, elsewhere the truncation of the product is the same integer (the two quotients differ by less than 1e-15 relative).
#include "xh_applygeo.h"
#include "xh_plan.h"
#include <cmath>
#include <memory>
#include <vector>

namespace {

constexpr int WB_TILE = 256;                     // directions of one LDS tile: one per thread of the workgroup
constexpr int WB_SEG = 16;                       // voxels of a row that one thread of the back-projection owns
constexpr double WB_SAMPL = 0.0001;              // Tabsinc TSINC(0.0001, dim), :538
constexpr int WB_HROW = 22;                      // the caller's row: shiftX, shiftY, flip, weight, filter matrix [9], back-projection matrix [9]
enum { WB_T_PREPARE = 0, WB_T_TRANSFORM, WB_T_FILTER, WB_T_BACKPROJECT, WB_T_FINISH, WB_NT };

// what the kernels read of an image: rows 0 and 1 of A (IS_INV: the source point is A (x, y, 1)), isIdentity, the weight,
// a00 a01 a10 a11 a20 a21 of the filter's matrix and of the back-projection's
struct WbRow { double A[6]; double ident, weight; double f[6]; double b[6]; };

// interpolatedElementBSpline2D at the logical point (xp, yp) of an image's coefficients; the taps mirrored as in xh_applygeo.h
__device__ __forceinline__ double wb_interp2(const double *__restrict__ coef, int D, double xp, double yp)
{
    const double x = xp + D / 2, y = yp + D / 2;
    const int l1 = (int)ceil(x - 2), m1 = (int)ceil(y - 2);
    double wx[4], wy[4];
    d_bspline03_w4<double>(x, l1, wx);
    d_bspline03_w4<double>(y, m1, wy);
    int el[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) el[t] = sy_mirror(l1 + t, D);
    double columns = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double *ref = coef + (size_t)sy_mirror(m1 + t, D) * D;
        double rows = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) rows += ref[el[u]] * wx[u];
        columns += rows * wy[t];
    }
    return columns;
}

// grid (pixels / 256, images): F[e][n] = (the prepared image, 0)
__global__ void __launch_bounds__(256)
k_wbp_prepare(const float *__restrict__ img, const double *__restrict__ coef, const WbRow *__restrict__ rows, int D, xh_cd *__restrict__ F)
{
    const int DD = D * D, e = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= DD) return;
    const WbRow &R = rows[e];
    double v;
    if (R.ident != 0.0) v = (double)img[(size_t)e * DD + n];
    else {
        const int i = n / D, j = n - i * D, cen = D / 2;
        const double x = (double)(j - cen), y = (double)(i - cen);
        double xp = x * R.A[0] + y * R.A[1] + R.A[2];
        double yp = x * R.A[3] + y * R.A[4] + R.A[5];
        sy_axis<true>(xp, D);
        sy_axis<true>(yp, D);
        v = wb_interp2(coef + (size_t)e * DD, D, xp, yp);
    }
    F[(size_t)e * DD + n] = xh_cd{v * R.weight, 0.0};
}

// TSINCVALUE's index of argum, below nelem (an index past the table is never formed for rotation matrices and a diameter <= D)
__device__ __forceinline__ int wb_index(double argum, int nelem)
{
    const double q = argum * 10000.0;
    int n = (int)q;
    if (fabs(q - rint(q)) <= fabs(q) * 1e-14) n = (int)(argum / WB_SAMPL);
    return min(abs(n), nelem - 1);
}

// grid (work cells / 256, images). Work cell w < D (D / 2 + 1): cell (w / H, w % H) of the half plane; above, for even D, the cells
// (D / 2, D / 2 + 1 + e) that only count. w_out (nullable): the weights of image w_img, [D][D] in the uncentred layout
__global__ void __launch_bounds__(256)
k_wbp_filter(xh_cd *__restrict__ F, const WbRow *__restrict__ rows, const double *__restrict__ g, int no_mats, const double *__restrict__ table,
             int nelem, int D, double K, double threshold, double factor, double isize, unsigned long long *__restrict__ count_thr,
             double *__restrict__ w_out, int w_img)
{
    __shared__ double sfx[WB_TILE], sfy[WB_TILE], scnt[WB_TILE];
    __shared__ unsigned int s_count;
    const int e = blockIdx.y, H = D / 2 + 1, W0 = D * H, W = W0 + ((D & 1) ? 0 : D / 2 - 1);
    const int w = blockIdx.x * 256 + threadIdx.x;
    const bool live = w < W, extra = w >= W0;
    int iy = 0, jx = 0;
    if (live) {
        if (extra) { iy = D / 2; jx = D / 2 + 1 + (w - W0); }
        else { iy = w / H; jx = w - iy * H; }
    }
    const int i = (iy + D / 2) % D - D / 2, j = (jx + D / 2) % D - D / 2;     // the logical indices after CenterFFT(., true)
    const double x = K * j, y = K * i;
    const WbRow &R = rows[e];
    const double a00 = R.f[0], a01 = R.f[1], a10 = R.f[2], a11 = R.f[3], a20 = R.f[4], a21 = R.f[5];
    if (threadIdx.x == 0) s_count = 0;
    double weight = 0.;
    for (int k0 = 0; k0 < no_mats; k0 += WB_TILE) {
        const int nk = min(WB_TILE, no_mats - k0);
        __syncthreads();                                   // the tile before has been read; s_count is set
        if ((int)threadIdx.x < nk) {
            const double *q = g + 4 * (size_t)(k0 + threadIdx.x);
            sfx[threadIdx.x] = a00 * q[0] + a10 * q[1] + a20 * q[2];
            sfy[threadIdx.x] = a01 * q[0] + a11 * q[1] + a21 * q[2];
            scnt[threadIdx.x] = q[3];
        }
        __syncthreads();
        if (live)
            for (int k = 0; k < nk; ++k) {
                const double argum = x * sfx[k] + y * sfy[k];
                weight += scnt[k] * table[wb_index(argum, nelem)];
            }
    }
    unsigned int mine = 0;
    if (live) {
        const bool even = !(D & 1);
        const bool partner = !(even && (iy == D / 2 || jx == D / 2));       // (-i, -j) is a cell of the array
        const bool twice = !extra && partner && jx != 0;                       // and it lies outside the half plane
        const bool under = fabs(weight) < threshold;
        if (under) mine = twice ? 2 : 1;
        if (!extra) {
            const double div = under ? (weight >= 0 ? 1.0 : -1.0) * (threshold * factor) : weight * factor;
            xh_cd *Fe = F + (size_t)e * D * D;
            xh_cd c = Fe[(size_t)iy * D + jx];
            c.x *= isize;
            c.y *= isize;
            c.x /= div;
            c.y /= div;
            Fe[(size_t)iy * D + jx] = c;
            if (jx > 0 && 2 * jx < D) Fe[(size_t)((D - iy) % D) * D + (D - jx)] = xh_cd{c.x, -c.y};
        }
        if (w_out && e == w_img) {
            w_out[(size_t)iy * D + jx] = weight;
            if (twice) w_out[(size_t)((D - iy) % D) * D + (D - jx)] = weight;
        }
    }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(count_thr, (unsigned long long)s_count);
}

// grid (rows * segments / 256). A thread owns WB_SEG consecutive voxels of a row (i, j): it carries xp along the row as the reference does,
// after adding a00 once for every voxel of the row before its segment, so every voxel sees the reference's own xp. img [m][D][D]: the
// filtered images of the batch, rows[t].b their matrices
__global__ void __launch_bounds__(256)
k_wbp_backproject(const double *__restrict__ img, const WbRow *__restrict__ rows, int m, int D, int nseg, double radius2, double *__restrict__ vol)
{
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)D * D * nseg) return;
    const int seg = (int)(n % nseg), jj = (int)((n / nseg) % D), i = (int)(n / ((size_t)nseg * D));
    const int k0 = seg * WB_SEG;
    const double dim2 = D / 2, dim1 = D - 1;
    const double z = -i + dim2, y = jj - dim2, x0 = 0 - dim2;
    const double z2 = z * z;
    if (z2 > radius2) return;
    const double z2_plus_y2 = z2 + y * y;
    if (z2_plus_y2 > radius2) return;
    double *row = vol + ((size_t)i * D + jj) * D + k0;
    double v[WB_SEG];
    bool in[WB_SEG];
#pragma unroll
    for (int s = 0; s < WB_SEG; ++s) {
        const double x = (k0 + s) - dim2;
        in[s] = k0 + s < D && !(x * x + z2_plus_y2 > radius2);
        v[s] = in[s] ? row[s] : 0.0;
    }
    const size_t DD = (size_t)D * D;
    for (int t = 0; t < m; ++t) {
        const double *b = rows[t].b;
        const double a00 = b[0], a01 = b[1], a10 = b[2], a11 = b[3], a20 = b[4], a21 = b[5];
        const double xpz = z * a20 + dim2, ypz = z * a21 + dim2;
        const double yp = x0 * a01 + y * a11 + ypz;            // of the row's first voxel: the reference tests and truncates it once per row
        if (yp >= dim1 || yp < 0.0) continue;
        double xp = x0 * a00 + y * a10 + xpz;
        for (int q = 0; q < k0; ++q) xp += a00;
        const int l = (int)yp;
        const double scaley = yp - l, scale1y = 1. - scaley;
        const double *I = img + (size_t)t * DD + (size_t)l * D;
#pragma unroll
        for (int s = 0; s < WB_SEG; ++s, xp += a00) {
            if (!in[s] || xp >= dim1 || xp < 0.0) continue;
            const int mm = (int)xp;
            const double scalex = xp - mm, scale1x = 1. - scalex;
            const double value1 = scalex * I[mm + 1] + scale1x * I[mm];
            const double value2 = scalex * I[D + mm + 1] + scale1x * I[D + mm];
            v[s] += scaley * value2 + scale1y * value1;
        }
    }
#pragma unroll
    for (int s = 0; s < WB_SEG; ++s)
        if (in[s]) row[s] = v[s];
}

// BINARY_CIRCULAR_MASK, INNER_MASK about the Xmipp origin (data/mask.cpp:193-217): outside r^2 <= R1^2 the volume is 0
__global__ void __launch_bounds__(256) k_wbp_mask(double *__restrict__ vol, int D, double radius2)
{
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)D * D * D) return;
    const int c = D / 2;
    const double dx = (int)(n % D) - c, dy = (int)((n / D) % D) - c, dz = (int)(n / ((size_t)D * D)) - c;
    const double r2 = (dz * dz + dy * dy) + dx * dx;
    if (!(r2 <= radius2)) vol[n] = 0.0;
}

}  // namespace

struct xh_wbp {
    xh_ctx *ctx = nullptr;
    int D = 0, capacity = 0, no_mats = 0, nelem = 0, diameter = 0;
    size_t DD = 0, N = 0;
    double threshold = 0;
    bool directions = false;
    XhFft2d64 fft;
    xh_sym *sym = nullptr;
    XhBuf vol, vaux, img_in, coef, F, img, rows, g, table, count, wscratch;
    XhLapTimer<WB_NT> tm;
    void finish()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    ~xh_wbp()
    {
        finish();
        if (sym) xh_sym_destroy(sym);
    }
};

namespace {

int wb_make_row(const char *who, const double *q, WbRow &R)
{
    for (int c = 0; c < WB_HROW; ++c) XH_CHECK(std::isfinite(q[c]), XH_ERR_ARG, "%s: entry %d of an image's row is not finite", who, c);
    for (int c = 4; c < WB_HROW; ++c) XH_CHECK(std::fabs(q[c]) <= 1 + SY_ACC, XH_ERR_ARG, "%s: entry %d of an image's row, %g, is no entry of a rotation matrix", who, c, q[c]);
    // geo2TransformationMatrix with only_apply_shifts on a 3 x 3: the identity, the shifts in column 2, a flip negates A00 and A01
    double A[6] = {1, 0, q[0], 0, 1, q[1]};
    if (q[2] != 0) { A[0] *= -1.; A[1] *= -1.; }
    bool ident = true;
    const double I6[6] = {1, 0, 0, 0, 1, 0};
    for (int c = 0; c < 6; ++c) {
        R.A[c] = A[c];
        if (std::fabs(A[c] - I6[c]) > SY_ACC) ident = false;
    }
    R.ident = ident ? 1.0 : 0.0;
    R.weight = q[3];
    const double *f = q + 4, *b = q + 13;
    R.f[0] = f[0]; R.f[1] = f[1]; R.f[2] = f[3]; R.f[3] = f[4]; R.f[4] = f[6]; R.f[5] = f[7];
    R.b[0] = b[0]; R.b[1] = b[1]; R.b[2] = b[3]; R.b[3] = b[4]; R.b[4] = b[6]; R.b[5] = b[7];
    return XH_OK;
}

int wb_filter_launch(xh_wbp *h, int m, unsigned long long *count, double *w_out, int w_img)
{
    const int D = h->D, W = D * (D / 2 + 1) + ((D & 1) ? 0 : D / 2 - 1);
    hipLaunchKernelGGL(k_wbp_filter, dim3((unsigned)((W + 255) / 256), (unsigned)m), dim3(256), 0, h->ctx->stream, cp(h->F), (const WbRow *)h->rows.p,
                       (const double *)h->g.p, h->no_mats, (const double *)h->table.p, h->nelem, D, (double)h->diameter / D, h->threshold,
                       (double)h->diameter, 1.0 / ((double)D * (double)D), count, w_out, w_img);
    XH_LAUNCH_CHECK();
    return XH_OK;
}


// ---------------------------------------------------------------------------------------------------------------- host only
// xmippCore's macros as reconstruction/directions.cpp uses them
double wb_realwrap(double x, double x0, double xF)
{
    if (x >= x0 && x <= xF) return x;
    if (x < x0) return x - (int)((x - x0) / (xF - x0) - 1) * (xF - x0);
    return x - (int)((x - xF) / (xF - x0) + 1) * (xF - x0);
}
int wb_round(double x) { return x > 0 ? (int)(x + 0.5) : (int)(x - 0.5); }
int wb_ceil(double x) { return x == (int)x ? (int)x : (x > 0 ? (int)(x + 1) : (int)x); }

bool wb_close(double rot, double tilt, double rot2, double tilt2, double rot_limit, double tilt_limit)
{
    const double diff_rot = std::fabs(wb_realwrap(rot - rot2, -180, 180)), diff_tilt = std::fabs(wb_realwrap(tilt - tilt2, -180, 180));
    return (rot_limit - diff_rot) > 1e-3 && (tilt_limit - diff_tilt) > 1e-3;
}

// directions_are_unique (directions.cpp:31-89) without symmetry and with include_mirrors: the direction itself and Euler_another_set of it
// (rot + 180, -tilt)
bool wb_unique(double rot, double tilt, double rot2, double tilt2, double rot_limit, double tilt_limit)
{
    bool are_unique = true;
    if (wb_close(rot, tilt, rot2, tilt2, rot_limit, tilt_limit)) are_unique = false;
    if (wb_close(rot, tilt, rot2 + 180., -tilt2, rot_limit, tilt_limit)) are_unique = false;
    return are_unique;
}

double wb_diff(double rot1, double tilt1, double rot2, double tilt2)
{
    const double diff_rot = std::fabs(wb_realwrap(rot1 - rot2, -180, 180)), diff_tilt = std::fabs(wb_realwrap(tilt1 - tilt2, -180, 180));
    return std::sqrt((diff_rot * diff_rot) + (diff_tilt * diff_tilt));
}

}  // namespace

extern "C" {

int xh_wbp_create(xh_ctx *ctx, int32_t D, int32_t capacity, xh_wbp **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_wbp_create: null argument");
    XH_CHECK(D >= 2, XH_ERR_ARG, "xh_wbp_create: bad size %d", D);
    XH_CHECK(D <= 1024, XH_ERR_UNSUPPORTED, "xh_wbp_create: sizes above 1024 are not supported (%d)", D);
    XH_CHECK(capacity >= 1 && capacity <= 65535, XH_ERR_ARG, "xh_wbp_create: capacity %d (1 .. 65535)", capacity);
    std::unique_ptr<xh_wbp> h(new xh_wbp);
    XH_HIP(hipSetDevice(ctx->device));
    h->ctx = ctx;
    h->D = D;
    h->capacity = capacity;
    h->DD = (size_t)D * D;
    h->N = h->DD * D;
    XH_TRY(xh_fft2d64_create(ctx, D, D, h->fft, "xh_wbp_create"));
    XH_TRY(xh_buf_alloc(ctx, h->vol, sizeof(double) * h->N));
    XH_TRY(xh_buf_alloc(ctx, h->img_in, sizeof(float) * h->DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->coef, sizeof(double) * h->DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->F, sizeof(xh_cd) * h->DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->img, sizeof(double) * h->DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->rows, sizeof(WbRow) * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->count, sizeof(unsigned long long) * 2));
    XH_TRY(xh_buf_alloc(ctx, h->wscratch, sizeof(double) * h->DD));
    // Tabsinc(0.0001, dim): no_elem = (int)(xmax / sampl) entries of sin(xx) / xx, xx = i sampl PI, entry 0 = 1
    h->nelem = (int)(D / WB_SAMPL);
    std::vector<double> tab((size_t)h->nelem);
    tab[0] = 1;
    for (int i = 1; i < h->nelem; ++i) {
        const double xx = (double)i * WB_SAMPL * 3.14159265358979323846;
        tab[i] = std::sin(xx) / xx;
    }
    XH_TRY(xh_buf_upload(ctx, h->table, tab.data(), sizeof(double) * tab.size()));
    XH_TRY(h->tm.create(ctx));
    XH_HIP(hipMemsetAsync(h->vol.p, 0, sizeof(double) * h->N, ctx->stream));
    XH_HIP(hipMemsetAsync(h->count.p, 0, sizeof(unsigned long long) * 2, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    *out = h.release();
    return XH_OK;
}

int xh_wbp_destroy(xh_wbp *h)
{
    delete h;
    return XH_OK;
}

int xh_wbp_reset(xh_wbp *h)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_wbp_reset: null handle");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemsetAsync(h->vol.p, 0, sizeof(double) * h->N, h->ctx->stream));
    XH_HIP(hipMemsetAsync(h->count.p, 0, sizeof(unsigned long long) * 2, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

int xh_wbp_set_directions(xh_wbp *h, const double *h_g, int32_t no_mats, double threshold, int32_t diameter)
{
    XH_CHECK(h && h_g, XH_ERR_ARG, "xh_wbp_set_directions: null argument");
    XH_CHECK(no_mats >= 1 && no_mats <= (1 << 26), XH_ERR_ARG, "xh_wbp_set_directions: %d directions (1 .. %d)", no_mats, 1 << 26);
    XH_CHECK(diameter >= 1 && diameter <= h->D, XH_ERR_ARG, "xh_wbp_set_directions: diameter %d (1 .. %d: beyond the image the reference reads past its sinc table)", diameter, h->D);
    XH_CHECK(std::isfinite(threshold), XH_ERR_ARG, "xh_wbp_set_directions: the threshold is not finite");
    for (size_t c = 0; c < 4 * (size_t)no_mats; ++c) {
        XH_CHECK(std::isfinite(h_g[c]), XH_ERR_ARG, "xh_wbp_set_directions: entry %zu of direction %zu is not finite", c % 4, c / 4);
        XH_CHECK(c % 4 == 3 || std::fabs(h_g[c]) <= 1 + SY_ACC, XH_ERR_ARG, "xh_wbp_set_directions: direction %zu is no unit vector (%g)", c / 4, h_g[c]);
    }
    XH_HIP(hipSetDevice(h->ctx->device));
    h->directions = false;
    XH_TRY(xh_buf_reserve(h->ctx, h->g, sizeof(double) * 4 * (size_t)no_mats));
    XH_HIP(hipMemcpyAsync(h->g.p, h_g, sizeof(double) * 4 * (size_t)no_mats, hipMemcpyHostToDevice, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    h->no_mats = no_mats;
    h->threshold = threshold;
    h->diameter = diameter;
    h->directions = true;
    return XH_OK;
}

int xh_wbp_add(xh_wbp *h, const float *h_images, const double *h_rows, int32_t n, double *h_filtered)
{
    XH_CHECK(h && (n == 0 || (h_images && h_rows)), XH_ERR_ARG, "xh_wbp_add: null argument");
    XH_CHECK(n >= 0, XH_ERR_ARG, "xh_wbp_add: %d images", n);
    XH_CHECK(h->directions, XH_ERR_STATE, "xh_wbp_add: no directions (xh_wbp_set_directions comes first)");
    XH_HIP(hipSetDevice(h->ctx->device));
    xh_ctx *ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const int D = h->D;
    const size_t DD = h->DD;
    const double r = h->diameter / 2.;
    std::vector<WbRow> R((size_t)std::min<int>(n, h->capacity));
    const int TR = std::max(1, std::min(32, (int)(60000 / ((D + 1) * sizeof(double)))));
    const int tiles = (D + TR - 1) / TR, nseg = (D + WB_SEG - 1) / WB_SEG;
    for (int i0 = 0; i0 < n; i0 += h->capacity) {
        const int m = std::min(h->capacity, n - i0);
        bool anyGeo = false;
        for (int t = 0; t < m; ++t) {
            XH_TRY(wb_make_row("xh_wbp_add", h_rows + WB_HROW * (size_t)(i0 + t), R[t]));
            anyGeo = anyGeo || R[t].ident == 0.0;
        }
        XH_HIP(hipMemcpyAsync(h->img_in.p, h_images + DD * i0, sizeof(float) * DD * m, hipMemcpyHostToDevice, st));
        XH_HIP(hipMemcpyAsync(h->rows.p, R.data(), sizeof(WbRow) * m, hipMemcpyHostToDevice, st));
        XH_HIP(hipStreamSynchronize(st));                 // R is reused by the next batch
        XH_TRY(h->tm.start());
        if (anyGeo) {
            // produceSplineCoefficients(BSPLINE3) in doubles: rows through LDS tiles, then columns
            hipLaunchKernelGGL((k_pm_prefilter_rows<double, float>), dim3(m * tiles), dim3(64), sizeof(double) * TR * (D + 1), st, (const float *)h->img_in.p,
                               (const int *)nullptr, dp(h->coef), D, TR, (const int *)nullptr);
            hipLaunchKernelGGL((k_pm_prefilter_cols<double>), dim3((m * D + 63) / 64), dim3(64), 0, st, dp(h->coef), D, m, (const int *)nullptr);
        }
        hipLaunchKernelGGL(k_wbp_prepare, dim3((unsigned)((DD + 255) / 256), (unsigned)m), dim3(256), 0, st, (const float *)h->img_in.p, (const double *)h->coef.p,
                           (const WbRow *)h->rows.p, D, cp(h->F));
        XH_LAUNCH_CHECK();
        XH_TRY(h->tm.lap(WB_T_PREPARE));
        XH_TRY(xh_fft2d64(ctx, h->fft, cp(h->F), m, false));
        XH_TRY(h->tm.lap(WB_T_TRANSFORM));
        XH_TRY(wb_filter_launch(h, m, (unsigned long long *)h->count.p, nullptr, -1));
        XH_TRY(h->tm.lap(WB_T_FILTER));
        XH_TRY(xh_fft2d64(ctx, h->fft, cp(h->F), m, true));
        XH_LAUNCH256(ctx, xh_k_real64<double>, (unsigned)((DD * m + 255) / 256), (const xh_cd *)h->F.p, dp(h->img), DD * m);
        XH_TRY(h->tm.lap(WB_T_TRANSFORM));
        XH_LAUNCH256(ctx, k_wbp_backproject, (unsigned)((DD * nseg + 255) / 256), (const double *)h->img.p, (const WbRow *)h->rows.p, m, D, nseg, r * r, dp(h->vol));
        XH_TRY(h->tm.lap(WB_T_BACKPROJECT));
        if (h_filtered) XH_HIP(hipMemcpyAsync(h_filtered + DD * i0, h->img.p, sizeof(double) * DD * m, hipMemcpyDeviceToHost, st));
    }
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

int xh_wbp_weights(xh_wbp *h, const double *h_row, double *h_weights)
{
    XH_CHECK(h && h_row && h_weights, XH_ERR_ARG, "xh_wbp_weights: null argument");
    XH_CHECK(h->directions, XH_ERR_STATE, "xh_wbp_weights: no directions (xh_wbp_set_directions comes first)");
    WbRow R;
    XH_TRY(wb_make_row("xh_wbp_weights", h_row, R));
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    XH_HIP(hipMemcpyAsync(h->rows.p, &R, sizeof(WbRow), hipMemcpyHostToDevice, st));
    XH_HIP(hipMemsetAsync(h->F.p, 0, sizeof(xh_cd) * h->DD, st));
    XH_HIP(hipMemsetAsync(h->wscratch.p, 0, sizeof(double) * h->DD, st));
    XH_TRY(wb_filter_launch(h, 1, (unsigned long long *)h->count.p + 1, dp(h->wscratch), 0));       // its count goes beside the run's
    XH_HIP(hipMemcpyAsync(h_weights, h->wscratch.p, sizeof(double) * h->DD, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

int xh_wbp_finish(xh_wbp *h, const double *h_R, int32_t nsym)
{
    XH_CHECK(h && (h_R || nsym == 0), XH_ERR_ARG, "xh_wbp_finish: null argument");
    XH_CHECK(nsym >= 0, XH_ERR_ARG, "xh_wbp_finish: %d matrices", nsym);
    XH_CHECK(h->directions, XH_ERR_STATE, "xh_wbp_finish: no directions (xh_wbp_set_directions comes first)");
    if (nsym == 0) return XH_OK;                          // :567: without a symmetry the volume is left as the back-projection wrote it
    XH_HIP(hipSetDevice(h->ctx->device));
    if (!h->sym) XH_TRY(xh_sym_create(h->ctx, h->D, h->D, h->D, &h->sym));
    XH_TRY(xh_buf_reserve(h->ctx, h->vaux, sizeof(double) * h->N));
    XH_TRY(xh_sym_set_matrices(h->sym, h_R, nsym));
    XH_TRY(h->tm.start());
    XH_TRY(xh_sym_symmetrize(h->sym, (const double *)h->vol.p, 3, 1, 0, dp(h->vaux)));
    XH_HIP(hipMemcpyAsync(h->vol.p, h->vaux.p, sizeof(double) * h->N, hipMemcpyDeviceToDevice, h->ctx->stream));
    const double r = h->diameter / 2.;
    XH_LAUNCH256(h->ctx, k_wbp_mask, (unsigned)((h->N + 255) / 256), dp(h->vol), h->D, r * r);
    XH_TRY(h->tm.lap(WB_T_FINISH));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

int xh_wbp_volume(xh_wbp *h, double *out)
{
    XH_CHECK(h && out, XH_ERR_ARG, "xh_wbp_volume: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(out, h->vol.p, sizeof(double) * h->N, hipMemcpyDefault, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

int xh_wbp_count_thr(xh_wbp *h, int64_t *count)
{
    XH_CHECK(h && count, XH_ERR_ARG, "xh_wbp_count_thr: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    unsigned long long c = 0;
    XH_HIP(hipMemcpyAsync(&c, h->count.p, sizeof(c), hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    *count = (int64_t)c;
    return XH_OK;
}

int xh_wbp_table(const xh_wbp *h, double *h_table, int64_t *n)
{
    XH_CHECK(h && n, XH_ERR_ARG, "xh_wbp_table: null argument");
    *n = h->nelem;
    if (!h_table) return XH_OK;
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpy(h_table, h->table.p, sizeof(double) * (size_t)h->nelem, hipMemcpyDeviceToHost));
    return XH_OK;
}

int xh_wbp_image_matrices(double rot, double tilt, double psi, double *h_dir, double *h_filter, double *h_back)
{
    XH_CHECK(h_dir && h_filter && h_back, XH_ERR_ARG, "xh_wbp_image_matrices: null argument");
    XH_CHECK(std::isfinite(rot) && std::isfinite(tilt) && std::isfinite(psi), XH_ERR_ARG, "xh_wbp_image_matrices: the angles are not finite");
    double E[9];
    xh_fp_euler(rot, -tilt, psi, E);
    h_dir[0] = E[6]; h_dir[1] = E[7]; h_dir[2] = E[8];
    sy_inv3x3(E, h_back);
    xh_fp_euler(-rot, tilt, -psi, h_filter);
    return XH_OK;
}

int xh_wbp_even_distribution(double sampling, double *h_rot, double *h_tilt, int32_t capacity, int32_t *n)
{
    XH_CHECK(n, XH_ERR_ARG, "xh_wbp_even_distribution: null argument");
    XH_CHECK(std::isfinite(sampling) && sampling >= 0.5 && sampling <= 180, XH_ERR_ARG, "xh_wbp_even_distribution: a sampling of %g degrees (0.5 .. 180)", sampling);
    // make_even_distribution (directions.cpp:133-183), include_mirror, no symmetry
    const int tilt_nstep = wb_round(180. / sampling) + 1;
    const double tilt_sam = 180. / tilt_nstep;
    std::vector<double> rotList, tiltList;
    for (int tilt_step = 0; tilt_step < tilt_nstep; tilt_step++) {
        const double tilt = ((double)tilt_step / (tilt_nstep - 1)) * 180.;
        const int rot_nstep = tilt > 0 ? wb_ceil(360. * std::sin(tilt * 3.14159265358979323846 / 180.) / sampling) : 1;
        const double rot_sam = 360. / (double)rot_nstep;
        for (double rot = 0.; rot < 360.; rot += rot_sam) {
            bool append = true;
            for (size_t i = 0; i < rotList.size(); ++i)
                if (!wb_unique(rot, tilt, rotList[i], tiltList[i], rot_sam, tilt_sam)) {
                    append = false;
                    break;
                }
            if (append) {
                rotList.push_back(rot);
                tiltList.push_back(tilt);
            }
        }
    }
    *n = (int32_t)rotList.size();
    if (!h_rot || !h_tilt) return XH_OK;
    XH_CHECK(capacity >= *n, XH_ERR_ARG, "xh_wbp_even_distribution: %d directions for a capacity of %d", *n, capacity);
    std::copy(rotList.begin(), rotList.end(), h_rot);
    std::copy(tiltList.begin(), tiltList.end(), h_tilt);
    return XH_OK;
}

int xh_wbp_nearest_direction(double rot, double tilt, const double *h_rot, const double *h_tilt, int32_t n, int32_t *index)
{
    XH_CHECK(index && (n == 0 || (h_rot && h_tilt)) && n >= 0, XH_ERR_ARG, "xh_wbp_nearest_direction: bad argument");
    // find_nearest_direction (:194-237) without symmetry; distance_directions (:91-131) without mirrors
    int optdir = -1;
    double mindist = 9999.;
    for (int i = 0; i < n; ++i) {
        double dist = wb_diff(rot, tilt, h_rot[i], h_tilt[i]);
        dist = std::fmin(dist, wb_diff(rot, tilt, h_rot[i] + 180., -h_tilt[i]));
        if (dist < mindist) {
            mindist = dist;
            optdir = i;
        }
    }
    *index = optdir;
    return XH_OK;
}

int xh_wbp_tile(void) { return WB_TILE; }

int xh_wbp_set_timing(xh_wbp *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_wbp_set_timing: null handle");
    h->tm.set(on != 0);
    return XH_OK;
}

int xh_wbp_stage_ms(const xh_wbp *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_wbp_stage_ms: null argument");
    h->tm.read(h_ms);
    return XH_OK;
}

}  // extern "C"
