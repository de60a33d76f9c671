// xh_rsp.hip -- projectVolume in real space on the device (gfx950): four rays per pixel traced through the voxel grid.
// Reference: libraries/data/projection.cpp:337-589 (projectVolume), restated as written; what xmipp_subtract_projection
// (reconstruction/subtract_projection.cpp:258,280,653) uses for every mask projection of every particle.
//
//   create : value mode keeps a copy of the volume [D][D][D] (doubles, Xmipp origin). Support mode packs v > 0 into bits, one 64-bit
//            word per 64 consecutive voxels, when the volume has no negative voxel; with a negative voxel it keeps the doubles and
//            project() runs the value walk followed by > 0.
//   project: one ray per lane. The four rays of a pixel sit in adjacent lanes and a wave covers a 4 x 4 pixel tile, so a wave's rays
//            walk neighbouring voxels; a 256-thread block covers 8 x 8 pixels. Every pixel is written once by the lane of its ray 0.
//
// As written, kept: eulert and direction are the host's (xh_fp_euler), zero direction components become XMIPP_EQUAL_ACCURACY, the
// rays sit at +-1/3, the alpha range, ROUND and CLIP of the entry voxel, the smallest of diffx / diffy / diffz with the strict <
// in the order x, y, z, and the do ... while (alpha_max - alpha > XMIPP_EQUAL_ACCURACY) loop. Which voxel a ray enters next is
// decided by doubles that differ in the last bits: this file is built with -ffp-contract=off and every expression keeps the
// reference's order of operations.
//
// Deviations:
//   - The reference keeps one running ray_sum over the four rays of a pixel. Here every ray has its own sum, and the pixel is
//     ((s0 + s1) + s2) + s3 in ray order, times 0.25: the same terms, associated differently.
//   - A ray whose index leaves the volume (the reference would read outside the array) contributes 0 for that step, and a ray ends
//     after 3 D + 8 steps whatever its alpha: a ray inside the volume crosses fewer than 3 D voxel faces.
//
// Support mode is the walk above with the sum replaced by a question: it writes 1.0 when some step of some ray of the pixel has
// diff_alpha > 0 on a voxel with v > 0, else 0.0, and a ray ends at its first such step. On a volume without negative voxels this is
// value > 0: a sum of non-negative terms is positive iff one term is. (Underflow of diff_alpha * v to zero is ignored.)
#include "xh_common.h"
#include <cmath>
#include <vector>

namespace {

const int kRspPrm = 18;                  // doubles per projection: euler [9], direction [3], 1 / direction [3], roffset [2], has offset
const double kEqualAccuracy = 1e-6;      // XMIPP_EQUAL_ACCURACY

enum { RSP_SUM = 0, RSP_BITS = 1, RSP_SUM_POSITIVE = 2 };

// v > 0 of 64 consecutive voxels per word; neg[block] != 0 when the block saw a negative voxel
__global__ void __launch_bounds__(256)
k_rsp_pack(const double *__restrict__ vol, unsigned long long *__restrict__ words, int *__restrict__ neg, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double v = idx < total ? vol[idx] : 0.0;
    const unsigned long long m = __ballot(v > 0.0);
    if ((threadIdx.x & 63) == 0 && idx < total) words[idx >> 6] = m;
    const int any = __syncthreads_or(v < 0.0);
    if (threadIdx.x == 0) neg[blockIdx.x] = any;
}

// projectVolume (L387-588). Thread t of block b: projection b / (tiles * tiles), tile b % (tiles * tiles) of 8 x 8 pixels; wave w of
// the block has the 4 x 4 pixels at (w & 1, w >> 1), lane l the ray l & 3 of pixel (l >> 2) & 3, l >> 4 of them.
template <int MODE, bool STEPS>
__global__ void __launch_bounds__(256)
k_rsp_project(const double *__restrict__ vol, const unsigned long long *__restrict__ words, const double *__restrict__ prm,
              double *__restrict__ out, int *__restrict__ steps, int D, int tiles)
{
    const int per = tiles * tiles;
    const int p = blockIdx.x / per, tile = blockIdx.x - p * per;
    const int ty = tile / tiles, tx = tile - ty * tiles;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, ray = l & 3, q = l >> 2;
    const int pi = ty * 8 + (w >> 1) * 4 + (q >> 2), pj = tx * 8 + (w & 1) * 4 + (q & 3);       // physical pixel
    const bool inside = pi < D && pj < D;
    const double *P = prm + (size_t)p * kRspPrm;

    // STARTINGX .. FINISHINGX of the volume and of the projection: FIRST_XMIPP_INDEX(D) = -(D / 2)
    const int x_0 = -(D / 2), x_F = x_0 + D - 1;
    const double step = 1.0 / 3.0;
    double sum = 0.0;
    bool hit = false;
    int nsteps = 0;

    if (inside) {
        const double dirx = P[9], diry = P[10], dirz = P[11];
        const int x_sign = dirx >= 0 ? 1 : -1, y_sign = diry >= 0 ? 1 : -1, z_sign = dirz >= 0 ? 1 : -1;
        const double half_x_sign = 0.5 * x_sign, half_y_sign = 0.5 * y_sign, half_z_sign = 0.5 * z_sign;
        const double idirx = P[12], idiry = P[13], idirz = P[14];
        const int i = pi + x_0, j = pj + x_0;                  // logical
        // L395-409
        double rx = (ray & 2) ? j + step : j - step;
        double ry = (ray & 1) ? i + step : i - step;
        double rz = 0;
        if (P[17] != 0.0) { rx -= P[15]; ry -= P[16]; }
        // M3x3_BY_V3x1(p1, eulert, r_p)
        const double p1x = P[0] * rx + P[3] * ry + P[6] * rz;
        const double p1y = P[1] * rx + P[4] * ry + P[7] * rz;
        const double p1z = P[2] * rx + P[5] * ry + P[8] * rz;
        const double psx = p1x - half_x_sign, psy = p1y - half_y_sign, psz = p1z - half_z_sign;

        const double alpha_xmin = (x_0 - 0.5 - p1x) * idirx, alpha_xmax = (x_F + 0.5 - p1x) * idirx;
        const double alpha_ymin = (x_0 - 0.5 - p1y) * idiry, alpha_ymax = (x_F + 0.5 - p1y) * idiry;
        const double alpha_zmin = (x_0 - 0.5 - p1z) * idirz, alpha_zmax = (x_F + 0.5 - p1z) * idirz;
        double auxMin, auxMax;
        if (alpha_xmin < alpha_xmax) { auxMin = alpha_xmin; auxMax = alpha_xmax; } else { auxMin = alpha_xmax; auxMax = alpha_xmin; }
        double alpha_min = auxMin, alpha_max = auxMax;
        if (alpha_ymin < alpha_ymax) { auxMin = alpha_ymin; auxMax = alpha_ymax; } else { auxMin = alpha_ymax; auxMax = alpha_ymin; }
        alpha_min = fmax(auxMin, alpha_min);
        alpha_max = fmin(auxMax, alpha_max);
        if (alpha_zmin < alpha_zmax) { auxMin = alpha_zmin; auxMax = alpha_zmax; } else { auxMin = alpha_zmax; auxMax = alpha_zmin; }
        alpha_min = fmax(auxMin, alpha_min);
        alpha_max = fmin(auxMax, alpha_max);

        if (!(alpha_max - alpha_min < kEqualAccuracy)) {
            // the first voxel (L494-504)
            const double vx = p1x + dirx * alpha_min, vy = p1y + diry * alpha_min, vz = p1z + dirz * alpha_min;
            int xx = vx > 0 ? (int)(vx + 0.5) : (int)(vx - 0.5);
            int yy = vy > 0 ? (int)(vy + 0.5) : (int)(vy - 0.5);
            int zz = vz > 0 ? (int)(vz + 0.5) : (int)(vz - 0.5);
            xx = xx < x_0 ? x_0 : (xx > x_F ? x_F : xx);
            yy = yy < x_0 ? x_0 : (yy > x_F ? x_F : yy);
            zz = zz < x_0 ? x_0 : (zz > x_F ? x_F : zz);
            double alpha = alpha_min;
            const int cap = 3 * D + 8;
            do {
                const double alpha_x = ((double)xx - psx) * idirx;
                const double alpha_y = ((double)yy - psy) * idiry;
                const double alpha_z = ((double)zz - psz) * idirz;
                const double diffx = fabs(alpha - alpha_x), diffy = fabs(alpha - alpha_y), diffz = fabs(alpha - alpha_z);
                int diff_source = 0;
                double diff_alpha = diffx;
                if (diffy < diff_alpha) { diff_source = 1; diff_alpha = diffy; }
                if (diffz < diff_alpha) { diff_source = 2; diff_alpha = diffz; }
                const unsigned ux = (unsigned)(xx - x_0), uy = (unsigned)(yy - x_0), uz = (unsigned)(zz - x_0);
                if (ux < (unsigned)D && uy < (unsigned)D && uz < (unsigned)D) {
                    const size_t vi = ((size_t)uz * D + uy) * D + ux;
                    if (MODE == RSP_BITS) {
                        if (diff_alpha > 0 && ((words[vi >> 6] >> (vi & 63)) & 1ull)) hit = true;
                    } else {
                        sum += diff_alpha * vol[vi];
                    }
                }
                ++nsteps;
                if (diff_source == 0) { alpha = alpha_x; xx += x_sign; }
                else if (diff_source == 1) { alpha = alpha_y; yy += y_sign; }
                else { alpha = alpha_z; zz += z_sign; }
            } while ((alpha_max - alpha) > kEqualAccuracy && nsteps < cap && !hit);
        }
    }

    // the pixel's four rays, lanes l & ~3 .. (l & ~3) + 3; every lane of the wave arrives here
    const int base = l & ~3;
    double res;
    if (MODE == RSP_BITS) {
        const int h0 = __shfl((int)hit, base, 64), h1 = __shfl((int)hit, base + 1, 64), h2 = __shfl((int)hit, base + 2, 64),
                  h3 = __shfl((int)hit, base + 3, 64);
        res = (h0 | h1 | h2 | h3) ? 1.0 : 0.0;
    } else {
        const double s0 = __shfl(sum, base, 64), s1 = __shfl(sum, base + 1, 64), s2 = __shfl(sum, base + 2, 64),
                     s3 = __shfl(sum, base + 3, 64);
        res = (((s0 + s1) + s2) + s3) * 0.25;
        if (MODE == RSP_SUM_POSITIVE) res = res > 0 ? 1.0 : 0.0;
    }
    int ns = 0;
    if (STEPS) ns = __shfl(nsteps, base, 64) + __shfl(nsteps, base + 1, 64) + __shfl(nsteps, base + 2, 64) + __shfl(nsteps, base + 3, 64);
    if (inside && ray == 0) {
        const size_t o = ((size_t)p * D + pi) * D + pj;
        if (STEPS) steps[o] = ns;
        else out[o] = res;
    }
}

}  // namespace

struct xh_rsp {
    xh_ctx *ctx;
    int D, mode;
    bool packed;                 // support mode on bits
    XhBuf d_vol, d_words, d_prm;
    ~xh_rsp()
    {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
};

// the per-projection constants of L345-376 on the host, so that sines, cosines and the reciprocals are the host's
static void rsp_params(const double *ang, const double *off, double *P)
{
    xh_fp_euler(ang[0], ang[1], ang[2], P);
    for (int c = 0; c < 3; ++c) {
        double d = P[6 + c];                                    // direction = row 2 of euler
        if (d == 0) d = kEqualAccuracy;
        P[9 + c] = d;
        P[12 + c] = 1.0 / d;
    }
    P[15] = off ? off[0] : 0.0;
    P[16] = off ? off[1] : 0.0;
    P[17] = off ? 1.0 : 0.0;
}

static int rsp_run(xh_rsp *h, const double *h_angles, const double *h_offsets, int32_t n, double *d_out, int32_t *d_steps)
{
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    if (n == 0) return XH_OK;
    for (size_t k = 0; k < (size_t)3 * n; ++k)
        XH_CHECK(std::isfinite(h_angles[k]), XH_ERR_ARG, "xh_rsp_project: angle %zu of projection %zu is not finite", k % 3, k / 3);
    for (size_t k = 0; h_offsets && k < (size_t)2 * n; ++k)
        XH_CHECK(std::isfinite(h_offsets[k]), XH_ERR_ARG, "xh_rsp_project: offset %zu of projection %zu is not finite", k % 2, k / 2);
    const int D = h->D, tiles = (D + 7) / 8;
    const int chunk = std::min(n, 4096);                       // 4096 projections x (1024 / 8)^2 tiles: 2^26 blocks at the most
    XH_TRY(xh_buf_reserve(ctx, h->d_prm, sizeof(double) * kRspPrm * (size_t)chunk));
    std::vector<double> P((size_t)kRspPrm * chunk);
    const int mode = h->mode == XH_RSP_VALUE ? RSP_SUM : (h->packed ? RSP_BITS : RSP_SUM_POSITIVE);
    for (int p0 = 0; p0 < n; p0 += chunk) {
        const int m = std::min(chunk, n - p0);
        for (int p = 0; p < m; ++p)
            rsp_params(h_angles + 3 * (size_t)(p0 + p), h_offsets ? h_offsets + 2 * (size_t)(p0 + p) : nullptr, &P[(size_t)kRspPrm * p]);
        XH_HIP(hipMemcpyAsync(h->d_prm.p, P.data(), sizeof(double) * kRspPrm * m, hipMemcpyHostToDevice, ctx->stream));
        XH_HIP(hipStreamSynchronize(ctx->stream));
        const dim3 grid((unsigned)((size_t)m * tiles * tiles));
        const double *vol = (const double *)h->d_vol.p, *prm = (const double *)h->d_prm.p;
        const unsigned long long *words = (const unsigned long long *)h->d_words.p;
        double *out = d_out ? d_out + (size_t)p0 * D * D : nullptr;
        int *st = d_steps ? d_steps + (size_t)p0 * D * D : nullptr;
#define RSP_LAUNCH(MODE, STEPS) hipLaunchKernelGGL((k_rsp_project<MODE, STEPS>), grid, dim3(256), 0, ctx->stream, vol, words, prm, out, st, D, tiles)
        if (d_steps) {
            if (mode == RSP_BITS) RSP_LAUNCH(RSP_BITS, true);
            else RSP_LAUNCH(RSP_SUM, true);
        } else if (mode == RSP_SUM) RSP_LAUNCH(RSP_SUM, false);
        else if (mode == RSP_BITS) RSP_LAUNCH(RSP_BITS, false);
        else RSP_LAUNCH(RSP_SUM_POSITIVE, false);
#undef RSP_LAUNCH
        XH_LAUNCH_CHECK();
    }
    return XH_OK;
}

extern "C" {

int xh_rsp_create(xh_ctx *ctx, const double *d_vol, int32_t D, int32_t mode, xh_rsp **out)
{
    XH_CHECK(ctx && d_vol && out, XH_ERR_ARG, "xh_rsp_create: bad argument");
    XH_CHECK(D >= 1 && D <= 1024, XH_ERR_ARG, "xh_rsp_create: volume side %d outside 1 .. 1024", D);
    XH_CHECK(mode == XH_RSP_VALUE || mode == XH_RSP_SUPPORT, XH_ERR_ARG, "xh_rsp_create: unknown mode %d", mode);
    XH_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<xh_rsp> h(new xh_rsp);
    h->ctx = ctx; h->D = D; h->mode = mode; h->packed = false;
    const size_t total = (size_t)D * D * D;
    if (mode == XH_RSP_SUPPORT) {
        const size_t nblocks = (total + 255) / 256;
        XhBuf d_neg;
        XH_TRY(xh_buf_alloc(ctx, h->d_words, sizeof(unsigned long long) * ((total + 63) / 64)));
        XH_TRY(xh_buf_alloc(ctx, d_neg, sizeof(int) * nblocks));
        hipLaunchKernelGGL(k_rsp_pack, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, d_vol, (unsigned long long *)h->d_words.p,
                           (int *)d_neg.p, total);
        XH_LAUNCH_CHECK();
        std::vector<int> neg(nblocks);
        XH_HIP(hipMemcpyAsync(neg.data(), d_neg.p, sizeof(int) * nblocks, hipMemcpyDeviceToHost, ctx->stream));
        XH_HIP(hipStreamSynchronize(ctx->stream));
        h->packed = true;
        for (int f : neg) if (f) { h->packed = false; break; }
        if (!h->packed) xh_buf_free(h->d_words);
    }
    if (!h->packed) {
        XH_TRY(xh_buf_alloc(ctx, h->d_vol, sizeof(double) * total));
        XH_HIP(hipMemcpyAsync(h->d_vol.p, d_vol, sizeof(double) * total, hipMemcpyDeviceToDevice, ctx->stream));
        XH_HIP(hipStreamSynchronize(ctx->stream));
    }
    *out = h.release();
    return XH_OK;
}

int xh_rsp_destroy(xh_rsp *h)
{
    delete h;
    return XH_OK;
}

int xh_rsp_info(const xh_rsp *h, int32_t *D, int32_t *mode, int32_t *packed)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_rsp_info: null handle");
    if (D) *D = h->D;
    if (mode) *mode = h->mode;
    if (packed) *packed = h->packed ? 1 : 0;
    return XH_OK;
}

int xh_rsp_project(xh_rsp *h, const double *h_angles, const double *h_offsets, int32_t n, double *d_out)
{
    XH_CHECK(h && n >= 0 && (n == 0 || (h_angles && d_out)), XH_ERR_ARG, "xh_rsp_project: bad argument");
    return rsp_run(h, h_angles, h_offsets, n, d_out, nullptr);
}

int xh_rsp_steps(xh_rsp *h, const double *h_angles, const double *h_offsets, int32_t n, int32_t *d_steps)
{
    XH_CHECK(h && n >= 0 && (n == 0 || (h_angles && d_steps)), XH_ERR_ARG, "xh_rsp_steps: bad argument");
    return rsp_run(h, h_angles, h_offsets, n, nullptr, d_steps);
}

}  // extern "C"
