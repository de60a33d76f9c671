// xh_faz.hip -- xmipp_forward_art_zernike3d on the device (gfx950), fp64: ART reconstruction of the undeformed ("canonical") volume from
// particles that each carry a pose and a Zernike3D deformation (the rows xmipp_angular_sph_alignment writes).
// Reference: reconstruction_adapt_cuda11/forward_art_zernike3d_gpu.cpp (preProcess L175-380, processImage L389-458, run L520-626,
// sortOrthogonal L628-690, artModel L704-805) and reconstruction_cuda11/cuda_forward_art_zernike3d.{cpp,cu} (the mask's coordinate list
// cpp L230-265, runForwardKernel / runBackwardKernel cpp L330-483, the kernels cu L1039-1376). The reference allocates, uploads, runs one
// kernel, downloads P and W, filters them on the host, uploads Idiff and Iws and frees everything for every image; here the volume V, the
// regulariser's fields Dx, Dy, Dz, Dl1 and Reg never leave the device and a sweep over many images is one stream of kernels.
//
// Per presentation of an image (an image is presented once per symmetry matrix, the identity first):
//   k_faz_splat  : forwardKernel. One workgroup per 16^3 brick of the list that create builds from maskF and --step (bricks without a
//                  voxel are dropped; with several sigmas one list entry per (brick, sigma)). The workgroup projects the brick's deformed
//                  centre and keeps a 48 x 48 tile of (P, W) around it in LDS (36 KB); a voxel at logical (k, i, j) with weight V(k, i, j)
//                  goes to pos = R ((j, i, k) + g), g = sum c Z((j, i, k) / RDef) (vds_disp of xh_zernike.h), pixel (i', j') =
//                  round-half-away(pos_y, pos_x), gw = 1 - a - b + ab with a = |i' - pos_y| / step, b = |j' - pos_x| / step,
//                  P(i', j') += weight gw, W(i', j') += gw^2: an LDS atomic when the pixel is in the tile, a global atomic otherwise
//                  (large deformations). The tile's non-zero entries are added to the global planes at the end, consecutive lanes on
//                  consecutive pixels of a tile row. A position that is not finite contributes nothing (tested before any conversion to
//                  int); every global index is range-checked against the image. Rotation and coefficients come from the presentation's
//                  row through a workgroup-uniform pointer at compile-time offsets, as in k_asa_project. Instantiated on (L1, L2) like
//                  k_asa_project, on the row's effective l2, plus an instantiation without deformation.
//                  THE SUMS DEPEND ON ARRIVAL ORDER IN THEIR LAST BITS: P and W are sums of up to ~2 D terms per pixel added by atomics.
//   filter       : P_s times exp(-2 pi^2 w^2 sigma_s^2) (REALGAUSSIANZ), W_s times exp(-pi^2 w^2 sigma_s^2) / (4 pi sigma_s^2)
//                  (REALGAUSSIANZ2), w the digital frequency: all planes of all sigmas in one batched transform pair (XhFft2d64).
//   k_faz_residual: diff = I_shifted - sum c_s P_s, sumMw = sum c_s^2 W_s (c_s = sigma_s^2 with several sigmas, else 1); where sumMw > 0:
//                  Idiff = lambda diff, Iws = max(sumMw, 1), and the pixel counts in error = sqrt(sum diff^2 / N); block partials in a
//                  fixed order (xh_reduce.h), reduced per presentation at the end of the sweep.
//   k_faz_tv, k_faz_dtv: computeTV and computeDTV exactly as written, with 0.5 next - prev (not 0.5 (next - prev)), the Dz Dx product in
//                  grad_x2, Dl1 = lst where V > 0 and ll1 V where V < 0, entries of Dx, Dy, Dz, Dl1 written only under their conditions
//                  and never cleared. Reg = -lambda (ltv div + ltk div2 + Dl1) inside maskB.
//   k_faz_back   : backwardKernel over maskB at step 1: V += bilinear(Idiff, pos) / (bilinear(Iws, pos) + 1e-5) + Reg, taps outside the
//                  image 0. The displacement is recomputed, no D^3 cache of positions.
// The particles are prepared once per load (step 4): the CTFINV filter (xh_k_ctfinv of xh_image2d.h) when the row has a CTF and
// --useCTF is given, then applyGeometry LINEAR with the shift and the flip (d_ca2_linear).
//
// Deviations from the reference:
//  - Arithmetic: fp64 throughout (the reference instantiates float only), Euler matrices from double angles.
//  - Symmetry: with symmetry the rotation is E R_sym itself, not the matrix of the angles extracted from it (Euler_apply_transf L446).
//    The left matrices are the identity for every group this library builds.
//  - Particle preparation happens once per image; the reference filters I again and negates A again for every symmetry matrix
//    (L734-744). For c1 the results are the reference's.
//  - minCTF is never set for this filter in the reference (an uninitialised member); here it is 0.05, the default of the ctfinv
//    filter's own option.
//  - --phaseFlipped takes the absolute value of the CTF before it is inverted. The reference calls correctPhase() on the previous
//    image's mask and then overwrites it, so the flag does nothing there. Without the flag the outputs are unchanged.
//  - A maskF value that matches no sigma skips the voxel; the reference indexes past its plane array.
//  - sphCoefficients must hold exactly 3 vecSize values; any other count is an error that names both numbers.
//  - A row without the `enabled` label is enabled.
//  - 2-D images above 1024 x 1024 are refused; the reference silently builds no filter mask for them.
//  - Degrees above l1 = 5, l2 = 4 are XH_ERR_UNSUPPORTED, as in xh_vds and xh_asa; the volume is a cube of the images' side.
//  - The _small images, --mr and --dSize reach no arithmetic in the reference (their reads are commented out, cu L1257-1258): nothing
//    is computed for them.
#include "xh_common.h"
#include "xh_fft.h"
#include "xh_plan.h"
#include "xh_reduce.h"
#include "xh_ctf.h"
#include "xh_image2d.h"
#include "xh_zernike.h"
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace {
// doubles per presentation row on the device: R[9], the coefficients in VdsCoef's layout [3 * 45], Ainv[6], identity, CTF (0 none, 1
// computed from the CtfSide that follows), CtfSide[18]
const int kRowCoef = 9, kRowA = kRowCoef + 3 * VDS_MAXT, kRowIdent = kRowA + 6, kRowCtf = kRowIdent + 1, kRowSide = kRowCtf + 1,
          kRow = kRowSide + 18;
static_assert(sizeof(VdsCoef) == 3 * VDS_MAXT * sizeof(double), "VdsCoef rides in a presentation row");
const int kBrick = 16, kTile = 48, kMaxSigma = 8;
const int FAZ_NODEF = -2;      // the L1 of the instantiations without deformation
const double kMinCTF = 0.05;

struct FazBrick { int x, y, z, plane, value; };      // physical origin, the (P, W) pair, the maskF value that selects the voxel

struct FazGeom {
    int D, DD, c, step, multi;      // multi: several sigmas, a voxel belongs to the sigma its maskF value equals
    double iRDef, istep;
};

// pos = R ((j, i, k) + g), first two rows
template <int L1, int L2>
__device__ __forceinline__ void faz_pos(const double *__restrict__ q, int l1, int l2, double iRDef, int k, int i, int j, double &px, double &py)
{
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if constexpr (L1 != FAZ_NODEF) {
        const VdsCoef &C = *reinterpret_cast<const VdsCoef *>(q + kRowCoef);
        const double r2 = (double)(k * k + i * i + j * j);
        vds_disp<L1, L2>(C, l1, l2, j * iRDef, i * iRDef, k * iRDef, sqrt(r2) * iRDef, gx, gy, gz);
    }
    const double rx = j + gx, ry = i + gy, rz = k + gz;
    px = q[0] * rx + q[1] * ry + q[2] * rz;
    py = q[3] * rx + q[4] * ry + q[5] * rz;
}

// forwardKernel + splattingAtPos (cu L1039-1057, L1112-1190): see the header. planes: P_s at [s], W_s at [nsigma + s], each [D][D]
template <int L1, int L2>
__global__ void __launch_bounds__(256)
k_faz_splat(const double *__restrict__ V, const int *__restrict__ maskF, const FazBrick *__restrict__ bricks, const double *__restrict__ q,
            const FazGeom g, int l1, int l2, int nsigma, double *__restrict__ planes)
{
    __shared__ double tP[kTile * kTile], tW[kTile * kTile];
    const FazBrick b = bricks[blockIdx.x];
    const int tid = threadIdx.x, D = g.D, c = g.c;
    for (int e = tid; e < kTile * kTile; e += 256) { tP[e] = 0.0; tW[e] = 0.0; }
    // the tile's origin (logical pixel of its first entry): around the projection of the brick's deformed centre, clipped to the volume
    int ti0 = 0, tj0 = 0;
    {
        const int ck = min(b.z + kBrick / 2, D - 1) - c, ci = min(b.y + kBrick / 2, D - 1) - c, cj = min(b.x + kBrick / 2, D - 1) - c;
        double cx, cy;
        faz_pos<L1, L2>(q, l1, l2, g.iRDef, ck, ci, cj, cx, cy);
        if (fabs(cx) < 1e6 && fabs(cy) < 1e6) { ti0 = (int)round(cy) - kTile / 2; tj0 = (int)round(cx) - kTile / 2; }
    }
    __syncthreads();
    double *__restrict__ P = planes + (size_t)b.plane * g.DD, *__restrict__ W = planes + (size_t)(nsigma + b.plane) * g.DD;
    const int pj = b.x + (tid & 15), pi = b.y + (tid >> 4);
    if (pj < D && pi < D && pj % g.step == 0 && pi % g.step == 0) {
        const int i = pi - c, j = pj - c;
        for (int z = 0; z < kBrick; ++z) {
            const int pk = b.z + z;
            if (pk >= D) break;
            if (pk % g.step != 0) continue;
            const size_t n = ((size_t)pk * D + pi) * D + pj;
            const int mv = maskF[n];
            if (g.multi ? mv != b.value : mv == 0) continue;
            const double weight = V[n];
            double px, py;
            faz_pos<L1, L2>(q, l1, l2, g.iRDef, pk - c, i, j, px, py);
            if (!(fabs(px) < 1e6 && fabs(py) < 1e6)) continue;      // not finite, or far outside any image
            const double ry = round(py), rx = round(px);
            const int ii = (int)ry, jj = (int)rx;
            if (ii < -c || ii > D - 1 - c || jj < -c || jj > D - 1 - c) continue;      // IS_OUTSIDE2D
            const double a = g.istep * fabs(ry - py), bb = g.istep * fabs(rx - px);
            const double gw = 1.0 - a - bb + a * bb;
            const int ti = ii - ti0, tj = jj - tj0;
            if (ti >= 0 && ti < kTile && tj >= 0 && tj < kTile) {
                atomicAdd(&tP[ti * kTile + tj], weight * gw);
                atomicAdd(&tW[ti * kTile + tj], gw * gw);
            } else {
                const size_t o = (size_t)(ii + c) * D + (jj + c);
                atomicAdd(&P[o], weight * gw);
                atomicAdd(&W[o], gw * gw);
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < kTile * kTile; e += 256) {
        const double w = tW[e];
        if (w == 0.0) continue;      // gw > 0 for every voxel that landed here
        const int ti = e / kTile, tj = e - ti * kTile;
        const int oi = ti0 + ti + c, oj = tj0 + tj + c;
        if (oi < 0 || oi >= D || oj < 0 || oj >= D) continue;
        const size_t o = (size_t)oi * D + oj;
        atomicAdd(&P[o], tP[e]);
        atomicAdd(&W[o], w);
    }
}

// the Gaussian filters of artModel L727-732 on the spectra F [2 nsigma][D][D], the 1 / D^2 of the forward transform folded in
struct FazSigmas { double s[kMaxSigma]; };
__global__ void __launch_bounds__(256)
k_faz_filter(xh_cd *__restrict__ F, size_t total, int D, int nsigma, const FazSigmas sig)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = idx % D, i = (idx / D) % D, p = (int)(idx / ((size_t)D * D));
    const double fy = d_digfreq(i, D), fx = d_digfreq(j, D);
    const double absw = sqrt(fx * fx + fy * fy);
    const double w1 = sig.s[p < nsigma ? p : p - nsigma];
    double m;
    if (p < nsigma) m = exp(-2. * VDS_PI * VDS_PI * absw * absw * w1 * w1);
    else m = (1. / (4 * VDS_PI * w1 * w1)) * exp(-VDS_PI * VDS_PI * absw * absw * w1 * w1);
    m /= (double)D * (double)D;
    const xh_cd v = F[idx];
    F[idx] = xh_cd{v.x * m, v.y * m};
}

// artModel L755-780 on the filtered planes (the real parts of F). partials [2][gridDim.x]: sum diff^2 and N
__global__ void __launch_bounds__(256)
k_faz_residual(const xh_cd *__restrict__ F, const double *__restrict__ Is, int DD, int nsigma, const FazSigmas sig, double lambda,
               double *__restrict__ Idiff, double *__restrict__ Iws, double *__restrict__ partials)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    double acc[2] = {0.0, 0.0};
    if (n < DD) {
        double diff = Is[n], sumMw = 0.0;
        for (int s = 0; s < nsigma; ++s) {
            const double cs = nsigma > 1 ? sig.s[s] * sig.s[s] : 1.0;
            diff -= cs * F[(size_t)s * DD + n].x;
            sumMw += cs * cs * F[(size_t)(nsigma + s) * DD + n].x;
        }
        double d = 0.0, w = 0.0;
        if (sumMw > 0.0) {
            d = lambda * diff;
            w = fmax(sumMw, 1.0);
            acc[0] = diff * diff;
            acc[1] = 1.0;
        }
        Idiff[n] = d;
        Iws[n] = w;
    }
    xh_block_partials(acc, partials);
}

// the partials of `count` presentations [count][2][tiles] -> errors [count] = sqrt(sum diff^2 / N), one workgroup each
__global__ void __launch_bounds__(256)
k_faz_errors(const double *__restrict__ partials, int tiles, double *__restrict__ errors)
{
    __shared__ double red[1][256];
    const double *p = partials + (size_t)blockIdx.x * 2 * tiles;
    double tot[2];
    for (int cix = 0; cix < 2; ++cix) {
        double v = 0.0;
        for (int t = threadIdx.x; t < tiles; t += 256) v += p[(size_t)cix * tiles + t];
        tot[cix] = xh_block_sum(v, red);
    }
    if (threadIdx.x == 0) errors[blockIdx.x] = sqrt(tot[0] / tot[1]);
}

// computeTV (cu L1318-1348), as written
__global__ void __launch_bounds__(256)
k_faz_tv(const double *__restrict__ V, const int *__restrict__ maskB, int D, size_t N, double ll1, double lst, double *__restrict__ Dx,
         double *__restrict__ Dy, double *__restrict__ Dz, double *__restrict__ Dl1)
{
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N || maskB[n] == 0) return;
    const int pj = n % D, pi = (n / D) % D, pk = (int)(n / ((size_t)D * D));
    const size_t sy = (size_t)D, sz = (size_t)D * D;
    const bool inx = pj > 0 && pj < D - 1, iny = pi > 0 && pi < D - 1, inz = pk > 0 && pk < D - 1;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (inx) gx = 0.5 * V[n + 1] - V[n - 1];
    if (iny) gy = 0.5 * V[n + sy] - V[n - sy];
    if (inz) gz = 0.5 * V[n + sz] - V[n - sz];
    const double magnitude = sqrt(gx * gx + gy * gy + gz * gz + 1e-5);
    if (inx) Dx[n] = gx / magnitude;
    if (iny) Dy[n] = gy / magnitude;
    if (inz) Dz[n] = gz / magnitude;
    const double v = V[n];
    if (v > 0.0) Dl1[n] = lst * 1.0;
    if (v < 0.0) Dl1[n] = ll1 * 1.0 * v;
}

// computeDTV (cu L1350-1376), as written
__global__ void __launch_bounds__(256)
k_faz_dtv(const double *__restrict__ Dx, const double *__restrict__ Dy, const double *__restrict__ Dz, const double *__restrict__ Dl1,
          const int *__restrict__ maskB, int D, size_t N, double lambda, double ltv, double ltk, double *__restrict__ Reg)
{
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N || maskB[n] == 0) return;
    const int pj = n % D, pi = (n / D) % D, pk = (int)(n / ((size_t)D * D));
    const size_t sy = (size_t)D, sz = (size_t)D * D;
    const bool inx = pj > 0 && pj < D - 1, iny = pi > 0 && pi < D - 1, inz = pk > 0 && pk < D - 1;
    double gx = 0.0, gy = 0.0, gz = 0.0, gx2 = 0.0, gy2 = 0.0, gz2 = 0.0;
    if (inx) {
        gx = 0.5 * Dx[n + 1] - Dx[n - 1];
        gx2 = 0.5 * Dz[n + 1] * Dx[n + 1] - Dx[n - 1] * Dx[n - 1];
    }
    if (iny) {
        gy = 0.5 * Dy[n + sy] - Dy[n - sy];
        gy2 = 0.5 * Dy[n + sy] * Dy[n + sy] - Dy[n - sy] * Dy[n - sy];
    }
    if (inz) {
        gz = 0.5 * Dz[n + sz] - Dz[n - sz];
        gz2 = 0.5 * Dz[n + sz] * Dz[n + sz] - Dz[n - sz] * Dz[n - sz];
    }
    const double divergence = gx + gy + gz, divergence2 = 2.0 * (gx2 + gy2 + gz2);
    Reg[n] = -lambda * (ltv * divergence + ltk * divergence2 + Dl1[n]);
}

// interpolatedElement2DCuda (cu L1073-1105) at the logical (x, y), both finite and within 1e6; taps outside the image are 0
__device__ __forceinline__ double faz_interp2(const double *__restrict__ I, int D, int c, double x, double y)
{
    const double fx0 = floor(x), fy0 = floor(y);
    const double fx = x - fx0, fy = y - fy0;
    const int x0 = (int)fx0 + c, y0 = (int)fy0 + c;      // physical
    const bool xa = x0 >= 0 && x0 < D, xb = x0 + 1 >= 0 && x0 + 1 < D, ya = y0 >= 0 && y0 < D, yb = y0 + 1 >= 0 && y0 + 1 < D;
    const double *p = I + ((ptrdiff_t)y0 * D + x0);
    const double d00 = (ya && xa) ? p[0] : 0.0, d01 = (ya && xb) ? p[1] : 0.0;
    const double d10 = (yb && xa) ? p[D] : 0.0, d11 = (yb && xb) ? p[D + 1] : 0.0;
    const double d0 = d00 + (d01 - d00) * fx, d1 = d10 + (d11 - d10) * fx;
    return d0 + (d1 - d0) * fy;
}

// backwardKernel (cu L1195-1263): see the header
template <int L1, int L2>
__global__ void __launch_bounds__(256)
k_faz_back(double *__restrict__ V, const int *__restrict__ maskB, const double *__restrict__ Reg, const double *__restrict__ Idiff,
           const double *__restrict__ Iws, const double *__restrict__ q, const FazGeom g, size_t N, int l1, int l2)
{
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N || maskB[n] == 0) return;
    const int D = g.D, c = g.c;
    const int pj = n % D, pi = (n / D) % D, pk = (int)(n / ((size_t)D * D));
    double px, py;
    faz_pos<L1, L2>(q, l1, l2, g.iRDef, pk - c, pi - c, pj - c, px, py);
    double voxel = 0.0, weight = 0.0;
    if (fabs(px) < 1e6 && fabs(py) < 1e6) {      // a position that is not finite has every tap outside
        voxel = faz_interp2(Idiff, D, c, px, py);
        weight = faz_interp2(Iws, D, c, px, py);
    }
    V[n] += (voxel / (weight + 1e-5)) + Reg[n];
}

// step 4's applyGeometry (artModel L740-752) of every loaded image: out [n][D][D] from the CTF-corrected images in [n][D][D]
__global__ void __launch_bounds__(256)
k_faz_shift(const double *__restrict__ in, const double *__restrict__ rows, int stride, size_t total, int D, double *__restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t DD = (size_t)D * D, img = idx / DD;
    const int n = (int)(idx - img * DD), i = n / D, j = n - i * D;
    const double *q = rows + (size_t)stride * img;
    double A[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) A[k] = q[kRowA + k];
    const double *V1 = in + img * DD;
    out[idx] = q[kRowIdent] != 0.0 ? V1[n] : d_ca2_linear(V1, D, A, i, j);
}
}  // namespace

namespace {
// the stages a timed sweep reports (xh_faz_stage_ms)
enum { FAZ_T_SPLAT, FAZ_T_FILTER, FAZ_T_RESIDUAL, FAZ_T_REGULARISER, FAZ_T_BACK, FAZ_NT };
}  // namespace

struct xh_faz {
    xh_ctx *ctx = nullptr;
    xh_faz_params prm;
    FazGeom g = {};
    FazSigmas sig = {};
    int D = 0, nsigma = 0, nsym = 0, per = 1, nbricks = 0, vecSize = 0, tiles = 0, nloaded = 0;
    double RDef = 0;
    bool timing = false;                // a sweep records events around its stages
    double stage_ms[FAZ_NT] = {};       // of the last timed sweep, summed over its presentations
    std::vector<double> sym;            // [nsym][9]
    std::vector<int> effl2;             // per loaded image: the instantiation's l2
    XhBuf d_V, d_Dx, d_Dy, d_Dz, d_Dl1, d_Reg, d_maskF, d_maskB, d_bricks;
    XhBuf d_rows, d_Is, d_planes, d_F, d_Idiff, d_Iws, d_partials, d_errors;
    XhFft2d64 fft;
    ~xh_faz()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
};

namespace {
// steps 2-5 for presentation s of image img; partials: where the residual's block partials go; ev (nullable): the presentation's
// FAZ_NT + 1 events, of which [0 .. FAZ_T_RESIDUAL + 1) are recorded here
int faz_forward(xh_faz *h, int img, int s, double *partials, const XhEvent *ev = nullptr)
{
    xh_ctx *ctx = h->ctx;
    const int S = h->nsigma, D = h->D;
    const size_t DD = (size_t)D * D, total = DD * 2 * S;
    double *planes = (double *)h->d_planes.p;
    xh_cd *F = (xh_cd *)h->d_F.p;
    const double *q = (const double *)h->d_rows.p + (size_t)kRow * ((size_t)img * h->per + s);
    if (ev) XH_HIP(hipEventRecord(ev[FAZ_T_SPLAT], ctx->stream));
    XH_HIP(hipMemsetAsync(planes, 0, sizeof(double) * total, ctx->stream));
    if (h->nbricks > 0) {
        const double *V = (const double *)h->d_V.p;
        const int *M = (const int *)h->d_maskF.p;
        const FazBrick *B = (const FazBrick *)h->d_bricks.p;
        const int l1 = h->prm.l1, l2 = h->effl2[img];
#define FAZ_SPLAT(A, B_)                                                                                                            \
    do {                                                                                                                            \
        hipLaunchKernelGGL((k_faz_splat<A, B_>), dim3((unsigned)h->nbricks), dim3(256), 0, ctx->stream, V, M, B, q, h->g, l1, l2, S, planes); \
        XH_LAUNCH_CHECK();                                                                                                          \
    } while (0)
        if (!h->prm.use_zernike) FAZ_SPLAT(FAZ_NODEF, 0);
        else ZK_DISPATCH(l1, l2, FAZ_SPLAT);
#undef FAZ_SPLAT
    }
    if (ev) XH_HIP(hipEventRecord(ev[FAZ_T_FILTER], ctx->stream));
    const unsigned gr = (unsigned)((total + 255) / 256);
    XH_LAUNCH256(ctx, xh_k_to_complex64<double>, gr, (const double *)planes, F, total);
    XH_TRY(xh_fft2d64(ctx, h->fft, F, 2 * S, false));
    XH_LAUNCH256(ctx, k_faz_filter, gr, F, total, D, S, h->sig);
    XH_TRY(xh_fft2d64(ctx, h->fft, F, 2 * S, true));
    if (ev) XH_HIP(hipEventRecord(ev[FAZ_T_RESIDUAL], ctx->stream));
    XH_LAUNCH256(ctx, k_faz_residual, h->tiles, (const xh_cd *)F, (const double *)h->d_Is.p + DD * img, (int)DD, S, h->sig, h->prm.lambda,
                 (double *)h->d_Idiff.p, (double *)h->d_Iws.p, partials);
    if (ev) XH_HIP(hipEventRecord(ev[FAZ_T_REGULARISER], ctx->stream));
    return XH_OK;
}

// steps 6-7 for presentation s of image img; ev as in faz_forward, [FAZ_T_BACK, FAZ_NT] are recorded here
int faz_backward(xh_faz *h, int img, int s, const XhEvent *ev = nullptr)
{
    xh_ctx *ctx = h->ctx;
    const int D = h->D;
    const size_t N = (size_t)D * D * D;
    const unsigned gr = (unsigned)((N + 255) / 256);
    double *V = (double *)h->d_V.p, *Reg = (double *)h->d_Reg.p;
    const int *MB = (const int *)h->d_maskB.p;
    const double *q = (const double *)h->d_rows.p + (size_t)kRow * ((size_t)img * h->per + s);
    XH_LAUNCH256(ctx, k_faz_tv, gr, (const double *)V, MB, D, N, h->prm.ll1, h->prm.lst, (double *)h->d_Dx.p, (double *)h->d_Dy.p,
                 (double *)h->d_Dz.p, (double *)h->d_Dl1.p);
    XH_LAUNCH256(ctx, k_faz_dtv, gr, (const double *)h->d_Dx.p, (const double *)h->d_Dy.p, (const double *)h->d_Dz.p,
                 (const double *)h->d_Dl1.p, MB, D, N, h->prm.lambda, h->prm.ltv, h->prm.ltk, Reg);
    if (ev) XH_HIP(hipEventRecord(ev[FAZ_T_BACK], ctx->stream));
    const double *Idiff = (const double *)h->d_Idiff.p, *Iws = (const double *)h->d_Iws.p;
    const int l1 = h->prm.l1, l2 = h->effl2[img];
#define FAZ_BACK(A, B_)                                                                                                                   \
    do {                                                                                                                                  \
        hipLaunchKernelGGL((k_faz_back<A, B_>), dim3(gr), dim3(256), 0, ctx->stream, V, MB, (const double *)Reg, Idiff, Iws, q, h->g, N, l1, l2); \
        XH_LAUNCH_CHECK();                                                                                                                \
    } while (0)
    if (!h->prm.use_zernike) FAZ_BACK(FAZ_NODEF, 0);
    else ZK_DISPATCH(l1, l2, FAZ_BACK);
#undef FAZ_BACK
    if (ev) XH_HIP(hipEventRecord(ev[FAZ_NT], ctx->stream));
    return XH_OK;
}

int faz_load(xh_faz *h, const float *h_images, int32_t n, const xh_faz_row *rows, const double *h_coef)
{
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const int D = h->D, per = h->per, vs = h->vecSize;
    const size_t DD = (size_t)D * D;
    std::vector<double> hr((size_t)kRow * n * per, 0.0);
    h->effl2.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        const xh_faz_row &r = rows[i];
        const double v[5] = {r.rot, r.tilt, r.psi, r.shift_x, r.shift_y};
        for (double x : v) XH_CHECK(std::isfinite(x), XH_ERR_ARG, "xh_faz_load: particle %d has a non-finite pose", i);
        const bool ctf = r.has_ctf && h->prm.use_ctf;
        if (ctf) {
            const double *c = reinterpret_cast<const double *>(&r.ctf);
            for (size_t k = 0; k < sizeof(xh_ctf_params) / sizeof(double); ++k)
                XH_CHECK(std::isfinite(c[k]), XH_ERR_ARG, "xh_faz_load: particle %d has a non-finite CTF parameter", i);
        }
        double E[9];
        xh_fp_euler(r.rot, r.tilt, r.psi, E);
        double *row0 = &hr[(size_t)kRow * i * per];
        if (h->prm.use_zernike) {
            const double *x = h_coef + (size_t)3 * vs * i;
            for (int k = 0; k < 3 * vs; ++k) XH_CHECK(std::isfinite(x[k]), XH_ERR_ARG, "xh_faz_load: particle %d has a non-finite coefficient", i);
            h->effl2[i] = zk_pack(h->prm.l1, h->prm.l2, vs, x, row0 + kRowCoef);
        }
        for (int a = 0; a < 9; ++a) row0[a] = E[a];
        // A (processImage L425-430, artModel L740-744): the identity with the shift, its first row negated by the flip; inverted for IS_NOT_INV
        const double f = r.flip ? -1.0 : 1.0;
        double *A = row0 + kRowA;
        A[0] = f; A[1] = 0; A[2] = -r.shift_x; A[3] = 0; A[4] = 1; A[5] = -r.shift_y;
        row0[kRowIdent] = (!r.flip && std::fabs(r.shift_x) <= kAcc && std::fabs(r.shift_y) <= kAcc) ? 1.0 : 0.0;
        row0[kRowCtf] = 0;
        if (ctf) {
            xh_ctf_params c = r.ctf;      // processImage L418-422: Tm = Ts; the noise model is off
            c.Tm = h->prm.sampling;
            const CtfSide s = side_info(c, false);
            row0[kRowCtf] = 1;
            std::memcpy(row0 + kRowSide, &s, sizeof(s));
        }
        for (int s = 1; s < per; ++s) {      // the other presentations: E R_sym
            double *row = row0 + (size_t)kRow * s;
            std::memcpy(row, row0, sizeof(double) * kRow);
            const double *Rs = &h->sym[(size_t)9 * (s - 1)];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    double t = 0.0;
                    for (int k = 0; k < 3; ++k) t += E[a * 3 + k] * Rs[k * 3 + b];
                    row[a * 3 + b] = t;
                }
        }
    }
    XH_TRY(xh_buf_upload(ctx, h->d_rows, hr.data(), sizeof(double) * hr.size()));
    XH_TRY(xh_buf_alloc(ctx, h->d_Is, sizeof(double) * DD * n));
    XH_TRY(xh_buf_alloc(ctx, h->d_partials, sizeof(double) * 2 * h->tiles * ((size_t)n * per + 1)));
    XH_TRY(xh_buf_alloc(ctx, h->d_errors, sizeof(double) * ((size_t)n * per + 1)));
    // step 4 in chunks of at most 256 MiB of spectra: float -> complex, forward, CTFINV (or the normalisation alone), inverse, the real
    // part, applyGeometry
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(n, ((size_t)256 << 20) / (DD * sizeof(xh_cd))));
    XhBuf d_img, d_F, d_real;
    XH_TRY(xh_buf_alloc(ctx, d_img, sizeof(float) * DD * chunk));
    XH_TRY(xh_buf_alloc(ctx, d_F, sizeof(xh_cd) * DD * chunk));
    XH_TRY(xh_buf_alloc(ctx, d_real, sizeof(double) * DD * chunk));
    xh_cd *F = (xh_cd *)d_F.p;
    const int stride = kRow * per;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        const size_t total = DD * m;
        const unsigned gr = (unsigned)((total + 255) / 256);
        const double *qr = (const double *)h->d_rows.p + (size_t)stride * i0;
        XH_HIP(hipMemcpyAsync(d_img.p, h_images + DD * i0, sizeof(float) * total, hipMemcpyHostToDevice, ctx->stream));
        bool any = false;
        for (int i = i0; i < i0 + m; ++i) any = any || hr[(size_t)stride * i + kRowCtf] != 0.0;
        if (any) {
            XH_LAUNCH256(ctx, xh_k_to_complex64<float>, gr, (const float *)d_img.p, F, total);
            XH_TRY(xh_fft2d64(ctx, h->fft, F, m, false));
            if (h->prm.phase_flipped) XH_LAUNCH256(ctx, xh_k_ctfinv<true>, gr, F, total, D, qr, stride, kRowCtf, 1.0 / h->prm.sampling, kMinCTF);
            else XH_LAUNCH256(ctx, xh_k_ctfinv<false>, gr, F, total, D, qr, stride, kRowCtf, 1.0 / h->prm.sampling, kMinCTF);
            XH_TRY(xh_fft2d64(ctx, h->fft, F, m, true));
            XH_LAUNCH256(ctx, xh_k_real64<double>, gr, (const xh_cd *)F, (double *)d_real.p, total);
        } else {
            // no image of the chunk has a CTF: the particles are not filtered at all (artModel L734)
            XH_LAUNCH256(ctx, xh_k_to_complex64<float>, gr, (const float *)d_img.p, F, total);
            XH_LAUNCH256(ctx, xh_k_real64<double>, gr, (const xh_cd *)F, (double *)d_real.p, total);
        }
        XH_LAUNCH256(ctx, k_faz_shift, gr, (const double *)d_real.p, qr, stride, total, D, (double *)h->d_Is.p + DD * i0);
        XH_HIP(hipStreamSynchronize(ctx->stream));
    }
    return XH_OK;
}
}  // namespace

extern "C" {

void xh_faz_defaults(xh_faz_params *p)
{
    if (!p) return;
    p->RDef = -1; p->sampling = 1; p->lambda = 0.01; p->ltv = p->ltk = p->ll1 = p->lst = 1e-4;
    p->l1 = 3; p->l2 = 2; p->step = 1;
    p->use_zernike = p->use_ctf = p->phase_flipped = 0;
}

int xh_faz_sort_orthogonal(int32_t n, const double *h_rot, const double *h_tilt, int32_t sort_last, int32_t *h_order)
{
    XH_CHECK(n >= 0 && (n == 0 || (h_rot && h_tilt && h_order)), XH_ERR_ARG, "xh_faz_sort_orthogonal: bad argument");
    if (n == 0) return XH_OK;
    std::vector<double> v((size_t)3 * n), product((size_t)n, 0.0);
    std::vector<char> chosen((size_t)n, 0);
    for (int i = 0; i < n; ++i) {      // the third row of Euler_angles2matrix(rot, tilt, 0)
        double E[9];
        xh_fp_euler(h_rot[i], h_tilt[i], 0.0, E);
        for (int k = 0; k < 3; ++k) v[(size_t)3 * i + k] = E[6 + k];
    }
    auto dot = [&](int a, int b) { return v[3 * (size_t)a] * v[3 * (size_t)b] + v[3 * (size_t)a + 1] * v[3 * (size_t)b + 1] + v[3 * (size_t)a + 2] * v[3 * (size_t)b + 2]; };
    chosen[0] = 1;
    h_order[0] = 0;
    int min_prod_proj = 0;
    for (int i = 1; i < n; ++i) {
        double min_prod = (double)FLT_MAX;      // MAXFLOAT
        const int last = h_order[i - 1];
        const bool drop = sort_last != -1 && i > sort_last;
        const int old = drop ? h_order[i - sort_last - 1] : 0;
        for (int j = 0; j < n; ++j) {
            if (chosen[j]) continue;
            product[j] += std::fabs(dot(last, j));
            if (drop) product[j] -= std::fabs(dot(old, j));
            if (product[j] < min_prod) {
                min_prod = product[j];
                min_prod_proj = j;
            }
        }
        h_order[i] = min_prod_proj;
        chosen[min_prod_proj] = 1;
    }
    return XH_OK;
}

int xh_faz_save_schedule(int32_t n, int32_t save_iter, int32_t *h_flags)
{
    XH_CHECK(n >= 0 && (n == 0 || h_flags), XH_ERR_ARG, "xh_faz_save_schedule: bad argument");
    int current_save_iter = 1;      // run L554, L587-592
    for (int k = 0; k < n; ++k) {
        h_flags[k] = 0;
        if (current_save_iter == save_iter && save_iter > 0) {
            h_flags[k] = 1;
            current_save_iter = 1;
        }
        current_save_iter++;
    }
    return XH_OK;
}

int xh_faz_check(int32_t l1, int32_t l2, int32_t ncoef)
{
    XH_TRY(zk_check_degrees("xh_faz_check", l1, l2));
    const int vs = vds_num_terms(l1, l2);
    XH_CHECK(ncoef < 0 || ncoef == 3 * vs, XH_ERR_ARG, "xh_faz_check: sphCoefficients holds %d values, degrees l1 = %d, l2 = %d need 3 x %d = %d", ncoef, l1,
             l2, vs, 3 * vs);
    return XH_OK;
}

int xh_faz_create(xh_ctx *ctx, int32_t D, const double *h_V0, const int32_t *h_maskF, const int32_t *h_maskB, const double *h_sigma,
                  int32_t nsigma, const double *h_sym, int32_t nsym, const xh_faz_params *prm, xh_faz **out)
{
    XH_CHECK(ctx && prm && out && h_sigma && D >= 4 && nsym >= 0 && (nsym == 0 || h_sym), XH_ERR_ARG, "xh_faz_create: bad argument");
    XH_CHECK(D <= 1024, XH_ERR_UNSUPPORTED, "xh_faz_create: images above 1024 x 1024 are not supported (%d)", D);
    XH_CHECK(nsigma >= 1 && nsigma <= kMaxSigma, XH_ERR_UNSUPPORTED, "xh_faz_create: %d sigmas (1 .. %d are supported)", nsigma, kMaxSigma);
    XH_TRY(zk_check_degrees("xh_faz_create", prm->l1, prm->l2));
    XH_CHECK(prm->step >= 1, XH_ERR_ARG, "xh_faz_create: step %d must be positive", prm->step);
    XH_CHECK(prm->sampling > 0, XH_ERR_ARG, "xh_faz_create: sampling %g must be positive", prm->sampling);
    const double w[6] = {prm->RDef, prm->lambda, prm->ltv, prm->ltk, prm->ll1, prm->lst};
    for (double x : w) XH_CHECK(std::isfinite(x), XH_ERR_ARG, "xh_faz_create: a non-finite parameter");
    for (int s = 0; s < nsigma; ++s) XH_CHECK(std::isfinite(h_sigma[s]) && h_sigma[s] > 0, XH_ERR_ARG, "xh_faz_create: sigma %g must be positive", h_sigma[s]);
    XH_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<xh_faz> h(new xh_faz);
    h->ctx = ctx; h->prm = *prm; h->D = D; h->nsigma = nsigma; h->nsym = nsym; h->per = 1 + nsym;
    h->vecSize = vds_num_terms(prm->l1, prm->l2);
    h->RDef = prm->RDef < 0 ? (double)(D / 2) : prm->RDef;      // preProcess L212-213
    XH_CHECK(h->RDef > 0, XH_ERR_ARG, "xh_faz_create: RDef %g must be positive", h->RDef);
    for (int s = 0; s < nsigma; ++s) h->sig.s[s] = h_sigma[s];
    if (nsym) h->sym.assign(h_sym, h_sym + (size_t)9 * nsym);
    const size_t DD = (size_t)D * D, N = DD * D;
    const int c = D / 2;
    // the masks (L226-273): a file's values where r^2 < RDef^2, else the sphere r^2 <= RDef^2
    std::vector<int32_t> mF(N), mB(N);
    const double R2 = h->RDef * h->RDef;
    auto make = [&](const int32_t *src, std::vector<int32_t> &m) -> int {
        if (!src) return xh_halves_circular_mask(D, D, D, -h->RDef, 0, 0, 0, m.data());
        for (int pk = 0; pk < D; ++pk)
            for (int pi = 0; pi < D; ++pi)
                for (int pj = 0; pj < D; ++pj) {
                    const int k = pk - c, i = pi - c, j = pj - c;
                    const size_t e = ((size_t)pk * D + pi) * D + pj;
                    m[e] = (double)(k * k + i * i + j * j) >= R2 ? 0 : src[e];
                }
        return XH_OK;
    };
    XH_TRY(make(h_maskF, mF));
    XH_TRY(make(h_maskB, mB));
    // the forward list: per sigma the 16^3 bricks that hold a voxel of that sigma on the --step lattice (cpp L230-265)
    std::vector<FazBrick> bricks;
    const int step = prm->step, nb = (D + kBrick - 1) / kBrick;
    for (int s = 0; s < nsigma; ++s) {
        const bool multi = nsigma > 1;
        const int value = (int)h_sigma[s];
        if (multi && (double)value != h_sigma[s]) continue;      // no int mask value equals this sigma
        for (int bz = 0; bz < nb; ++bz)
            for (int by = 0; by < nb; ++by)
                for (int bx = 0; bx < nb; ++bx) {
                    bool any = false;
                    for (int pk = bz * kBrick; pk < std::min(D, (bz + 1) * kBrick) && !any; ++pk) {
                        if (pk % step) continue;
                        for (int pi = by * kBrick; pi < std::min(D, (by + 1) * kBrick) && !any; ++pi) {
                            if (pi % step) continue;
                            for (int pj = bx * kBrick; pj < std::min(D, (bx + 1) * kBrick); ++pj) {
                                if (pj % step) continue;
                                const int mv = mF[((size_t)pk * D + pi) * D + pj];
                                if (multi ? mv == value && mv != 0 : mv != 0) { any = true; break; }
                            }
                        }
                    }
                    if (any) bricks.push_back(FazBrick{bx * kBrick, by * kBrick, bz * kBrick, s, value});
                }
    }
    // with several sigmas a voxel whose value is 0 never reaches the list (checkStep); value 0 can equal no positive sigma
    h->nbricks = (int)bricks.size();
    if (h->nbricks) XH_TRY(xh_buf_upload(ctx, h->d_bricks, bricks.data(), sizeof(FazBrick) * bricks.size()));
    XH_TRY(xh_buf_upload(ctx, h->d_maskF, mF.data(), sizeof(int32_t) * N));
    XH_TRY(xh_buf_upload(ctx, h->d_maskB, mB.data(), sizeof(int32_t) * N));
    XhBuf *vols[6] = {&h->d_V, &h->d_Dx, &h->d_Dy, &h->d_Dz, &h->d_Dl1, &h->d_Reg};
    for (XhBuf *b : vols) {
        XH_TRY(xh_buf_alloc(ctx, *b, sizeof(double) * N));
        XH_HIP(hipMemsetAsync(b->p, 0, sizeof(double) * N, ctx->stream));
    }
    if (h_V0) XH_HIP(hipMemcpyAsync(h->d_V.p, h_V0, sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    FazGeom &g = h->g;
    g.D = D; g.DD = (int)DD; g.c = c; g.step = step; g.multi = nsigma > 1;
    g.iRDef = 1.0 / h->RDef; g.istep = 1.0 / (double)step;
    h->tiles = (int)((DD + 255) / 256);
    XH_TRY(xh_fft2d64_create(ctx, D, D, h->fft, "xh_faz_create"));
    XH_TRY(xh_buf_alloc(ctx, h->d_planes, sizeof(double) * DD * 2 * nsigma));
    XH_TRY(xh_buf_alloc(ctx, h->d_F, sizeof(xh_cd) * DD * 2 * nsigma));
    XH_TRY(xh_buf_alloc(ctx, h->d_Idiff, sizeof(double) * DD));
    XH_TRY(xh_buf_alloc(ctx, h->d_Iws, sizeof(double) * DD));
    *out = h.release();
    return XH_OK;
}

int xh_faz_destroy(xh_faz *h)
{
    delete h;
    return XH_OK;
}

int xh_faz_info(const xh_faz *h, double *RDef, int32_t *vecSize, int32_t *nbricks, int32_t *per_image)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_faz_info: null handle");
    if (RDef) *RDef = h->RDef;
    if (vecSize) *vecSize = h->vecSize;
    if (nbricks) *nbricks = h->nbricks;
    if (per_image) *per_image = h->per;
    return XH_OK;
}

int xh_faz_load(xh_faz *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_faz_row *rows, const double *h_coef)
{
    XH_CHECK(h && h_images && rows && n >= 1, XH_ERR_ARG, "xh_faz_load: bad argument");
    XH_CHECK(!h->prm.use_zernike || h_coef, XH_ERR_ARG, "xh_faz_load: the handle deforms (use_zernike) and no coefficients are given");
    XH_CHECK(ydim == xdim && xdim == h->D, XH_ERR_UNSUPPORTED, "xh_faz_load: images of %d x %d against a volume of size %d", ydim, xdim, h->D);
    h->nloaded = 0;
    const int rc = faz_load(h, h_images, n, rows, h_coef);
    if (rc == XH_OK) h->nloaded = n;
    return rc;
}

int xh_faz_sweep(xh_faz *h, int32_t first, int32_t count, double *h_errors)
{
    XH_CHECK(h && count >= 0 && first >= 0, XH_ERR_ARG, "xh_faz_sweep: bad argument");
    XH_CHECK(first + count <= h->nloaded, XH_ERR_STATE, "xh_faz_sweep: images %d .. %d of the %d loaded", first, first + count - 1, h->nloaded);
    if (count == 0) return XH_OK;
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    double *partials = (double *)h->d_partials.p;
    const int per = h->per;
    std::vector<XhEvent> events(h->timing ? (size_t)(FAZ_NT + 1) * count * per : 0);      // of this sweep, FAZ_NT + 1 per presentation
    for (XhEvent &e : events) XH_TRY(xh_event_create(e));
    for (int k = 0; k < count; ++k)
        for (int s = 0; s < per; ++s) {
            const XhEvent *ev = h->timing ? &events[(size_t)(FAZ_NT + 1) * ((size_t)k * per + s)] : nullptr;
            XH_TRY(faz_forward(h, first + k, s, partials + (size_t)2 * h->tiles * ((size_t)k * per + s), ev));
            XH_TRY(faz_backward(h, first + k, s, ev));
        }
    XH_LAUNCH256(ctx, k_faz_errors, count * per, (const double *)partials, h->tiles, (double *)h->d_errors.p);
    if (h_errors) XH_HIP(hipMemcpyAsync(h_errors, h->d_errors.p, sizeof(double) * count * per, hipMemcpyDeviceToHost, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    if (h->timing) {
        for (double &v : h->stage_ms) v = 0.0;
        for (size_t p = 0; p < (size_t)count * per; ++p)
            for (int t = 0; t < FAZ_NT; ++t) {
                float ms = 0.f;
                XH_HIP(hipEventElapsedTime(&ms, events[(FAZ_NT + 1) * p + t], events[(FAZ_NT + 1) * p + t + 1]));
                h->stage_ms[t] += ms;
            }
    }
    return XH_OK;
}

int xh_faz_set_timing(xh_faz *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_faz_set_timing: null handle");
    h->timing = on != 0;
    return XH_OK;
}

int xh_faz_stage_ms(const xh_faz *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_faz_stage_ms: null argument");
    for (int t = 0; t < FAZ_NT; ++t) h_ms[t] = h->stage_ms[t];
    return XH_OK;
}

int xh_faz_forward(xh_faz *h, int32_t index, int32_t sym, double *d_P_raw, double *d_W_raw, double *d_P, double *d_W, double *d_Idiff,
                   double *d_Iws, double *d_particle, double *h_error)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_faz_forward: null handle");
    XH_CHECK(index >= 0 && index < h->nloaded, XH_ERR_STATE, "xh_faz_forward: image %d of the %d loaded", index, h->nloaded);
    XH_CHECK(sym >= 0 && sym < h->per, XH_ERR_ARG, "xh_faz_forward: presentation %d of %d", sym, h->per);
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int S = h->nsigma;
    const size_t DD = (size_t)h->D * h->D, plane = sizeof(double) * DD;
    // the slot after the last presentation's is this call's
    double *partials = (double *)h->d_partials.p + (size_t)2 * h->tiles * ((size_t)h->nloaded * h->per);
    double *err = (double *)h->d_errors.p + (size_t)h->nloaded * h->per;
    XH_TRY(faz_forward(h, index, sym, partials));
    XH_LAUNCH256(ctx, k_faz_errors, 1, (const double *)partials, h->tiles, err);
    if (d_P_raw) XH_HIP(hipMemcpyAsync(d_P_raw, h->d_planes.p, plane * S, hipMemcpyDeviceToDevice, st));
    if (d_W_raw) XH_HIP(hipMemcpyAsync(d_W_raw, (const char *)h->d_planes.p + plane * S, plane * S, hipMemcpyDeviceToDevice, st));
    const unsigned gr = (unsigned)((DD * S + 255) / 256);
    if (d_P) XH_LAUNCH256(ctx, xh_k_real64<double>, gr, (const xh_cd *)h->d_F.p, d_P, DD * S);
    if (d_W) XH_LAUNCH256(ctx, xh_k_real64<double>, gr, (const xh_cd *)h->d_F.p + DD * S, d_W, DD * S);
    if (d_Idiff) XH_HIP(hipMemcpyAsync(d_Idiff, h->d_Idiff.p, plane, hipMemcpyDeviceToDevice, st));
    if (d_Iws) XH_HIP(hipMemcpyAsync(d_Iws, h->d_Iws.p, plane, hipMemcpyDeviceToDevice, st));
    if (d_particle) XH_HIP(hipMemcpyAsync(d_particle, (const char *)h->d_Is.p + plane * index, plane, hipMemcpyDeviceToDevice, st));
    if (h_error) XH_HIP(hipMemcpyAsync(h_error, err, sizeof(double), hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

int xh_faz_get_volume(xh_faz *h, double *h_V)
{
    XH_CHECK(h && h_V, XH_ERR_ARG, "xh_faz_get_volume: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(h_V, h->d_V.p, h->d_V.bytes, hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

int xh_faz_set_volume(xh_faz *h, const double *h_V)
{
    XH_CHECK(h && h_V, XH_ERR_ARG, "xh_faz_set_volume: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(h->d_V.p, h_V, h->d_V.bytes, hipMemcpyHostToDevice, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    return XH_OK;
}

}  // extern "C"
