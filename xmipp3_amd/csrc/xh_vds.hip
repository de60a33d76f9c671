// xh_vds.hip -- the device side of xmipp_volume_deform_sph (reconstruction/volume_deform_sph.cpp; CUDA twin
// reconstruction_adapt_cuda/volume_deform_sph_gpu.cpp, reconstruction_cuda/cuda_volume_deform_sph.{cu,cpp}), fp64.
//
// Two volumes in, one deformation out: the displacement field g = sum_idx c_idx Z_idx over the ball r < Rmax, three coefficients
// (x, y, z) per term of the Zernike3D basis, is fitted by Powell's method so that the input volume sampled at p + g(p) matches the
// reference. One cost evaluation (k_vds_cost) covers every voxel of the ball, every (input, reference) pair: basis sum, trilinear
// sample with 0 outside the volume, three sums. Powell calls it thousands of times, one after the other.
//
// Basis (vds_radial, vds_harmonic; __host__ __device__, so xh_vds_zsh and the kernels run the same code). Term (l1, n, l2, m) is
//     Z = R_l1^n(r) S_l2^m(xr, yr, zr)
// with (xr, yr, zr) the voxel's logical coordinates over Rmax and r their norm.
//  - R_l^n(r) = sqrt(2 l + 3) r^n P_k^(0, n + 1/2)(2 r^2 - 1), k = (l - n) / 2, the 3-D Zernike radial polynomial normalised to
//    int_0^1 R^2 r^2 dr = 1, written out for l <= 5 and evaluated by Horner's rule in r^2.
//  - S_l^m is the real solid harmonic r^l Y_l^m (m < 0: sine, m > 0: cosine, in the usual 4 pi normalisation of Y), a homogeneous
//    polynomial of degree l in (xr, yr, zr), written out for l <= 4. It is evaluated at the scaled coordinates, not on the unit sphere,
//    as the reference evaluates it: a coefficient file means the same field here and upstream.
//  - S_4^0 is the one exception, and it is the reference's: 35 zr^4 - 30 zr^2 + 3, the unit-sphere form at scaled coordinates, in both
//    its CPU and its CUDA source. It is kept, because <oroot>_clnm.txt is read back by upstream programs that evaluate that form.
//
// k_vds_cost is instantiated for every (L1, L2) with 1 <= L1 <= 5, L2 <= min(L1, 4): the term loop unrolls into straight-line
// polynomial code that shares x^2, y^2, z^2, r^2, every harmonic of a degree and every radial polynomial across the terms; any other
// pair of degrees runs the same function with run-time bounds. The coefficients are a kernel argument (3 * 45 doubles at most), read
// at compile-time offsets: scalar loads. A stage of the search moves only the terms of degrees (L1, h): while every coefficient past
// them is exactly 0, the evaluation runs the (L1, h) instantiation, whose terms are a prefix of the full list; the skipped terms would
// each add c * Z = 0.
// Lanes run along x inside the bounding box of the ball, so the taps of neighbouring voxels are neighbours in memory. Voxels with
// r^2 >= Rmax^2 have g = 0 and sample exactly I[k, i, j]: their share of diff2 and sumVD is a constant of the loaded pairs, summed once
// on the host by xh_vds_set_pairs, and their share of modg is 0.
// Reduction: every thread sums its voxels in index order, a workgroup adds its 256 sums in a fixed tree in LDS, one workgroup adds the
// per-workgroup partials in a fixed order (xh_reduce.h). No floating-point atomics, and the grid depends on the handle's geometry alone: the same
// coefficients give the same bits on every call. Three doubles come back per evaluation, into page-locked memory.
//
// Deviations from the reference, each where it reads what it never wrote, or where its two versions disagree:
//  - The displacement is the CUDA twin's: every term counts. The CPU computeShift skips a term when its x coefficient alone is 0, which
//    leaves the cost flat along every y-only and z-only direction.
//  - An empty --sigma (and, as in the reference, the single value 0) means no filtered pairs; the reference indexes an empty vector.
//  - The first background mask of normalize_Robust is zeros; the reference leaves it uninitialised.
//  - Degrees above l1 = 5, l2 = 4 (the reference's trigonometric forms) are refused with XH_ERR_UNSUPPORTED.
//  - modg counts each voxel once per pair (pairs * |g|^2), as the twin does; the final evaluation that writes the output volume counts
//    the raw pair in no sum, so the value it prints is the search's own cost at the returned coefficients.
//  - The search hands Powell only the variables whose step is 1 (the reference hands it all 3 vecSize, the frozen ones with step 0, and
//    spends line searches on flat directions): the minimum agrees within ftol, not bit for bit (host/powell.h).
//  - normalize_Robust rests on xmippCore primitives whose source is not in the reference tree (compute_hist, index2val, binarize, the
//    median within a mask); the readings used are stated at xh_vds_normalize_robust and in SURVEY Appendix B.
#include "xh_fft3d.h"
#include "xh_reduce.h"
#include "xh_zernike.h"
#include <algorithm>
#include <cmath>

namespace {

struct VdsGeom : ZkDims {    // Z, Y, X: the volume
    int z0, y0, x0;          // the box's first voxel (physical)
    int bz, by, bx;          // the box
    int npairs;
    size_t N;
    double Rmax2, iRmax;
};


// diff2, sumVD, modg over the voxels of the box with r^2 < Rmax^2
template <int L1, int L2>
__global__ void __launch_bounds__(256)
k_vds_cost(const double *__restrict__ I, const double *__restrict__ R, const VdsGeom g, const VdsCoef C, int l1, int l2, double *__restrict__ partials)
{
    double acc[3] = {0.0, 0.0, 0.0};
    const unsigned nbox = (unsigned)g.bz * (unsigned)g.by * (unsigned)g.bx;
    for (unsigned n = blockIdx.x * 256u + threadIdx.x; n < nbox; n += gridDim.x * 256u) {
        const unsigned t = n / (unsigned)g.bx;
        const int pj = g.x0 + (int)(n - t * (unsigned)g.bx);
        const unsigned bk = t / (unsigned)g.by;
        const int pi = g.y0 + (int)(t - bk * (unsigned)g.by), pk = g.z0 + (int)bk;
        const int j = pj - g.X / 2, i = pi - g.Y / 2, k = pk - g.Z / 2;
        const double r2 = (double)(k * k + i * i + j * j);
        if (!(r2 < g.Rmax2)) continue;
        const double rr = sqrt(r2) * g.iRmax;
        double gx, gy, gz;
        vds_disp<L1, L2>(C, l1, l2, j * g.iRmax, i * g.iRmax, k * g.iRmax, rr, gx, gy, gz);
        const size_t e = ((size_t)pk * g.Y + pi) * g.X + pj;
        const double x = j + gx, y = i + gy, z = k + gz;
        for (int p = 0; p < g.npairs; ++p) {
            const double vI = vds_sample(I + (size_t)p * g.N, g, x, y, z);
            const double d = R[(size_t)p * g.N + e] - vI;
            acc[0] += d * d;
            if (vI >= 0.0) acc[1] += vI;
        }
        acc[2] += (double)g.npairs * (gx * gx + gy * gy + gz * gz);
    }
    xh_block_partials(acc, partials);
}

// the output volume and the field: every voxel of the volume. G (nullable) [3][N]
__global__ void __launch_bounds__(256)
k_vds_apply(const double *__restrict__ raw, const VdsGeom g, const VdsCoef C, int l1, int l2, double *__restrict__ VO, double *__restrict__ G)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < g.N; e += (size_t)gridDim.x * 256) {
        const int pj = (int)(e % g.X);
        const size_t t = e / g.X;
        const int pi = (int)(t % g.Y), pk = (int)(t / g.Y);
        const int j = pj - g.X / 2, i = pi - g.Y / 2, k = pk - g.Z / 2;
        const double r2 = (double)(k * k + i * i + j * j);
        double gx = 0.0, gy = 0.0, gz = 0.0;
        if (r2 < g.Rmax2) vds_disp<-1, -1>(C, l1, l2, j * g.iRmax, i * g.iRmax, k * g.iRmax, sqrt(r2) * g.iRmax, gx, gy, gz);
        VO[e] = vds_sample(raw, g, j + gx, i + gy, k + gz);
        if (G) { G[e] = gx; G[g.N + e] = gy; G[2 * g.N + e] = gz; }
    }
}

// REALGAUSSIAN low pass exp(-pi^2 w^2 sigma^2) of a half spectrum [Z][Y][xh], times scale
__global__ void __launch_bounds__(256) k_vds_gauss(xh_cd *__restrict__ F, int Z, int Y, int X, int xh, double sigma, double scale)
{
    const size_t NF = (size_t)Z * Y * xh;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < NF; e += (size_t)gridDim.x * 256) {
        const int j = (int)(e % xh);
        const size_t r = e / xh;
        const double fx = d_digfreq(j, X), fy = d_digfreq((int)(r % Y), Y), fz = d_digfreq((int)(r / Y), Z);
        const double w = scale * exp(-VDS_PI * VDS_PI * (fx * fx + fy * fy + fz * fz) * sigma * sigma);
        F[e] = xh_cd{F[e].x * w, F[e].y * w};
    }
}

// computeStrain over the interior (2 voxels in from every face); LS and LR are zeroed before. The sums are written without
// contraction, so that a restatement in scalar double arithmetic gives the same bits.
__global__ void __launch_bounds__(256)
k_vds_strain(const double *__restrict__ G, int Z, int Y, int X, double *__restrict__ LS, double *__restrict__ LR)
{
#pragma clang fp contract(off)
    const size_t N = (size_t)Z * Y * X, sy = (size_t)X, sz = (size_t)X * Y;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (size_t)gridDim.x * 256) {
        const int pj = (int)(e % X);
        const size_t t = e / X;
        const int pi = (int)(t % Y), pk = (int)(t / Y);
        if (pj < 2 || pj >= X - 2 || pi < 2 || pi >= Y - 2 || pk < 2 || pk >= Z - 2) continue;
        double U[3][3];
        for (int c = 0; c < 3; ++c) {
            const double *V = G + (size_t)c * N + e;
            U[c][0] = (V[-2] - 8 * V[-1] + 8 * V[1] - V[2]) / 12.0;
            U[c][1] = (V[-2 * (ptrdiff_t)sy] - 8 * V[-(ptrdiff_t)sy] + 8 * V[sy] - V[2 * sy]) / 12.0;
            U[c][2] = (V[-2 * (ptrdiff_t)sz] - 8 * V[-(ptrdiff_t)sz] + 8 * V[sz] - V[2 * sz]) / 12.0;
        }
        const double d00 = U[0][0], d11 = U[1][1], d22 = U[2][2];
        const double d01 = 0.5 * (U[0][1] + U[1][0]), d02 = 0.5 * (U[0][2] + U[2][0]), d12 = 0.5 * (U[1][2] + U[2][1]);
        const double h01 = 0.5 * (U[0][1] - U[1][0]), h02 = 0.5 * (U[0][2] - U[2][0]), h12 = 0.5 * (U[1][2] - U[2][1]);
        const double det = d00 * (d11 * d22 - d12 * d12) - d01 * (d01 * d22 - d12 * d02) + d02 * (d01 * d12 - d11 * d02);
        LS[e] = fabs(det);
        // the eigenvalues of a 3 x 3 antisymmetric matrix are 0 and +- i sqrt(h01^2 + h02^2 + h12^2)
        const double w = sqrt(h01 * h01 + h02 * h02 + h12 * h12);
        LR[e] = w > 1e-6 ? w * 180.0 / VDS_PI : 0.0;
    }
}

}  // namespace

// ---------------------------------------------------------------- the handle
struct xh_vds {
    xh_ctx *ctx = nullptr;
    VdsGeom g = {};
    int L1 = 0, L2 = 0, vecSize = 0;
    double Rmax = 0, lambda = 0;
    unsigned grid = 0, gridVol = 0;
    XhFft3d fft;
    XhBuf I, R;                    // the pairs [npairs][N]
    XhBuf B[2];                    // scratch volumes: raw and VO, LS and LR
    XhBuf C, partials, result;
    XhBuf G;                       // the field [3][N] of apply and strain, allocated at the first use
    XhPinned pinned;               // 3 doubles
    double sumVI = 0, outDiff2 = 0, outSumVD = 0;
    int64_t evals = 0;
    int costRc = XH_OK;
    ~xh_vds()
    {
        if (ctx) (void)hipSetDevice(ctx->device);
    }
};

namespace {

int vds_launch_cost(xh_vds *h, const VdsCoef &C, int l2)
{
    const double *I = (const double *)h->I.p, *R = (const double *)h->R.p;
    double *part = (double *)h->partials.p;
    const int l1 = h->L1;
#define VDS_LAUNCH(A, B) XH_LAUNCH256(h->ctx, (k_vds_cost<A, B>), h->grid, I, R, h->g, C, l1, l2, part)
    ZK_DISPATCH(l1, l2, VDS_LAUNCH);
#undef VDS_LAUNCH
    return XH_OK;
}

int vds_gauss_dev(xh_vds *h, double *d_v, double sigma)
{
    xh_cd *F = (xh_cd *)h->C.p;
    XH_TRY(h->fft.r2c(d_v, F));
    XH_LAUNCH256(h->ctx, k_vds_gauss, h->gridVol, F, h->g.Z, h->g.Y, h->g.X, h->fft.xh, sigma, 1.0 / (double)h->g.N);
    return h->fft.c2r(F, d_v, 1.0);
}

struct VdsStage { xh_vds *h; std::vector<double> x; std::vector<int> active; };

double vds_stage_cb(double *p, void *prm)
{
    VdsStage *s = (VdsStage *)prm;
    for (size_t a = 0; a < s->active.size(); ++a) s->x[s->active[a]] = p[a + 1];
    double out[4] = {1e38, 0, 0, 0};
    if (s->h->costRc == XH_OK) s->h->costRc = xh_vds_cost(s->h, s->x.data(), out);
    ++s->h->evals;
    return s->h->costRc == XH_OK ? out[0] : 1e38;
}

// Shannon entropy (base 10) of the bins [first, last) of a normalised histogram, taken as a distribution of total mass `mass`:
// bins are added in index order; an empty bin (and an empty partition) contributes nothing
double vds_partition_entropy(const std::vector<double> &prob, int first, int last, double mass)
{
    const double tiny = 1e-15;
    double entropy = 0.0;
    if (mass <= tiny) return entropy;
    for (int b = first; b < last; ++b)
        if (prob[b] > tiny) {
            const double q = prob[b] / mass;
            entropy -= q * std::log10(q);
        }
    return entropy;
}

// Maximum-entropy threshold (Kapur's criterion, what the reference's EntropySegmentation computes) over a histogram of
// VDS_HIST_BINS bins: the cut after bin c splits the histogram into [0, c] and (c, end); the threshold is the lower edge of the first
// cut, among all but the last bin, at which the two partitions' entropies add up to the most. Readings of the xmippCore
// histogram: bins of (max - min) / bins over [min, max], index floor((v - min) / width), the maximum in the last bin; the value of
// bin c is min + c width.
int vds_entropy_threshold(const double *v, size_t n, double *thr)
{
    constexpr int VDS_HIST_BINS = 200;
    const auto range = std::minmax_element(v, v + n);
    const double lowest = *range.first, highest = *range.second;
    XH_CHECK(highest > lowest, XH_ERR_ARG, "xh_vds_normalize_robust: the volume is constant (%g)", lowest);
    const double width = (highest - lowest) / VDS_HIST_BINS;
    std::vector<double> prob(VDS_HIST_BINS, 0.0);
    for (size_t e = 0; e < n; ++e) prob[std::min((int)std::floor((v[e] - lowest) / width), VDS_HIST_BINS - 1)] += 1.0;
    for (double &p : prob) p /= (double)n;
    int bestCut = 0;
    double best = 0.0, below = 0.0;          // below: the mass of bins 0 .. cut
    for (int cut = 0; cut < VDS_HIST_BINS - 1; ++cut) {
        below += prob[cut];
        const double total = vds_partition_entropy(prob, 0, cut + 1, below) + vds_partition_entropy(prob, cut + 1, VDS_HIST_BINS, 1 - below);
        if (cut == 0 || total > best) { best = total; bestCut = cut; }
    }
    *thr = lowest + bestCut * width;
    return XH_OK;
}

}  // namespace

extern "C" {

int xh_vds_num_terms(int32_t L1, int32_t L2, int32_t *n)
{
    XH_CHECK(n, XH_ERR_ARG, "xh_vds_num_terms: null argument");
    XH_TRY(zk_check_degrees("xh_vds_num_terms", L1, L2));
    *n = vds_num_terms(L1, L2);
    return XH_OK;
}

int xh_vds_terms(int32_t L1, int32_t L2, int32_t *out)
{
    XH_CHECK(out, XH_ERR_ARG, "xh_vds_terms: null argument");
    XH_TRY(zk_check_degrees("xh_vds_terms", L1, L2));
    int idx = 0;
    for (int h = 0; h <= L2; ++h)
        for (int l = h; l <= L1; l += 2)
            for (int m = -h; m <= h; ++m, ++idx) { out[4 * idx] = l; out[4 * idx + 1] = h; out[4 * idx + 2] = h; out[4 * idx + 3] = m; }
    return XH_OK;
}

int xh_vds_zsh(int32_t l1, int32_t n, int32_t l2, int32_t m, double xr, double yr, double zr, double r, double *out)
{
    XH_CHECK(out, XH_ERR_ARG, "xh_vds_zsh: null argument");
    XH_TRY(zk_check_degrees("xh_vds_zsh", l1, l2));
    XH_CHECK(n >= 0 && n <= l1 && (l1 - n) % 2 == 0 && m >= -l2 && m <= l2, XH_ERR_ARG, "xh_vds_zsh: (l1 %d, n %d, l2 %d, m %d) is no basis term", l1, n, l2, m);
    *out = vds_radial(l1, n, r, r * r) * vds_harmonic(l2, m, xr, yr, zr, xr * xr, yr * yr, zr * zr);
    return XH_OK;
}

// normalize_Robust (data/normalize.cpp:265-313) with a zero background mask: the background is where EntropySegmentation's binarize
// (v <= threshold + 1e-6 -> 0) gives 0, medianBg its median (middle element, mean of the two middle ones for an even count), p99 the
// element int(0.99 n) of the sorted foreground; v = (v - medianBg) / p99, clipped to +-clip when clip > 0.
int xh_vds_normalize_robust(double *v, size_t n, double clip)
{
    XH_CHECK(v && n > 0, XH_ERR_ARG, "xh_vds_normalize_robust: bad argument");
    for (size_t i = 0; i < n; ++i) XH_CHECK(std::isfinite(v[i]), XH_ERR_ARG, "xh_vds_normalize_robust: voxel %zu is not finite", i);
    double thr;
    XH_TRY(vds_entropy_threshold(v, n, &thr));
    std::vector<double> bg, fg;
    for (size_t i = 0; i < n; ++i) (v[i] <= thr + 1e-6 ? bg : fg).push_back(v[i]);
    XH_CHECK(!fg.empty(), XH_ERR_ARG, "xh_vds_normalize_robust: the segmentation left no foreground");
    XH_CHECK(!bg.empty(), XH_ERR_ARG, "xh_vds_normalize_robust: the segmentation left no background");
    std::sort(bg.begin(), bg.end());
    std::sort(fg.begin(), fg.end());
    const size_t nb = bg.size();
    const double medianBg = nb % 2 ? bg[nb / 2] : 0.5 * (bg[nb / 2 - 1] + bg[nb / 2]);
    const double p99 = fg[(size_t)(int)(fg.size() * 0.99)];
    XH_CHECK(p99 > 0, XH_ERR_ARG, "xh_vds_normalize_robust: the foreground's 99th percentile %g is not positive", p99);
    const double ip99 = 1 / p99;
    for (size_t i = 0; i < n; ++i) {
        double a = (v[i] - medianBg) * ip99;
        if (clip > 0) a = a > clip ? clip : a < -clip ? -clip : a;
        v[i] = a;
    }
    return XH_OK;
}

int xh_vds_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t L1, int32_t L2, double Rmax, double lambda, xh_vds **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_vds_create: null argument");
    XH_CHECK(Z >= 1 && Y >= 1 && X >= 2, XH_ERR_ARG, "xh_vds_create: bad size %d x %d x %d", Z, Y, X);
    XH_CHECK(Z <= 1024 && Y <= 1024 && X <= 1024, XH_ERR_UNSUPPORTED, "xh_vds_create: sizes above 1024 are not supported (%d x %d x %d)", Z, Y, X);
    XH_TRY(zk_check_degrees("xh_vds_create", L1, L2));
    if (Rmax < 0) Rmax = (double)(X / 2);
    XH_CHECK(std::isfinite(Rmax) && Rmax > 0 && std::isfinite(lambda), XH_ERR_ARG, "xh_vds_create: Rmax %g, lambda %g", Rmax, lambda);
    XH_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<xh_vds> h(new xh_vds);
    h->ctx = ctx; h->L1 = L1; h->L2 = L2; h->Rmax = Rmax; h->lambda = lambda;
    h->vecSize = vds_num_terms(L1, L2);
    XH_TRY(xh_fft3d_create(ctx, Z, Y, X, h->fft));
    VdsGeom &g = h->g;
    g.Z = Z; g.Y = Y; g.X = X; g.N = (size_t)Z * Y * X; g.npairs = 0;
    g.Rmax2 = Rmax * Rmax; g.iRmax = 1.0 / Rmax;
    // r^2 < Rmax^2 needs |coordinate| < Rmax, so |coordinate| <= ceil(Rmax) - 1; clipped to the volume
    const int B = (int)std::min(2048.0, std::ceil(Rmax)) - 1;
    const int dims[3] = {Z, Y, X};
    int lo[3], n[3];
    for (int a = 0; a < 3; ++a) {
        const int c = dims[a] / 2, first = std::max(0, c - B), last = std::min(dims[a] - 1, c + B);
        lo[a] = first; n[a] = last - first + 1;
    }
    g.z0 = lo[0]; g.y0 = lo[1]; g.x0 = lo[2]; g.bz = n[0]; g.by = n[1]; g.bx = n[2];
    const size_t nbox = (size_t)g.bz * g.by * g.bx, NF = (size_t)Z * Y * h->fft.xh;
    h->grid = (unsigned)std::max<size_t>(1, std::min<size_t>((nbox + 255) / 256, (size_t)ctx->num_cus * 8));
    h->gridVol = (unsigned)std::max<size_t>(1, std::min<size_t>((g.N + 255) / 256, (size_t)ctx->num_cus * 8));
    for (XhBuf &b : h->B) XH_TRY(xh_buf_alloc(ctx, b, sizeof(double) * g.N));
    XH_TRY(xh_buf_alloc(ctx, h->C, sizeof(xh_cd) * NF));
    XH_TRY(xh_buf_alloc(ctx, h->partials, sizeof(double) * 3 * h->grid));
    XH_TRY(xh_buf_alloc(ctx, h->result, sizeof(double) * 3));
    XH_TRY(xh_pinned_alloc(ctx, h->pinned, sizeof(double) * 3));
    *out = h.release();
    return XH_OK;
}

int xh_vds_destroy(xh_vds *h)
{
    delete h;
    return XH_OK;
}

int xh_vds_info(const xh_vds *h, double *Rmax, int32_t *nterms, double *sumVI)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_vds_info: null handle");
    if (Rmax) *Rmax = h->Rmax;
    if (nterms) *nterms = h->vecSize;
    if (sumVI) *sumVI = h->sumVI;
    return XH_OK;
}

int xh_vds_gauss(xh_vds *h, double sigma, const double *h_in, double *h_out)
{
    XH_CHECK(h && h_in && h_out, XH_ERR_ARG, "xh_vds_gauss: null argument");
    XH_CHECK(std::isfinite(sigma), XH_ERR_ARG, "xh_vds_gauss: sigma %g", sigma);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    XH_HIP(hipMemcpyAsync(h->B[0].p, h_in, h->B[0].bytes, hipMemcpyHostToDevice, st));
    XH_TRY(vds_gauss_dev(h, (double *)h->B[0].p, sigma));
    XH_HIP(hipMemcpyAsync(h_out, h->B[0].p, h->B[0].bytes, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

int xh_vds_set_pairs(xh_vds *h, int32_t npairs, const double *h_I, const double *h_R)
{
    XH_CHECK(h && h_I && h_R, XH_ERR_ARG, "xh_vds_set_pairs: null argument");
    XH_CHECK(npairs >= 1 && npairs <= 64, XH_ERR_ARG, "xh_vds_set_pairs: %d pairs (1 .. 64)", npairs);
    XH_HIP(hipSetDevice(h->ctx->device));
    const VdsGeom &g = h->g;
    const size_t bytes = sizeof(double) * g.N * npairs;
    h->g.npairs = 0;
    XH_TRY(xh_buf_upload(h->ctx, h->I, h_I, bytes));
    XH_TRY(xh_buf_upload(h->ctx, h->R, h_R, bytes));
    // sumVI, and the share of diff2 and sumVD of the voxels with r^2 >= Rmax^2, where the sample is I itself
    double sumVI = 0, d2 = 0, vd = 0;
    for (int p = 0; p < npairs; ++p) {
        const double *I = h_I + (size_t)p * g.N, *R = h_R + (size_t)p * g.N;
        size_t e = 0;
        for (int pk = 0; pk < g.Z; ++pk)
            for (int pi = 0; pi < g.Y; ++pi)
                for (int pj = 0; pj < g.X; ++pj, ++e) {
                    const int k = pk - g.Z / 2, i = pi - g.Y / 2, j = pj - g.X / 2;
                    const double v = I[e];
                    if (v >= 0.0) sumVI += v;
                    if ((double)(k * k + i * i + j * j) < g.Rmax2) continue;
                    const double d = R[e] - v;
                    d2 += d * d;
                    if (v >= 0.0) vd += v;
                }
    }
    XH_CHECK(std::isfinite(sumVI) && sumVI > 0, XH_ERR_ARG, "xh_vds_set_pairs: the input volumes have no positive mass (sum %g)", sumVI);
    h->sumVI = sumVI; h->outDiff2 = d2; h->outSumVD = vd;
    h->g.npairs = npairs;
    return XH_OK;
}

int xh_vds_cost(xh_vds *h, const double *h_x, double *h_out)
{
    XH_CHECK(h && h_x && h_out, XH_ERR_ARG, "xh_vds_cost: null argument");
    XH_CHECK(h->g.npairs > 0, XH_ERR_STATE, "xh_vds_cost: no pairs loaded");
    XH_HIP(hipSetDevice(h->ctx->device));
    VdsCoef C;
    const int l2 = zk_pack(h->L1, h->L2, h->vecSize, h_x, C.c);
    XH_TRY(vds_launch_cost(h, C, l2));
    XH_TRY(xh_reduce_finish(h->ctx, (const double *)h->partials.p, (int)h->grid, 3, (double *)h->result.p, h->pinned.f64()));
    const double count = (double)h->g.npairs * (double)h->g.N;
    const double *sums = h->pinned.f64();
    const double diff2 = sums[0] + h->outDiff2, sumVD = sums[1] + h->outSumVD, modg = sums[2];
    const double deformation = std::sqrt(modg / count);
    h_out[0] = std::sqrt(diff2 / count) + h->lambda * (deformation + std::fabs(h->sumVI - sumVD) / h->sumVI);
    h_out[1] = diff2;
    h_out[2] = sumVD;
    h_out[3] = modg;
    return XH_OK;
}

int xh_vds_refine_stage(xh_vds *h, int32_t l2_stage, double *h_x, double *fret, int32_t *iter, int64_t *evals)
{
    XH_CHECK(h && h_x && fret && iter, XH_ERR_ARG, "xh_vds_refine_stage: null argument");
    XH_CHECK(l2_stage >= 0 && l2_stage <= h->L2, XH_ERR_ARG, "xh_vds_refine_stage: stage %d outside 0 .. %d", l2_stage, h->L2);
    XH_CHECK(h->g.npairs > 0, XH_ERR_STATE, "xh_vds_refine_stage: no pairs loaded");
    // minimizepos: step 1 for the first numCoefficients(L1, stage) entries of each third
    const int nst = vds_num_terms(h->L1, l2_stage);
    VdsStage s{h, std::vector<double>(h_x, h_x + 3 * (size_t)h->vecSize), {}};
    for (int d = 0; d < 3; ++d)
        for (int idx = 0; idx < nst; ++idx) s.active.push_back(d * h->vecSize + idx);
    const int na = (int)s.active.size();
    std::vector<double> p((size_t)na), steps((size_t)na, 1.0);
    for (int a = 0; a < na; ++a) p[a] = s.x[s.active[a]];
    h->costRc = XH_OK;
    h->evals = 0;
    XH_TRY(xh_powell_minimize(na, p.data(), steps.data(), 0.01, vds_stage_cb, &s, fret, iter));
    XH_TRY(h->costRc);
    for (int a = 0; a < na; ++a) h_x[s.active[a]] = p[a];
    if (evals) *evals = h->evals;
    return XH_OK;
}

int xh_vds_apply(xh_vds *h, const double *h_raw, const double *h_x, double *h_VO, double *h_G)
{
    XH_CHECK(h && h_raw && h_x && h_VO, XH_ERR_ARG, "xh_vds_apply: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const size_t vb = h->B[0].bytes;
    VdsCoef C;
    zk_pack(h->L1, h->L2, h->vecSize, h_x, C.c);
    XH_HIP(hipMemcpyAsync(h->B[0].p, h_raw, vb, hipMemcpyHostToDevice, st));
    double *G = nullptr;
    if (h_G) {
        XH_TRY(xh_buf_reserve(h->ctx, h->G, 3 * vb));
        G = (double *)h->G.p;
    }
    XH_LAUNCH256(h->ctx, k_vds_apply, h->gridVol, (const double *)h->B[0].p, h->g, C, h->L1, h->L2, (double *)h->B[1].p, G);
    XH_HIP(hipMemcpyAsync(h_VO, h->B[1].p, vb, hipMemcpyDeviceToHost, st));
    if (h_G) XH_HIP(hipMemcpyAsync(h_G, G, 3 * vb, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

int xh_vds_strain(xh_vds *h, double *h_G, double *h_LS, double *h_LR)
{
    XH_CHECK(h && h_G && h_LS && h_LR, XH_ERR_ARG, "xh_vds_strain: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const size_t vb = h->B[0].bytes, N = h->g.N;
    XH_TRY(xh_buf_reserve(h->ctx, h->G, 3 * vb));
    double *G = (double *)h->G.p;
    XH_HIP(hipMemcpyAsync(G, h_G, 3 * vb, hipMemcpyHostToDevice, st));
    for (int c = 0; c < 3; ++c) XH_TRY(vds_gauss_dev(h, G + (size_t)c * N, 2.0));
    XH_HIP(hipMemsetAsync(h->B[0].p, 0, vb, st));
    XH_HIP(hipMemsetAsync(h->B[1].p, 0, vb, st));
    XH_LAUNCH256(h->ctx, k_vds_strain, h->gridVol, (const double *)G, h->g.Z, h->g.Y, h->g.X, (double *)h->B[0].p, (double *)h->B[1].p);
    XH_HIP(hipMemcpyAsync(h_G, G, 3 * vb, hipMemcpyDeviceToHost, st));
    XH_HIP(hipMemcpyAsync(h_LS, h->B[0].p, vb, hipMemcpyDeviceToHost, st));
    XH_HIP(hipMemcpyAsync(h_LR, h->B[1].p, vb, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

}  // extern "C"
