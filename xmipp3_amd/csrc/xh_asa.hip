// xh_asa.hip -- xmipp_angular_sph_alignment on the device (gfx950), fp64: for every particle a pose and a Zernike3D deformation of the
// reference volume, fitted by Powell's method over
//     cost = -correlationIndex(Ifilteredp, P, mask2D) + lambda (deformation + |sumV - sumVd| / sumV)
// with P the projection along z of the deformed, rotated volume.
// Reference: libraries/reconstruction/angular_sph_alignment.cpp -- preProcess (L120-188), tranformImageSph (L196-261), continuousSphCost
// (L263-289), processImage (L293-421), minimizepos / fillVectorTerms (L472-504), applyCTFImage / updateCTFImage (L506-528), deformVol
// (L530-609). The arithmetic contract is that CPU program's, in doubles. Its CUDA twin (reconstruction_adapt_cuda/
// angular_sph_alignment_gpu.cpp, reconstruction_cuda/cuda_angular_sph_alignment.cu) runs one launch per cost call and adds the projection
// with float atomics; here
//
//   the unit of device work is ONE EVALUATION FOR EACH OF MANY (particle, variables) ROWS, as in xh_ca2.hip: the rows go up through one
//   pinned buffer, a fixed sequence of launches evaluates all of them, four sums per row come back in one copy behind one stream wait
//   (XhRowEval of xh_lockstep.h, shared with xh_ca2.hip, as are the particle load, the filter kernel, the 2-D mask and the correlation
//   index of xh_image2d.h; the host side of the Zernike3D basis is xh_zernike.h's, shared with xh_vds.hip).
//
//   k_asa_project : grid (tiles of 256 projection columns, row). A thread owns one column (i, j), lanes along j, and walks k upwards:
//                   pos = R (j, i, k), g = sum c Z(pos / RDef) (vds_disp of xh_zernike.h), the mask at the truncated pos + g, the trilinear
//                   sample of V at pos + g. P(i, j) is a private sum in the order of the reference's k-outer loop: no atomics. The row's
//                   rotation and coefficients are read from the row buffer at compile-time offsets of a workgroup-uniform pointer (scalar
//                   loads). sumVd, modg and count leave as per-workgroup partials (xh_reduce.h) that k_asa_cost adds in a fixed order.
//                   Instantiated on (L1, L2); a row whose coefficients past the terms of (L1, h) are all exactly 0 runs the (L1, h)
//                   instantiation. The instantiation is chosen per row from the row's own coefficients (one launch per distinct h in the
//                   batch, the other rows' workgroups leave at once), so a row's bits never depend on what shares its batch.
//                   k is not split into segments: a split would change the order of the additions from the reference's, and a batch
//                   fills the device without it (D = 128: 64 workgroups per row); the grid depends on D alone.
//   FFT           : forward 2-D transforms of the planes (XhFft2d64), one multiply by the raised-cosine low pass times the row's CTF
//                   (xh_k_lowpass_ctf<XH_FACTOR_CTF>: FilterCTF's mask of applyCTFImage L506-519), inverse transforms.
//   k_asa_cost    : one workgroup per row: the partials' totals, then every pixel of mask2D takes Ifiltered at the inverse of A (LINEAR,
//                   DONT_WRAP, outside 0), then d_masked_correlation. The cost is assembled on the host in doubles.
//
// Deviations from the reference:
//  - r^2 is k^2 + i^2 + j^2 of the integer coordinates, not |R p|^2 of the rotated ones: a rotation keeps the norm, and the rounded
//    |R p|^2 puts every lattice point with k^2 + i^2 + j^2 = RDef^2 (D = 16, RDef = 8: (-8, 0, 0)) on either side of < by the rotation's
//    rounding.
//  - R^-1 is the transpose of the Euler matrix; the reference runs a general inverse.
//  - Every term counts in g; the reference skips the terms whose step is 0, whose coefficients are 0 in its own search.
//  - Powell is handed only the variables whose step is non-zero, as in xh_ca2 and xh_vds: the minimum agrees within ftol, not bit for bit.
//  - The reference writes clnm and totalDeformation from whatever Powell evaluated last; here the returned p is evaluated once more and
//    those values are written (xh_ca2 deviates the same way).
//  - Low pass and CTF are both real, even masks: they are applied in one transform pair, not two.
//  - An evaluation with count = 0 costs 1e38; the reference takes sqrt(0 / 0) there.
//  - sumV equal to 0 or non-finite is XH_ERR_ARG at create.
//  - Degrees above l1 = 5, l2 = 4 are XH_ERR_UNSUPPORTED, as in xh_vds; so are particles of another size than the volume. (A non-cubic
//    volume and a mask of another shape cannot be expressed at this interface; the program and the Python class refuse them.)
//  - The mask test is == 1, as in the reference. The mask stays the int32 array the reference holds (MultidimArray<int>).
#include "xh_common.h"
#include "xh_fft.h"
#include "xh_plan.h"
#include "xh_reduce.h"
#include "xh_ctf.h"
#include "xh_image2d.h"
#include "xh_zernike.h"
#include "xh_lockstep.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace {
// doubles per evaluation row on the device: R[9] (the inverse rotation), the coefficients in VdsCoef's layout [3 * 45], Ainv[6], particle,
// identity, CTF (0 none, 1 computed from the CtfSide that follows), CtfSide[18], the instantiation's l2
const int kRowCoef = 9, kRowA = kRowCoef + 3 * VDS_MAXT, kRowPart = kRowA + 6, kRowIdent = kRowPart + 1, kRowCtf = kRowIdent + 1,
          kRowSide = kRowCtf + 1, kRowL2 = kRowSide + 18, kRow = kRowL2 + 1;
static_assert(sizeof(VdsCoef) == 3 * VDS_MAXT * sizeof(double), "VdsCoef rides in an evaluation row");

struct AsaGeom : ZkDims {    // Z, Y, X: the volume (a cube of side D)
    int D, DD, tiles;        // tiles: workgroups of 256 columns per row
    int kmin, kmax;          // the logical k that can lie inside the ball, clipped to the volume
    double RDef2, iRDef;
};

// deformVol (L530-609) for one row: see the header
template <int L1, int L2>
__global__ void __launch_bounds__(256)
k_asa_project(const double *__restrict__ V, const int *__restrict__ M, const double *__restrict__ ev, const AsaGeom g, int l1, int l2,
              double *__restrict__ Praw, double *__restrict__ partials)
{
    const int e = blockIdx.y;
    const double *__restrict__ q = ev + (size_t)kRow * e;
    if ((int)q[kRowL2] != l2) return;      // uniform over the workgroup: this row belongs to another instantiation's launch
    const VdsCoef &C = *reinterpret_cast<const VdsCoef *>(q + kRowCoef);
    const double R0 = q[0], R1 = q[1], R2 = q[2], R3 = q[3], R4 = q[4], R5 = q[5], R6 = q[6], R7 = q[7], R8 = q[8];
    double acc[3] = {0.0, 0.0, 0.0};
    const int n = blockIdx.x * 256 + threadIdx.x, D = g.D, c = D / 2;
    if (n < g.DD) {
        const int pi = n / D, i = pi - c, j = n - pi * D - c;
        const int ij2 = i * i + j * j;
        double P = 0.0;
        for (int k = g.kmin; k <= g.kmax; ++k) {
            const double r2 = (double)(ij2 + k * k);
            if (!(r2 < g.RDef2)) continue;
            const double x = R0 * j + R1 * i + R2 * k, y = R3 * j + R4 * i + R5 * k, z = R6 * j + R7 * i + R8 * k;
            double gx, gy, gz;
            vds_disp<L1, L2>(C, l1, l2, x * g.iRDef, y * g.iRDef, z * g.iRDef, sqrt(r2) * g.iRDef, gx, gy, gz);
            const double sx = x + gx, sy = y + gy, sz = z + gz;
            // V_mask at ((int)sz, (int)sy, (int)sx), the C cast, 0 outside; a NaN and a position far off are outside before the cast
            if (!(fabs(sx) < 1e6 && fabs(sy) < 1e6 && fabs(sz) < 1e6)) continue;
            const int mj = (int)sx + c, mi = (int)sy + c, mk = (int)sz + c;
            if (mj < 0 || mj >= D || mi < 0 || mi >= D || mk < 0 || mk >= D) continue;
            if (M[((size_t)mk * D + mi) * D + mj] != 1) continue;
            const double v = vds_sample(V, g, sx, sy, sz);
            P += v;
            acc[0] += v;
            acc[1] += gx * gx + gy * gy + gz * gz;
            acc[2] += 1.0;
        }
        Praw[(size_t)e * g.DD + n] = P;
    }
    xh_block_partials(acc, partials + (size_t)e * 3 * g.tiles);
}

// tranformImageSph (L218-224) for one row per workgroup: the totals of the projection's partials, P = the real part of the filtered plane,
// Ifilteredp (0 outside mask2D), correlationIndex(Ifilteredp, P, mask2D) (0 where a sigma is below XMIPP_EQUAL_ACCURACY).
// out [m][4] = sumVd, modg, count, corr
__global__ void __launch_bounds__(256)
k_asa_cost(const double *__restrict__ ev, const double *__restrict__ Ifiltered, const xh_cd *__restrict__ F, const int *__restrict__ mask,
           const double *__restrict__ partials, int tiles, double *__restrict__ Pout, double *__restrict__ Ifp, double *__restrict__ out, int D,
           double nmask)
{
    __shared__ double red[1][256];
    const int e = blockIdx.x, tid = threadIdx.x, DD = D * D;
    const double *q = ev + (size_t)kRow * e;
    double tot[3];
    for (int c = 0; c < 3; ++c) {
        const double *p = partials + ((size_t)e * 3 + c) * tiles;
        double v = 0.0;
        for (int t = tid; t < tiles; t += 256) v += p[t];
        tot[c] = xh_block_sum(v, red);
    }
    double A[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) A[k] = q[kRowA + k];
    const double *V1 = Ifiltered + (size_t)q[kRowPart] * DD;
    const bool ident = q[kRowIdent] != 0.0;
    const xh_cd *Fe = F + (size_t)e * DD;
    double *Pe = Pout + (size_t)e * DD, *Ie = Ifp + (size_t)e * DD;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int n = tid; n < DD; n += 256) {
        const double p = Fe[n].x;
        double val = 0;
        if (mask[n]) {
            const int i = n / D, j = n - i * D;
            val = ident ? V1[n] : d_ca2_linear(V1, D, A, i, j);
            s0 += val; s1 += p; s2 += val * val; s3 += p * p;
        }
        Pe[n] = p;
        Ie[n] = val;
    }
    const double corr = d_masked_correlation(s0, s1, s2, s3, mask, Ie, Pe, DD, nmask, red);
    if (tid == 0) {
        out[4 * (size_t)e] = tot[0];
        out[4 * (size_t)e + 1] = tot[1];
        out[4 * (size_t)e + 2] = tot[2];
        out[4 * (size_t)e + 3] = corr;
    }
}

struct AsaParticle {
    double rot, tilt, psi, shiftX, shiftY;
    int flip, hasCTF;
    xh_ctf_params ctf;
};
}  // namespace

struct xh_asa {
    xh_ctx *ctx = nullptr;
    xh_asa_params prm;
    AsaGeom g = {};
    int D = 0, nmask = 0, L1 = 0, L2 = 0, vecSize = 0, nvars = 0;
    double RDef = 0, Rmax = 0, sumV = 0;
    XhRowEval ev;                                  // rows of kRow doubles up; sumVd, modg, count, corr per row down
    XhBuf d_vol, d_mask3, d_mask2, d_If, d_Praw, d_F, d_P, d_Ifp, d_partials;
    XhFft2d64 fft;
    std::vector<AsaParticle> parts;
    // refine's bookkeeping
    std::vector<int> active;
    std::vector<double> cur;                       // [particles][nvars]: the stage's frozen variables
    ~xh_asa()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
};

namespace {
// continuousSphCost's bound checks (L275-278) on the variables x; a non-finite variable never reaches the device
bool asa_out_of_bounds(const xh_asa *h, const double *x)
{
    for (int k = 0; k < h->nvars; ++k)
        if (!std::isfinite(x[k])) return true;
    const xh_asa_params &q = h->prm;
    const double *t = x + 3 * h->vecSize;
    if (q.max_shift > 0 && t[0] * t[0] + t[1] * t[1] > q.max_shift * q.max_shift) return true;
    if (q.max_angular_change > 0 &&
        (std::fabs(t[2]) > q.max_angular_change || std::fabs(t[3]) > q.max_angular_change || std::fabs(t[4]) > q.max_angular_change))
        return true;
    return false;
}

// one evaluation row (see kRow) from the variables x [nvars]
void asa_fill_row(const xh_asa *h, int part, const double *x, double *row)
{
    const AsaParticle &pt = h->parts[part];
    const int vs = h->vecSize;
    const double *t = x + 3 * vs;
    double E[9];
    xh_fp_euler(pt.rot + t[2], pt.tilt + t[3], pt.psi + t[4], E);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) row[r * 3 + c] = E[c * 3 + r];      // R^-1: the transpose
    row[kRowL2] = (double)zk_pack(h->L1, h->L2, vs, x, row + kRowCoef);
    // A (L280-285, L211-216): the identity with the translation, its whole first row negated by the flip; inverted for IS_NOT_INV
    const double f = pt.flip ? -1.0 : 1.0, tx = pt.shiftX + t[0], ty = pt.shiftY + t[1];
    double *A = row + kRowA;
    A[0] = f; A[1] = 0; A[2] = -tx; A[3] = 0; A[4] = 1; A[5] = -ty;
    row[kRowPart] = (double)part;
    // applyGeometry copies its input when A is the identity within XMIPP_EQUAL_ACCURACY
    row[kRowIdent] = (!pt.flip && std::fabs(tx) <= kAcc && std::fabs(ty) <= kAcc) ? 1.0 : 0.0;
    row[kRowCtf] = 0;
    if (pt.hasCTF) {
        xh_ctf_params c = pt.ctf;      // updateCTFImage (L521-528): K = 1
        c.K = 1;
        c.DeltafU = pt.ctf.DeltafU + t[5];
        c.DeltafV = pt.ctf.DeltafV + t[6];
        c.azimuthal_angle = pt.ctf.azimuthal_angle + t[7];
        const CtfSide s = side_info(c, true);
        row[kRowCtf] = 1;
        std::memcpy(row + kRowSide, &s, sizeof(s));
    } else
        for (int k = 0; k < 18; ++k) row[kRowSide + k] = 0.0;
}

int asa_launch_project(xh_asa *h, int m, int l2)
{
    const double *V = (const double *)h->d_vol.p, *ev = h->ev.dev_rows();
    const int *M = (const int *)h->d_mask3.p;
    double *Praw = (double *)h->d_Praw.p, *part = (double *)h->d_partials.p;
    const int l1 = h->L1;
    const dim3 grid((unsigned)h->g.tiles, (unsigned)m);
#define ASA_LAUNCH(A, B)                                                                                                   \
    do {                                                                                                                   \
        hipLaunchKernelGGL((k_asa_project<A, B>), grid, dim3(256), 0, h->ctx->stream, V, M, ev, h->g, l1, l2, Praw, part);  \
        XH_LAUNCH_CHECK();                                                                                                 \
    } while (0)
    ZK_DISPATCH(l1, l2, ASA_LAUNCH);
#undef ASA_LAUNCH
    return XH_OK;
}

// m <= capacity rows already in h->ev: upload, project, filter, cost, download; one stream wait
int asa_eval(xh_asa *h, int m)
{
    xh_ctx *ctx = h->ctx;
    const auto t1 = XhRowEval::now();
    XH_TRY(h->ev.upload(m));
    bool seen[VDS_MAX_L2 + 1] = {};
    for (int r = 0; r < m; ++r) seen[(int)h->ev.row(r)[kRowL2]] = true;
    for (int l2 = 0; l2 <= VDS_MAX_L2; ++l2)
        if (seen[l2]) XH_TRY(asa_launch_project(h, m, l2));
    const size_t total = (size_t)h->g.DD * m;
    const unsigned g = (unsigned)((total + 255) / 256);
    xh_cd *F = (xh_cd *)h->d_F.p;
    XH_LAUNCH256(ctx, xh_k_to_complex64<double>, g, (const double *)h->d_Praw.p, F, total);
    XH_TRY(xh_fft2d64(ctx, h->fft, F, m, false));
    XH_LAUNCH256(ctx, xh_k_lowpass_ctf<XH_FACTOR_CTF>, g, F, total, h->D, h->prm.sampling / h->prm.max_resolution, 0.02, h->ev.dev_rows(), kRow, kRowCtf,
                 1.0 / h->prm.sampling, (int)h->prm.phase_flipped);
    XH_TRY(xh_fft2d64(ctx, h->fft, F, m, true));
    XH_LAUNCH256(ctx, k_asa_cost, m, h->ev.dev_rows(), (const double *)h->d_If.p, (const xh_cd *)F, (const int *)h->d_mask2.p,
                 (const double *)h->d_partials.p, h->g.tiles, (double *)h->d_P.p, (double *)h->d_Ifp.p, (double *)h->ev.d_res.p, h->D, (double)h->nmask);
    XH_TRY(h->ev.download(m));
    h->ev.count(m, t1);      // every evaluation counts, a single cost call's too: xh_asa_stats reports the last cost or refine
    return XH_OK;
}

// tranformImageSph's return value (L256-257) from a row's sums s = sumVd, modg, count, corr
double asa_row_cost(const xh_asa *h, const double *s)
{
    if (!(s[2] > 0)) return kBarrier;      // count = 0: the reference takes sqrt(0 / 0)
    return -s[3] + h->prm.lambda * (std::sqrt(s[1] / s[2]) + std::fabs(h->sumV - s[0]) / h->sumV);
}

// m rows (any m): costs, and (nullable) each row's deformation sqrt(modg / count), 0 for a row that never reached the device
int asa_cost_rows(xh_asa *h, int m, const int32_t *particle, const double *vars, double *cost, double *deformation)
{
    return h->ev.cost_rows(
        m, [&](int r) { return asa_out_of_bounds(h, vars + (size_t)h->nvars * r); },      // no device work (L275-278)
        [&](int r, double *row) { asa_fill_row(h, particle[r], vars + (size_t)h->nvars * r, row); return XH_OK; }, [&](int k) { return asa_eval(h, k); },
        [&](int r, const double *s) {
            cost[r] = s ? asa_row_cost(h, s) : kBarrier;
            if (deformation) deformation[r] = s && s[2] > 0 ? std::sqrt(s[1] / s[2]) : 0.0;
        });
}

// the compact vector of a stage's search -> all the variables (the frozen ones keep the stage's starting values)
void asa_expand(const xh_asa *h, int part, const double *xc, double *x)
{
    xh_lockstep_expand(h->active, &h->cur[(size_t)part * h->nvars], h->nvars, xc, x);
}

int32_t asa_pre(int32_t problem, const double *xc, double *cost, void *user)
{
    xh_asa *h = (xh_asa *)user;
    std::vector<double> x((size_t)h->nvars);
    asa_expand(h, problem, xc, x.data());
    if (!asa_out_of_bounds(h, x.data())) return 0;
    *cost = kBarrier;
    return 1;
}

int32_t asa_batch(int32_t m, const int32_t *problem, const double *xc, double *cost, void *user)
{
    xh_asa *h = (xh_asa *)user;
    const int nact = (int)h->active.size();
    std::vector<double> x((size_t)h->nvars);
    for (int r = 0; r < m; ++r) {
        asa_expand(h, problem[r], xc + (size_t)r * nact, x.data());
        asa_fill_row(h, problem[r], x.data(), h->ev.row(r));
    }
    XH_TRY(asa_eval(h, m));
    for (int r = 0; r < m; ++r) cost[r] = asa_row_cost(h, h->ev.res(r));
    return 0;
}

// minimizepos (L472-482) and the steps of processImage (L351-358): the indices of the variables stage `stage` frees, ascending
void asa_stage(int L1, int vecSize, int stage, int flags, std::vector<int> &out)
{
    out.clear();
    if (flags & XH_ASA_OPT_DEFORMATION) {
        const int nst = vds_num_terms(L1, stage);
        for (int d = 0; d < 3; ++d)
            for (int idx = 0; idx < nst; ++idx) out.push_back(d * vecSize + idx);
    }
    if (flags & XH_ASA_OPT_ALIGNMENT)
        for (int k = 0; k < 5; ++k) out.push_back(3 * vecSize + k);
    if (flags & XH_ASA_OPT_DEFOCUS)
        for (int k = 5; k < 8; ++k) out.push_back(3 * vecSize + k);
}

int asa_flags(const xh_asa_params &q)
{
    return (q.optimize_deformation ? XH_ASA_OPT_DEFORMATION : 0) | (q.optimize_alignment ? XH_ASA_OPT_ALIGNMENT : 0) |
           (q.optimize_defocus ? XH_ASA_OPT_DEFOCUS : 0);
}
}  // namespace

extern "C" {

void xh_asa_defaults(xh_asa_params *p)
{
    if (!p) return;
    p->max_shift = -1; p->max_angular_change = 5; p->max_resolution = 4; p->sampling = 1; p->Rmax = -1; p->RDef = -1; p->lambda = 0.01;
    p->l1 = 3; p->l2 = 2;
    p->optimize_alignment = p->optimize_deformation = p->optimize_defocus = p->phase_flipped = 0;
}

int xh_asa_stage_active(int32_t L1, int32_t L2, int32_t stage, int32_t flags, int32_t *out, int32_t *n)
{
    XH_CHECK(out && n, XH_ERR_ARG, "xh_asa_stage_active: null argument");
    XH_TRY(zk_check_degrees("xh_asa_stage_active", L1, L2));
    XH_CHECK(stage >= 0 && stage <= L2, XH_ERR_ARG, "xh_asa_stage_active: stage %d outside 0 .. %d", stage, L2);
    XH_CHECK((flags & ~7) == 0, XH_ERR_ARG, "xh_asa_stage_active: unknown flags %d", flags);
    std::vector<int> a;
    asa_stage(L1, vds_num_terms(L1, L2), stage, flags, a);
    for (size_t k = 0; k < a.size(); ++k) out[k] = a[k];
    *n = (int32_t)a.size();
    return XH_OK;
}

int xh_asa_create(xh_ctx *ctx, const float *d_vol, int32_t D, const int32_t *h_mask, const xh_asa_params *prm, int32_t capacity, xh_asa **out)
{
    XH_CHECK(ctx && d_vol && prm && out && D >= 4 && capacity >= 1, XH_ERR_ARG, "xh_asa_create: bad argument");
    XH_CHECK(D <= 1024, XH_ERR_UNSUPPORTED, "xh_asa_create: sizes above 1024 are not supported (%d)", D);
    XH_CHECK(capacity <= 65535, XH_ERR_ARG, "xh_asa_create: capacity %d exceeds 65535 evaluations per step", capacity);
    XH_TRY(zk_check_degrees("xh_asa_create", prm->l1, prm->l2));
    XH_CHECK(prm->sampling > 0 && prm->max_resolution > 0, XH_ERR_ARG, "xh_asa_create: sampling %g / max_resolution %g must be positive", prm->sampling,
             prm->max_resolution);
    XH_CHECK(std::isfinite(prm->lambda) && std::isfinite(prm->RDef) && std::isfinite(prm->Rmax), XH_ERR_ARG, "xh_asa_create: lambda %g, RDef %g, Rmax %g",
             prm->lambda, prm->RDef, prm->Rmax);
    XH_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<xh_asa> h(new xh_asa);
    h->ctx = ctx; h->prm = *prm; h->D = D; h->L1 = prm->l1; h->L2 = prm->l2;
    h->vecSize = vds_num_terms(h->L1, h->L2);
    h->nvars = 3 * h->vecSize + 8;
    h->RDef = prm->RDef < 0 ? (double)(D / 2) : prm->RDef;      // preProcess L135-136
    h->Rmax = prm->Rmax < 0 ? (double)(D / 2) : prm->Rmax;      // L164-165
    XH_CHECK(h->RDef > 0, XH_ERR_ARG, "xh_asa_create: RDef %g must be positive", h->RDef);
    const size_t DD = (size_t)D * D, N = DD * D;
    // V as doubles; V_mask: the file's, or the sphere of radius RDef (L139-153); sumV over the mask in index order (L156-161)
    std::vector<float> vf(N);
    XH_HIP(hipMemcpy(vf.data(), d_vol, sizeof(float) * N, hipMemcpyDeviceToHost));
    std::vector<double> vd(vf.begin(), vf.end());
    std::vector<int32_t> mask3(N);
    if (h_mask) std::memcpy(mask3.data(), h_mask, sizeof(int32_t) * N);
    else XH_TRY(xh_halves_circular_mask(D, D, D, -h->RDef, 0, 0, 0, mask3.data()));
    double sumV = 0.0;
    for (size_t e = 0; e < N; ++e)
        if (mask3[e] == 1) sumV += vd[e];
    XH_CHECK(std::isfinite(sumV) && sumV != 0.0, XH_ERR_ARG, "xh_asa_create: the volume's mass inside the mask is %g", sumV);
    h->sumV = sumV;
    XH_TRY(xh_buf_upload(ctx, h->d_vol, vd.data(), sizeof(double) * N));
    XH_TRY(xh_buf_upload(ctx, h->d_mask3, mask3.data(), sizeof(int32_t) * N));
    // mask2D: BINARY_CIRCULAR_MASK, INNER_MASK, R1 = Rmax (L166-168)
    XH_TRY(xh_circular_mask2d(ctx, "xh_asa_create", D, h->Rmax, h->d_mask2, &h->nmask));
    AsaGeom &g = h->g;
    g.Z = g.Y = g.X = D; g.D = D; g.DD = (int)DD; g.tiles = (int)((DD + 255) / 256);
    g.RDef2 = h->RDef * h->RDef; g.iRDef = 1.0 / h->RDef;
    // r^2 < RDef^2 needs |k| <= ceil(RDef) - 1; clipped to the volume's logical range
    const int B = (int)std::min(2048.0, std::ceil(h->RDef)) - 1;
    g.kmin = std::max(-(D / 2), -B); g.kmax = std::min(D - 1 - D / 2, B);
    XH_TRY(xh_fft2d64_create(ctx, D, D, h->fft, "xh_asa_create"));
    XH_TRY(h->ev.create(ctx, capacity, kRow, 4));
    XH_TRY(xh_buf_alloc(ctx, h->d_Praw, sizeof(double) * DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->d_F, sizeof(xh_cd) * DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->d_P, sizeof(double) * DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->d_Ifp, sizeof(double) * DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->d_partials, sizeof(double) * 3 * g.tiles * capacity));
    *out = h.release();
    return XH_OK;
}

int xh_asa_destroy(xh_asa *h)
{
    delete h;
    return XH_OK;
}

int xh_asa_info(const xh_asa *h, double *RDef, double *Rmax, int32_t *vecSize, int32_t *nvars, double *sumV)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_asa_info: null handle");
    if (RDef) *RDef = h->RDef;
    if (Rmax) *Rmax = h->Rmax;
    if (vecSize) *vecSize = h->vecSize;
    if (nvars) *nvars = h->nvars;
    if (sumV) *sumV = h->sumV;
    return XH_OK;
}

static int asa_load(xh_asa *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_asa_row *rows)
{
    XH_CHECK(ydim == xdim, XH_ERR_UNSUPPORTED, "xh_asa_load: images must be square, got %d x %d", ydim, xdim);
    XH_CHECK(xdim == h->D, XH_ERR_UNSUPPORTED, "xh_asa_load: particles of size %d against a volume of size %d (rescaling is not done here)", xdim, h->D);
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const int D = h->D;
    const size_t DD = (size_t)D * D;
    h->parts.assign((size_t)n, AsaParticle());
    for (int i = 0; i < n; ++i) {
        const xh_asa_row &r = rows[i];
        if (r.has_ctf) {
            const double *c = reinterpret_cast<const double *>(&r.ctf);
            for (size_t k = 0; k < sizeof(xh_ctf_params) / sizeof(double); ++k)
                XH_CHECK(std::isfinite(c[k]), XH_ERR_ARG, "xh_asa_load: particle %d has a non-finite CTF parameter", i);
        }
        const double v[5] = {r.rot, r.tilt, r.psi, r.shift_x, r.shift_y};
        for (double q : v) XH_CHECK(std::isfinite(q), XH_ERR_ARG, "xh_asa_load: particle %d has a non-finite pose", i);
        AsaParticle &pt = h->parts[i];
        pt.rot = r.rot; pt.tilt = r.tilt; pt.psi = r.psi; pt.shiftX = r.shift_x; pt.shiftY = r.shift_y;
        pt.flip = r.flip != 0; pt.hasCTF = r.has_ctf != 0; pt.ctf = r.ctf;
    }
    // Ifiltered = the low pass of I (processImage L332-333), resident as doubles
    XH_TRY(xh_buf_alloc(ctx, h->d_If, sizeof(double) * DD * n));
    return xh_lowpass_images(ctx, h->fft, h_images, n, D, h->prm.sampling / h->prm.max_resolution, 1.0 / h->prm.sampling, nullptr, 0, 0,
                             (double *)h->d_If.p);
}

int xh_asa_load(xh_asa *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_asa_row *rows)
{
    XH_CHECK(h && h_images && rows && n >= 1, XH_ERR_ARG, "xh_asa_load: bad argument");
    h->ev.last_rows = 0;    // the images of the last evaluation belong to the particles that are being replaced
    const int rc = asa_load(h, h_images, n, ydim, xdim, rows);
    if (rc != XH_OK) h->parts.clear();      // a load that fails leaves no particles, not half-filled ones
    return rc;
}

int xh_asa_cost(xh_asa *h, int32_t m, const int32_t *h_particle, const double *h_vars, double *h_cost)
{
    XH_CHECK(h && h_particle && h_vars && h_cost && m >= 0, XH_ERR_ARG, "xh_asa_cost: bad argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    const int np = (int)h->parts.size();
    for (int r = 0; r < m; ++r) XH_CHECK(h_particle[r] >= 0 && h_particle[r] < np, XH_ERR_ARG, "xh_asa_cost: row %d names particle %d of %d", r, h_particle[r], np);
    const auto t0 = XhRowEval::now();
    h->ev.reset();
    XH_TRY(asa_cost_rows(h, m, h_particle, h_vars, h_cost, nullptr));
    h->ev.t_total = XhRowEval::since(t0);
    return XH_OK;
}

int xh_asa_last(xh_asa *h, int32_t row, double *d_P_raw, double *d_P, double *d_Ifilteredp, double *h_sums)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_asa_last: null handle");
    XH_CHECK(row >= 0 && row < h->ev.last_rows, XH_ERR_STATE, "xh_asa_last: row %d of the %d the last evaluation held", row, h->ev.last_rows);
    XH_HIP(hipSetDevice(h->ctx->device));
    const size_t bytes = sizeof(double) * h->D * h->D;
    hipStream_t st = h->ctx->stream;
    if (d_P_raw) XH_HIP(hipMemcpyAsync(d_P_raw, (const char *)h->d_Praw.p + bytes * row, bytes, hipMemcpyDeviceToDevice, st));
    if (d_P) XH_HIP(hipMemcpyAsync(d_P, (const char *)h->d_P.p + bytes * row, bytes, hipMemcpyDeviceToDevice, st));
    if (d_Ifilteredp) XH_HIP(hipMemcpyAsync(d_Ifilteredp, (const char *)h->d_Ifp.p + bytes * row, bytes, hipMemcpyDeviceToDevice, st));
    XH_HIP(hipStreamSynchronize(st));
    if (h_sums)
        for (int k = 0; k < 4; ++k) h_sums[k] = h->ev.res(row)[k];
    return XH_OK;
}

int xh_asa_refine(xh_asa *h, double *h_vars, double *h_cost, int32_t *h_enabled, double *h_deformation, int32_t *h_iter, int64_t *h_evals)
{
    XH_CHECK(h && h_vars && h_cost && h_enabled && h_deformation && h_iter && h_evals, XH_ERR_ARG, "xh_asa_refine: null argument");
    XH_CHECK(!h->parts.empty(), XH_ERR_STATE, "xh_asa_refine: no particles loaded");
    XH_CHECK(h->L2 >= 1, XH_ERR_ARG, "xh_asa_refine: l2 = %d leaves no stage to search (the stages are h = 1 .. l2)", h->L2);
    const int flags = asa_flags(h->prm);
    XH_CHECK(flags != 0, XH_ERR_ARG, "xh_asa_refine: no --optimize* flag is set, there is nothing to search");
    XH_HIP(hipSetDevice(h->ctx->device));
    const auto t0 = XhRowEval::now();
    const int np = (int)h->parts.size(), nv = h->nvars;
    h->cur.assign((size_t)np * nv, 0.0);      // p.initZeros (L297)
    for (int i = 0; i < np; ++i) { h_enabled[i] = 1; h_iter[i] = 0; h_evals[i] = 0; h_cost[i] = 0; }
    h->ev.reset();
    for (int stage = 1; stage <= h->L2; ++stage) {      // L335-415
        asa_stage(h->L1, h->vecSize, stage, flags, h->active);
        const int nact = (int)h->active.size();
        std::vector<int32_t> n((size_t)np, nact), it((size_t)np, 0);
        std::vector<double> p((size_t)np * nact), steps((size_t)np * nact, 1.0), fret((size_t)np, 0.0);
        std::vector<int64_t> ev((size_t)np, 0);
        for (int q = 0; q < np; ++q)
            for (int k = 0; k < nact; ++k) p[(size_t)q * nact + k] = h->cur[(size_t)q * nv + h->active[k]];
        XH_TRY(xh_powell_lockstep(np, n.data(), nact, p.data(), steps.data(), 0.01, h->ev.capacity, asa_batch, asa_pre, h, fret.data(), it.data(), ev.data()));
        for (int q = 0; q < np; ++q) {
            double *x = &h->cur[(size_t)q * nv];
            if (fret[q] > 0) {      // L369-373: disabled, p.initZeros(); the next stage still runs, from zero
                h_enabled[q] = -1;
                for (int k = 0; k < nv; ++k) x[k] = 0.0;
            } else
                for (int k = 0; k < nact; ++k) x[h->active[k]] = p[(size_t)q * nact + k];
            h_cost[q] = fret[q];
            h_iter[q] += it[q];
            h_evals[q] += ev[q];
        }
    }
    std::memcpy(h_vars, h->cur.data(), sizeof(double) * h->cur.size());
    // one more evaluation at the returned p: totalDeformation (see the header)
    std::vector<int32_t> idx((size_t)np);
    std::vector<double> c((size_t)np);
    for (int i = 0; i < np; ++i) idx[i] = i;
    XH_TRY(asa_cost_rows(h, np, idx.data(), h_vars, c.data(), h_deformation));
    h->ev.t_total = XhRowEval::since(t0);
    return XH_OK;
}

int xh_asa_stats(const xh_asa *h, double *h_stats)
{
    XH_CHECK(h && h_stats, XH_ERR_ARG, "xh_asa_stats: null argument");
    h->ev.stats(h_stats);
    return XH_OK;
}

}  // extern "C"
