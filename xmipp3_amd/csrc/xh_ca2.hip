// xh_ca2.hip -- xmipp_angular_continuous_assign2 on the device (gfx950): continuous refinement of each particle's pose (grey values,
// shift, scale, angles) by Powell's method over a projection-vs-particle cost.
// Reference: libraries/reconstruction/angular_continuous_assign2.cpp -- preProcess (L157-222), tranformImage (L251-345),
// continuous2cost (L348-395), processImage (L399-661). The arithmetic contract is that CPU program's; the device design is not its CUDA
// twin's (one projector call per cost evaluation per host thread), which is bound by launches:
//
//   the unit of device work is ONE EVALUATION FOR EACH OF MANY PARTICLES. Every particle owns a Powell search (the unchanged
//   powellOptimizer, paused at each cost call: host/powell_batch.h); at every step each live search asks for one parameter vector; the
//   rows go up through one pinned buffer, the device evaluates all of them in a fixed sequence of four launches, the costs come back in
//   one copy behind one stream wait.
//
//   load  : particles -> fp64, 2-D FFT (xh_plan.h line transforms), raised-cosine low pass w1 = Ts/maxResol, raised_w = 0.02
//           (fourier_filter.cpp:423-432, 710-716) times, where the particle has a CTF, the envelope image of generateEnvelope
//           (ctf.h:1271-1290) that processImage multiplies into the spectrum (L447-460), inverse -> Ifiltered, resident as doubles:
//           xh_lowpass_images and xh_k_lowpass_ctf<XH_FACTOR_ENVELOPE> of xh_image2d.h, shared with xh_asa.hip
//   cost  : (1) central slices of the projector's coefficient cubes at each row's own Euler matrix, (2) inverse along y, (3) c2r rows
//           -> P as doubles that never leave the device: these three are the projector's own kernels (xh_fp.hip, shared, not copied);
//           (4) k_ca2_cost, one workgroup per evaluation: every masked pixel takes Ifiltered at the inverse of A (LINEAR, DONT_WRAP,
//           outside 0), accumulates the sums of the cost, and the workgroup reduces them in a fixed order (strided partial sums, LDS
//           tree; no floating-point atomics), so a row's cost does not depend on what shares its batch.
//           Its correlation index is d_masked_correlation of xh_image2d.h.
// The row buffers, the chunked cost loop and the counters behind xh_ca2_stats are XhRowEval of xh_lockstep.h, shared with xh_asa.hip.
// All arithmetic is fp64, like the reference and xh_fp.hip.
#include "xh_common.h"
#include "xh_fft.h"
#include "xh_plan.h"
#include "xh_reduce.h"
#include "xh_ctf.h"
#include "xh_bspline.h"
#include "xh_image2d.h"
#include "xh_lockstep.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace {
// doubles per evaluation row on the device: E[9], Ainv[6], a, b, particle, identity, CTF mode (0 none, 1 the particle's resident image,
// 2 computed from the CtfSide that follows), CtfSide[18], pad
const int kEv = 40, kEvCtf = 19, kEvSide = 20;

// updateCTFImage (L225-247) for the rows of one evaluation: generateCTF with K = 1 on the half spectrum [D][D/2+1] (the part the projector
// reads), |.| when the particles were phase flipped. Mode 1 copies the image the particle keeps for its input defocus (the same function
// of the same numbers, so the same bits: a search that leaves the defocus alone never evaluates a CTF), mode 0 writes ones.
__global__ void __launch_bounds__(256)
k_ca2_ctf_rows(const double *__restrict__ ev, const double *__restrict__ ctfPart, double *__restrict__ out, int D, double iTs, int phaseFlipped)
{
    const int xh = D / 2 + 1, per = D * xh;
    const int t = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
    if (t >= per) return;
    const double *q = ev + (size_t)kEv * e;
    const int mode = (int)q[kEvCtf];
    double v = 1.0;
    if (mode == 1) v = ctfPart[(size_t)q[17] * per + t];
    else if (mode == 2) {
        D_CTF_SIDE_FROM_ROW(s, q + kEvSide)
        const int i = t / xh, j = t - i * xh;
        v = d_ctf_at(s, d_digfreq(j, D) * iTs, d_digfreq(i, D) * iTs, true);
        if (phaseFlipped) v = fabs(v);
    }
    out[(size_t)e * per + t] = v;
}

// tranformImage (L275-317): one workgroup per evaluation. Writes Ifilteredp (0 outside the mask), E, and the cost.
// l1: CONTCOST_L1 = mean over the mask of |a P + b - Ifilteredp|; else CONTCOST_CORR = -correlationIndex(Ifilteredp, P, mask), where a
// sigma below XMIPP_EQUAL_ACCURACY gives correlation 0.
__global__ void __launch_bounds__(256)
k_ca2_cost(const double *__restrict__ ev, const double *__restrict__ Ifiltered, const double *__restrict__ P, const int *__restrict__ mask,
           double *__restrict__ Ifp, double *__restrict__ E, double *__restrict__ cost, int D, int l1, double nmask)
{
    __shared__ double red[1][256];
    const int e = blockIdx.x, tid = threadIdx.x, DD = D * D;
    const double *q = ev + (size_t)kEv * e;
    double A[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) A[k] = q[9 + k];
    const double a = q[15], b = q[16];
    const double *V1 = Ifiltered + (size_t)q[17] * DD;
    const bool ident = q[18] != 0.0;
    const double *Pe = P + (size_t)e * DD;
    double *Ie = Ifp + (size_t)e * DD, *Ee = E + (size_t)e * DD;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int n = tid; n < DD; n += 256) {
        double val = 0, err = 0;
        if (mask[n]) {
            const int i = n / D, j = n - i * D;
            val = ident ? V1[n] : d_ca2_linear(V1, D, A, i, j);
            const double p = Pe[n];
            if (l1) {
                err = (a * p + b) - val;
                s0 += fabs(err);
            } else {
                err = p - val;
                s0 += val; s1 += p; s2 += val * val; s3 += p * p;
            }
        }
        Ie[n] = val;
        Ee[n] = err;
    }
    if (l1) {
        s0 = xh_block_sum(s0, red);
        if (tid == 0) cost[e] = s0 * (1.0 / nmask);      // cost *= iMask2Dsum (L314)
        return;
    }
    const double corr = d_masked_correlation(s0, s1, s2, s3, mask, Ie, Pe, DD, nmask, red);
    if (tid == 0) cost[e] = -corr;
}

// the final transform of processImage (L599-612): applyGeometry(BSPLINE3, ., A, IS_NOT_INV, DONT_WRAP) from the B-spline coefficients
// of the image, then (I - b) / a inside the mask and 0 outside when grey values were optimised. rows [n][10]: Ainv[6], identity, 1/a, b, pad
__global__ void __launch_bounds__(256)
k_ca2_apply(const double *__restrict__ coef, const float *__restrict__ img, const double *__restrict__ rows, const int *__restrict__ mask,
            float *__restrict__ out, int D, int gray)
{
    const int DD = D * D, e = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= DD) return;
    const double *q = rows + 10 * (size_t)e;
    double v;
    if (q[6] != 0.0) v = (double)img[(size_t)e * DD + n];       // applyGeometry copies its input when A is the identity
    else {
        const int i = n / D, j = n - i * D, cen = D / 2;
        const double minp = -cen - kAcc, maxp = (D - cen - 1) + kAcc;
        const double x = (double)(j - cen), y = (double)(i - cen);
        const double xp = x * q[0] + y * q[1] + q[2], yp = x * q[3] + y * q[4] + q[5];
        v = !(xp >= minp && xp <= maxp && yp >= minp && yp <= maxp) ? 0.0 : d_interp<double>(coef + (size_t)e * DD, D, xp, yp);
    }
    if (gray) v = mask[n] ? q[7] * (v - q[8]) : 0.0;
    out[(size_t)e * DD + n] = (float)v;
}

struct Particle {
    double rot, tilt, psi, shiftX, shiftY, grayA, grayB, Istddev;
    double p0[13];
    int flip, skipped;       // skipped: |old scale| > maxScale (L490-491)
    int hasCTF;
    xh_ctf_params ctf;       // as read from the row; old_defocusU / V / Angle are its DeltafU / DeltafV / azimuthal_angle
};

bool inv3(const double *A, double *B)
{
    const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    if (det == 0 || !std::isfinite(det)) return false;
    const double id = 1.0 / det;
    B[0] = (A[4] * A[8] - A[5] * A[7]) * id; B[1] = (A[2] * A[7] - A[1] * A[8]) * id; B[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    B[3] = (A[5] * A[6] - A[3] * A[8]) * id; B[4] = (A[0] * A[8] - A[2] * A[6]) * id; B[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    B[6] = (A[3] * A[7] - A[4] * A[6]) * id; B[7] = (A[1] * A[6] - A[0] * A[7]) * id; B[8] = (A[0] * A[4] - A[1] * A[3]) * id;
    return true;
}
}  // namespace

struct xh_ca2 {
    xh_ctx *ctx = nullptr;
    xh_ca2_params prm;
    int D = 0, nmask = 0, l1 = 0;
    xh_fp *fp = nullptr;
    XhRowEval ev;                                   // rows of kEv doubles up, one cost per row down
    XhBuf d_mask, d_If, d_P, d_Ifp, d_E;
    XhBuf d_ctfRow, d_ctfPart;                      // [capacity] and [particles] CTF images [D][D/2+1]; allocated when a particle has a CTF
    bool anyCTF = false;
    XhFft2d64 fft;                                  // the load's transforms
    std::vector<Particle> parts;
    std::vector<int> active;                        // the searched variables' indices into the 13
    std::vector<int> prob2part;                     // refine's problems: the particles that are not skipped
    ~xh_ca2()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        if (fp) xh_fp_destroy(fp);
    }
};

namespace {
// continuous2cost's bound checks (L364-375) on the 13 variables x (0-based)
bool ca2_out_of_bounds(const xh_ca2 *h, const Particle &pt, const double *x)
{
    const xh_ca2_params &q = h->prm;
    for (int k = 0; k < 13; ++k)
        if (!std::isfinite(x[k])) return true;      // a non-finite variable never reaches the device
    if (q.max_shift > 0 && x[2] * x[2] + x[3] * x[3] > q.max_shift * q.max_shift) return true;
    if (std::fabs(x[4]) > q.max_scale || std::fabs(x[5]) > q.max_scale) return true;
    if (std::fabs(x[7]) > q.max_angular_change || std::fabs(x[8]) > q.max_angular_change || std::fabs(x[9]) > q.max_angular_change) return true;
    if (std::fabs(x[0] - pt.grayA) > q.max_gray_scale) return true;
    if (std::fabs(x[1]) > q.max_gray_shift * pt.Istddev) return true;
    if (std::fabs(x[10]) > q.max_defocus_change || std::fabs(x[11]) > q.max_defocus_change) return true;
    return false;
}

// the CTF of tranformImage (L254-266) at the row's change of defocus: K = 1 (updateCTFImage), DeltafV = DeltafU when --sameDefocus
CtfSide ca2_side(const xh_ca2 *h, const Particle &pt, double dU, double dV, double dAngle, bool same_rule)
{
    xh_ctf_params c = pt.ctf;
    c.K = 1;
    c.DeltafU = pt.ctf.DeltafU + dU;
    c.DeltafV = (same_rule && h->prm.same_defocus) ? c.DeltafU : pt.ctf.DeltafV + dV;
    c.azimuthal_angle = pt.ctf.azimuthal_angle + dAngle;
    return side_info(c, true);
}

// A of L579-598 / L385-392 with the flip, inverted; *ident when it is the identity within XMIPP_EQUAL_ACCURACY
int ca2_matrix(const xh_ca2 *h, int part, const double *x, double *Ainv6, bool *ident)
{
    const Particle &pt = h->parts[part];
    const double scalex = x[4], scaley = x[5], scaleAngle = x[6];
    const double sin2_t = std::sin(scaleAngle) * std::sin(scaleAngle), sin_2t = std::sin(2 * scaleAngle);
    double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1}, B[9];
    A[0] = 1 + scalex + (scaley - scalex) * sin2_t;
    A[1] = 0.5 * (scaley - scalex) * sin_2t;
    A[3] = A[1];
    A[4] = 1 + scaley - (scaley - scalex) * sin2_t;
    A[2] = pt.shiftX + x[2];
    A[5] = pt.shiftY + x[3];
    if (pt.flip) { A[0] *= -1; A[1] *= -1; A[2] *= -1; }
    *ident = true;      // applyGeometry copies its input when A is the identity within XMIPP_EQUAL_ACCURACY
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            if (std::fabs(A[r * 3 + c] - (r == c ? 1.0 : 0.0)) > kAcc) *ident = false;
    XH_CHECK(inv3(A, B), XH_ERR_ARG, "xh_ca2: the transformation of particle %d is singular", part);
    for (int k = 0; k < 6; ++k) Ainv6[k] = B[k];
    return XH_OK;
}

// continuous2cost's A (L385-392), tranformImage's flip (L268-273), inverted for IS_NOT_INV; the row's Euler matrix
int ca2_fill_row(const xh_ca2 *h, int part, const double *x, double *row)
{
    const Particle &pt = h->parts[part];
    xh_fp_euler(pt.rot + x[7], pt.tilt + x[8], pt.psi + x[9], row);
    bool ident;
    XH_TRY(ca2_matrix(h, part, x, row + 9, &ident));
    row[15] = x[0];
    row[16] = x[1];
    row[17] = (double)part;
    row[18] = ident ? 1.0 : 0.0;
    row[kEvCtf] = 0;
    if (pt.hasCTF) {
        const bool moved = x[10] != 0 || (!h->prm.same_defocus && x[11] != 0) || x[12] != 0;
        row[kEvCtf] = moved ? 2 : 1;
        if (moved) {
            const CtfSide s = ca2_side(h, pt, x[10], x[11], x[12], true);
            std::memcpy(row + kEvSide, &s, sizeof(s));
        }
    }
    return XH_OK;
}

// m <= capacity rows already in h->ev: upload, project, cost, download; one stream wait
int ca2_eval(xh_ca2 *h, int m)
{
    xh_ctx *ctx = h->ctx;
    const double *d_ev = h->ev.dev_rows();
    XH_TRY(h->ev.upload(m));
    // the Euler matrix is the first 9 of a row's kEv doubles
    const size_t per = (size_t)h->D * (h->D / 2 + 1);
    if (h->anyCTF) {
        hipLaunchKernelGGL(k_ca2_ctf_rows, dim3((unsigned)((per + 255) / 256), m), dim3(256), 0, ctx->stream, d_ev,
                           (const double *)h->d_ctfPart.p, (double *)h->d_ctfRow.p, h->D, 1.0 / h->prm.sampling, h->prm.phase_flipped);
        XH_LAUNCH_CHECK();
    }
    XH_TRY(xh_fp_project_f64(h->fp, d_ev, kEv, m, h->anyCTF ? (const double *)h->d_ctfRow.p : nullptr, per, (double *)h->d_P.p));
    hipLaunchKernelGGL(k_ca2_cost, dim3(m), dim3(256), 0, ctx->stream, d_ev, (const double *)h->d_If.p,
                       (const double *)h->d_P.p, (const int *)h->d_mask.p, (double *)h->d_Ifp.p, (double *)h->d_E.p, (double *)h->ev.d_res.p,
                       h->D, h->l1, (double)h->nmask);
    XH_LAUNCH_CHECK();
    return h->ev.download(m);
}

// the compact vector of a search -> the reference's 13 (frozen variables keep their starting values)
void ca2_expand(const xh_ca2 *h, int part, const double *xc, double *x13)
{
    xh_lockstep_expand(h->active, h->parts[part].p0, 13, xc, x13);
}

int32_t ca2_pre(int32_t problem, const double *xc, double *cost, void *user)
{
    xh_ca2 *h = (xh_ca2 *)user;
    const int part = h->prob2part[problem];
    double x[13];
    ca2_expand(h, part, xc, x);
    if (!ca2_out_of_bounds(h, h->parts[part], x)) return 0;
    *cost = kBarrier;
    return 1;
}

int32_t ca2_batch(int32_t m, const int32_t *problem, const double *xc, double *cost, void *user)
{
    xh_ca2 *h = (xh_ca2 *)user;
    const int nact = (int)h->active.size();
    for (int r = 0; r < m; ++r) {
        const int part = h->prob2part[problem[r]];
        double x[13];
        ca2_expand(h, part, xc + (size_t)r * nact, x);
        XH_TRY(ca2_fill_row(h, part, x, h->ev.row(r)));
    }
    const auto t1 = XhRowEval::now();
    XH_TRY(ca2_eval(h, m));
    for (int r = 0; r < m; ++r) cost[r] = *h->ev.res(r);
    h->ev.count(m, t1);
    return 0;
}
}  // namespace

extern "C" {

void xh_ca2_defaults(xh_ca2_params *p)
{
    if (!p) return;
    p->max_shift = -1; p->max_scale = 0.02; p->max_angular_change = 5; p->max_defocus_change = 500; p->max_resolution = 4;
    p->max_gray_scale = 0.05; p->max_gray_shift = 0.05; p->sampling = 1; p->Rmax = -1; p->padding = 2;
    p->optimize_gray = p->optimize_shift = p->optimize_scale = p->optimize_angles = p->optimize_defocus = 0;
    p->phase_flipped = p->same_defocus = 0;
}

int xh_ca2_create(xh_ctx *ctx, const float *d_vol, int32_t D, const xh_ca2_params *prm, int32_t capacity, xh_ca2 **out)
{
    XH_CHECK(ctx && d_vol && prm && out && D >= 4 && capacity >= 1, XH_ERR_ARG, "xh_ca2_create: bad argument");
    XH_CHECK(capacity <= 65535, XH_ERR_ARG, "xh_ca2_create: capacity %d exceeds 65535 evaluations per step", capacity);
    XH_CHECK(prm->sampling > 0 && prm->max_resolution > 0, XH_ERR_ARG, "xh_ca2_create: sampling %g / max_resolution %g must be positive",
             prm->sampling, prm->max_resolution);
    XH_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<xh_ca2> h(new xh_ca2);
    h->ctx = ctx; h->prm = *prm; h->D = D;
    h->l1 = prm->optimize_gray ? 1 : 0;         // contCost (L218-221)
    // the projector of preProcess (L203-207): the coefficient cubes are xh_fp_create's own
    XH_TRY(xh_fp_create(ctx, d_vol, D, prm->padding, prm->sampling / prm->max_resolution, 3, &h->fp));
    XH_TRY(xh_fft2d64_create(ctx, D, D, h->fft, "xh_ca2_create"));
    // BINARY_CIRCULAR_MASK, INNER_MASK, R1 = Rmax about the Xmipp origin (L179-187)
    const double R = prm->Rmax < 0 ? (double)(D / 2) : prm->Rmax;
    XH_TRY(xh_circular_mask2d(ctx, "xh_ca2_create", D, R, h->d_mask, &h->nmask));
    const size_t DD = (size_t)D * D;
    XH_TRY(h->ev.create(ctx, capacity, kEv, 1));
    XH_TRY(xh_buf_alloc(ctx, h->d_P, sizeof(double) * DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->d_Ifp, sizeof(double) * DD * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->d_E, sizeof(double) * DD * capacity));
    // size the projector's scratch now, so that no evaluation allocates
    XH_HIP(hipMemsetAsync(h->ev.d_rows.p, 0, h->ev.d_rows.bytes, ctx->stream));
    XH_TRY(xh_fp_project_f64(h->fp, h->ev.dev_rows(), kEv, capacity, nullptr, 0, (double *)h->d_P.p));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    // the searched variables (L498-521): only those whose step is non-zero
    if (prm->optimize_gray) { h->active.push_back(0); h->active.push_back(1); }
    if (prm->optimize_shift) { h->active.push_back(2); h->active.push_back(3); }
    if (prm->optimize_scale) { h->active.push_back(4); h->active.push_back(5); h->active.push_back(6); }
    if (prm->optimize_angles) { h->active.push_back(7); h->active.push_back(8); h->active.push_back(9); }
    if (prm->optimize_defocus) {            // L507-520: with --sameDefocus the step of defocusV stays 0
        h->active.push_back(10);
        if (!prm->same_defocus) h->active.push_back(11);
        h->active.push_back(12);
    }
    *out = h.release();
    return XH_OK;
}

int xh_ca2_destroy(xh_ca2 *h)
{
    delete h;
    return XH_OK;
}

static int ca2_load(xh_ca2 *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_ca2_row *rows)
{
    XH_CHECK(ydim == xdim, XH_ERR_UNSUPPORTED, "xh_ca2_load: images must be square, got %d x %d", ydim, xdim);
    XH_CHECK(xdim == h->D, XH_ERR_UNSUPPORTED, "xh_ca2_load: particles of size %d against a volume of size %d (rescaling is not done here)", xdim,
             h->D);
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const int D = h->D;
    const size_t DD = (size_t)D * D;
    h->parts.assign((size_t)n, Particle());
    h->anyCTF = false;
    for (int i = 0; i < n; ++i) {
        if (rows[i].has_ctf) {
            const double *c = reinterpret_cast<const double *>(&rows[i].ctf);
            for (size_t k = 0; k < sizeof(xh_ctf_params) / sizeof(double); ++k)
                XH_CHECK(std::isfinite(c[k]), XH_ERR_ARG, "xh_ca2_load: particle %d has a non-finite CTF parameter", i);
        }
        const double v[8] = {rows[i].rot, rows[i].tilt, rows[i].psi, rows[i].shift_x, rows[i].shift_y, rows[i].scale_x, rows[i].scale_y, rows[i].scale_angle};
        for (double q : v) XH_CHECK(std::isfinite(q), XH_ERR_ARG, "xh_ca2_load: particle %d has a non-finite pose", i);
        XH_CHECK(std::isfinite(rows[i].gray_a) && std::isfinite(rows[i].gray_b), XH_ERR_ARG, "xh_ca2_load: particle %d has non-finite grey values", i);
        h->parts[i].hasCTF = rows[i].has_ctf != 0;
        h->parts[i].ctf = rows[i].ctf;
        h->anyCTF = h->anyCTF || h->parts[i].hasCTF;
    }
    const size_t per = (size_t)D * (D / 2 + 1);
    const double iTs = 1.0 / h->prm.sampling;
    XH_TRY(xh_buf_alloc(ctx, h->d_If, sizeof(double) * DD * n));
    XH_TRY(xh_buf_alloc(ctx, h->d_ctfPart, h->anyCTF ? sizeof(double) * per * n : 0));
    XH_TRY(xh_buf_alloc(ctx, h->d_ctfRow, h->anyCTF ? sizeof(double) * per * h->ev.capacity : 0));
    XhBuf d_rows;
    if (h->anyCTF) {
        // per particle an evaluation-style row holding its CtfSide: first the CTF image at the input defocus (what an evaluation that
        // leaves the defocus alone reads), then the side info of the envelope, which the reference takes before the --sameDefocus rule
        std::vector<double> hr((size_t)kEv * n, 0.0);
        for (int pass = 0; pass < 2; ++pass) {
            for (int i = 0; i < n; ++i) {
                if (!h->parts[i].hasCTF) continue;
                hr[(size_t)kEv * i + kEvCtf] = 2;
                const CtfSide s = ca2_side(h, h->parts[i], 0, 0, 0, pass == 0);
                std::memcpy(&hr[(size_t)kEv * i + kEvSide], &s, sizeof(s));
            }
            XH_TRY(xh_buf_upload(ctx, d_rows, hr.data(), sizeof(double) * hr.size()));
            if (pass == 0) {
                for (int i0 = 0; i0 < n; i0 += 32768) {      // one grid row per particle
                    hipLaunchKernelGGL(k_ca2_ctf_rows, dim3((unsigned)((per + 255) / 256), std::min(32768, n - i0)), dim3(256), 0, ctx->stream,
                                       (const double *)d_rows.p + (size_t)kEv * i0, (const double *)nullptr, (double *)h->d_ctfPart.p + per * i0, D,
                                       iTs, h->prm.phase_flipped);
                    XH_LAUNCH_CHECK();
                }
                XH_HIP(hipStreamSynchronize(ctx->stream));
            }
        }
    }
    XH_TRY(xh_lowpass_images(ctx, h->fft, h_images, n, D, h->prm.sampling / h->prm.max_resolution, iTs, (const double *)d_rows.p, kEv, kEvCtf,
                             (double *)h->d_If.p));
    for (int i = 0; i < n; ++i) {
        Particle &pt = h->parts[i];
        const xh_ca2_row &r = rows[i];
        pt.rot = r.rot; pt.tilt = r.tilt; pt.psi = r.psi; pt.shiftX = r.shift_x; pt.shiftY = r.shift_y; pt.flip = r.flip != 0;
        pt.grayA = h->prm.optimize_gray ? r.gray_a : 1.0;      // old_grayA is read only when grey values are optimised (L441-445)
        pt.grayB = h->prm.optimize_gray ? r.gray_b : 0.0;
        // Istddev = I().computeStddev() (L416), the population sigma in doubles; it only scales the bound on the grey shift
        const float *im = h_images + DD * i;
        double s = 0, s2 = 0;
        for (size_t k = 0; k < DD; ++k) { s += im[k]; s2 += (double)im[k] * im[k]; }
        const double avg = s / DD;
        pt.Istddev = std::sqrt(std::fabs(s2 / DD - avg * avg));
        for (int k = 0; k < 13; ++k) pt.p0[k] = 0;
        pt.p0[0] = pt.grayA; pt.p0[1] = pt.grayB;               // L466-478
        pt.p0[4] = r.scale_x; pt.p0[5] = r.scale_y; pt.p0[6] = r.scale_angle;
        pt.skipped = std::fabs(r.scale_x) > h->prm.max_scale || std::fabs(r.scale_y) > h->prm.max_scale;
    }
    return XH_OK;
}

int xh_ca2_load(xh_ca2 *h, const float *h_images, int32_t n, int32_t ydim, int32_t xdim, const xh_ca2_row *rows)
{
    XH_CHECK(h && h_images && rows && n >= 1, XH_ERR_ARG, "xh_ca2_load: bad argument");
    h->ev.last_rows = 0;    // the images of the last evaluation belong to the particles that are being replaced
    const int rc = ca2_load(h, h_images, n, ydim, xdim, rows);
    if (rc != XH_OK) h->parts.clear();      // a load that fails leaves no particles, not half-filled ones
    return rc;
}

int xh_ca2_cost(xh_ca2 *h, int32_t m, const int32_t *h_particle, const double *h_vars, double *h_cost)
{
    XH_CHECK(h && h_particle && h_vars && h_cost && m >= 0, XH_ERR_ARG, "xh_ca2_cost: bad argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    const int np = (int)h->parts.size();
    for (int r = 0; r < m; ++r) XH_CHECK(h_particle[r] >= 0 && h_particle[r] < np, XH_ERR_ARG, "xh_ca2_cost: row %d names particle %d of %d", r, h_particle[r], np);
    // a row out of bounds costs the barrier and takes no device work (L364-375); xh_ca2_stats goes on reporting the last refine
    return h->ev.cost_rows(
        m, [&](int r) { return ca2_out_of_bounds(h, h->parts[h_particle[r]], h_vars + 13 * (size_t)r); },
        [&](int r, double *row) { return ca2_fill_row(h, h_particle[r], h_vars + 13 * (size_t)r, row); }, [&](int k) { return ca2_eval(h, k); },
        [&](int r, const double *res) { h_cost[r] = res ? *res : kBarrier; });
}

int xh_ca2_last_images(xh_ca2 *h, int32_t row, double *d_P, double *d_E, double *d_Ifilteredp)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_ca2_last_images: null handle");
    XH_CHECK(row >= 0 && row < h->ev.last_rows, XH_ERR_STATE, "xh_ca2_last_images: row %d of the %d the last evaluation held", row, h->ev.last_rows);
    XH_HIP(hipSetDevice(h->ctx->device));
    const size_t bytes = sizeof(double) * h->D * h->D;
    hipStream_t st = h->ctx->stream;
    if (d_P) XH_HIP(hipMemcpyAsync(d_P, (const char *)h->d_P.p + bytes * row, bytes, hipMemcpyDeviceToDevice, st));
    if (d_E) XH_HIP(hipMemcpyAsync(d_E, (const char *)h->d_E.p + bytes * row, bytes, hipMemcpyDeviceToDevice, st));
    if (d_Ifilteredp) XH_HIP(hipMemcpyAsync(d_Ifilteredp, (const char *)h->d_Ifp.p + bytes * row, bytes, hipMemcpyDeviceToDevice, st));
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

int xh_ca2_measures(xh_ca2 *h, int32_t row, double *h_out)
{
    XH_CHECK(h && h_out, XH_ERR_ARG, "xh_ca2_measures: null argument");
    XH_CHECK(row >= 0 && row < h->ev.last_rows, XH_ERR_STATE, "xh_ca2_measures: row %d of the %d the last evaluation held", row, h->ev.last_rows);
    XH_HIP(hipSetDevice(h->ctx->device));
    const int D = h->D;
    const size_t N = (size_t)D * D;
    std::vector<double> P(N), I(N);
    XH_HIP(hipMemcpyAsync(P.data(), (const double *)h->d_P.p + N * row, sizeof(double) * N, hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipMemcpyAsync(I.data(), (const double *)h->d_Ifp.p + N * row, sizeof(double) * N, hipMemcpyDeviceToHost, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    // once per particle, after the search: sequential host sums in the reference's order
    // correlationIndex(P, Ifilteredp) without mask: population sigmas, 0 when one is below XMIPP_EQUAL_ACCURACY
    {
        double mx = 0, my = 0, sx = 0, sy = 0;
        for (size_t n = 0; n < N; ++n) { mx += P[n]; sx += P[n] * P[n]; my += I[n]; sy += I[n] * I[n]; }
        mx /= N; my /= N;
        sx = std::sqrt(std::fabs(sx / N - mx * mx));
        sy = std::sqrt(std::fabs(sy / N - my * my));
        double r = 0;
        if (!(std::fabs(sx) < kAcc || std::fabs(sy) < kAcc)) {
            for (size_t n = 0; n < N; ++n) r += (P[n] - mx) * (I[n] - my);
            r /= (sx * sy) * N;
        }
        h_out[0] = r;
    }
    // correlationMasked (filters.cpp:1397-1452): the pixels of P at or above its standard deviation give the means, those above it the sums
    {
        double m1 = 0, s1 = 0;
        for (size_t n = 0; n < N; ++n) { m1 += P[n]; s1 += P[n] * P[n]; }
        m1 /= N;
        const double th1 = std::sqrt(std::fabs(s1 / N - m1 * m1));
        double N1 = 0, sum1 = 0, sum2 = 0;
        for (size_t n = 0; n < N; ++n)
            if (P[n] >= th1) { sum1 += P[n]; sum2 += I[n]; N1 += 1.0; }
        double r = 0;
        if (N1 > 0) {
            const double iN1 = 1.0 / N1, a1 = sum1 * iN1, a2 = sum2 * iN1;
            double s11 = 0, s22 = 0, s12 = 0;
            for (size_t n = 0; n < N; ++n)
                if (P[n] > th1) {
                    const double p1a = P[n] - a1, p2a = I[n] - a2;
                    s11 += p1a * p1a; s22 += p2a * p2a; s12 += p1a * p2a;
                }
            r = s12 / std::sqrt(s11 * s22);
            if (!std::isfinite(r)) r = 0;       // no pixel above the threshold, or a flat image: the reference divides 0 by 0
        }
        h_out[1] = r;
    }
    // imedDistance (filters.cpp:1269-1318): the 7 x 7 weights exp(-(x^2 + y^2) / 2) / sqrt(2 pi) from their formula
    {
        double w[49];
        for (int a = -3; a <= 3; ++a)
            for (int b = -3; b <= 3; ++b) w[(a + 3) * 7 + (b + 3)] = std::exp(-0.5 * (a * a + b * b)) / std::sqrt(2.0 * 3.14159265358979323846);
        const int mid = D / 2, R2max = mid * mid;
        double imed = 0;
        for (int i = 3; i < D - 3; ++i)
            for (int j = 3; j < D - 3; ++j) {
                if ((i - mid) * (i - mid) + (j - mid) * (j - mid) > R2max) continue;
                const double diffi = P[(size_t)i * D + j] - I[(size_t)i * D + j];
                for (int ii = -3; ii <= 3; ++ii) {
                    double aux = 0;
                    for (int jj = -3; jj <= 3; ++jj)
                        aux += w[(ii + 3) * 7 + (jj + 3)] * (P[(size_t)(i + ii) * D + j + jj] - I[(size_t)(i + ii) * D + j + jj]);
                    imed += aux * diffi;
                }
            }
        h_out[2] = std::sqrt(imed);
    }
    return XH_OK;
}

int xh_ca2_apply(xh_ca2 *h, const float *h_images, const double *h_vars, float *h_out)
{
    XH_CHECK(h && h_images && h_vars && h_out, XH_ERR_ARG, "xh_ca2_apply: null argument");
    XH_CHECK(!h->parts.empty(), XH_ERR_STATE, "xh_ca2_apply: no particles loaded");
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const int D = h->D, n = (int)h->parts.size();
    const size_t DD = (size_t)D * D;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min(n, 32768), ((size_t)256 << 20) / (DD * sizeof(double))));
    XhBuf d_img, d_coef, d_rows, d_out;
    XH_TRY(xh_buf_alloc(ctx, d_img, sizeof(float) * DD * chunk));
    XH_TRY(xh_buf_alloc(ctx, d_out, sizeof(float) * DD * chunk));
    XH_TRY(xh_buf_alloc(ctx, d_coef, sizeof(double) * DD * chunk));
    XH_TRY(xh_buf_alloc(ctx, d_rows, sizeof(double) * 10 * chunk));
    std::vector<double> rows(10 * (size_t)chunk);
    const int TR = std::max(1, std::min(32, (int)(60000 / ((D + 1) * sizeof(double)))));
    const int tiles = (D + TR - 1) / TR;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        for (int r = 0; r < m; ++r) {
            const double *x = h_vars + 13 * (size_t)(i0 + r);
            double *q = &rows[10 * (size_t)r];
            bool ident;
            XH_TRY(ca2_matrix(h, i0 + r, x, q, &ident));
            q[6] = ident ? 1.0 : 0.0;
            q[7] = 1.0 / x[0];
            q[8] = x[1];
            q[9] = 0;
        }
        XH_HIP(hipMemcpyAsync(d_img.p, h_images + DD * i0, sizeof(float) * DD * m, hipMemcpyHostToDevice, ctx->stream));
        XH_HIP(hipMemcpyAsync(d_rows.p, rows.data(), sizeof(double) * 10 * m, hipMemcpyHostToDevice, ctx->stream));
        // produceSplineCoefficients(BSPLINE3) in doubles: rows through LDS tiles, then columns
        hipLaunchKernelGGL((k_pm_prefilter_rows<double, float>), dim3(m * tiles), dim3(64), sizeof(double) * TR * (D + 1), ctx->stream,
                           (const float *)d_img.p, (const int *)nullptr, (double *)d_coef.p, D, TR, (const int *)nullptr);
        hipLaunchKernelGGL((k_pm_prefilter_cols<double>), dim3((m * D + 63) / 64), dim3(64), 0, ctx->stream, (double *)d_coef.p, D, m,
                           (const int *)nullptr);
        hipLaunchKernelGGL(k_ca2_apply, dim3((unsigned)((DD + 255) / 256), m), dim3(256), 0, ctx->stream, (const double *)d_coef.p,
                           (const float *)d_img.p, (const double *)d_rows.p, (const int *)h->d_mask.p, (float *)d_out.p, D, h->l1);
        XH_LAUNCH_CHECK();
        XH_HIP(hipMemcpyAsync(h_out + DD * i0, d_out.p, sizeof(float) * DD * m, hipMemcpyDeviceToHost, ctx->stream));
        XH_HIP(hipStreamSynchronize(ctx->stream));
    }
    return XH_OK;
}

int xh_ca2_filtered(xh_ca2 *h, int32_t particle, double *h_out, double *h_stddev)
{
    XH_CHECK(h && particle >= 0 && particle < (int)h->parts.size(), XH_ERR_ARG, "xh_ca2_filtered: bad argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    const size_t bytes = sizeof(double) * h->D * h->D;
    if (h_out) {
        XH_HIP(hipMemcpyAsync(h_out, (const char *)h->d_If.p + bytes * particle, bytes, hipMemcpyDeviceToHost, h->ctx->stream));
        XH_HIP(hipStreamSynchronize(h->ctx->stream));
    }
    if (h_stddev) *h_stddev = h->parts[particle].Istddev;
    return XH_OK;
}

int xh_ca2_refine(xh_ca2 *h, double *h_vars, double *h_cost, int32_t *h_iter, int64_t *h_evals, int32_t *h_enabled)
{
    XH_CHECK(h && h_vars && h_cost && h_iter && h_evals && h_enabled, XH_ERR_ARG, "xh_ca2_refine: null argument");
    XH_CHECK(!h->parts.empty(), XH_ERR_STATE, "xh_ca2_refine: no particles loaded");
    XH_CHECK(!h->active.empty(), XH_ERR_ARG, "xh_ca2_refine: no --optimize* flag is set, there is nothing to search");
    XH_HIP(hipSetDevice(h->ctx->device));
    const auto t0 = XhRowEval::now();
    const int np = (int)h->parts.size(), nact = (int)h->active.size();
    h->prob2part.clear();
    for (int i = 0; i < np; ++i) {
        const Particle &pt = h->parts[i];
        for (int k = 0; k < 13; ++k) h_vars[13 * (size_t)i + k] = pt.p0[k];
        h_cost[i] = -1; h_iter[i] = 0; h_evals[i] = 0;        // cost = -1 and disabled when the input scale is out of bounds (L489-491)
        h_enabled[i] = pt.skipped ? -1 : 1;
        if (!pt.skipped) h->prob2part.push_back(i);
    }
    const int nprob = (int)h->prob2part.size();
    std::vector<int32_t> nv((size_t)nprob, nact), it((size_t)nprob, 0);
    std::vector<double> p((size_t)nprob * nact), steps((size_t)nprob * nact, 1.0), fret((size_t)nprob, 0.0);
    std::vector<int64_t> ev((size_t)nprob, 0);
    for (int q = 0; q < nprob; ++q)
        for (int k = 0; k < nact; ++k) p[(size_t)q * nact + k] = h->parts[h->prob2part[q]].p0[h->active[k]];
    h->ev.reset();
    XH_TRY(xh_powell_lockstep(nprob, nv.data(), nact, p.data(), steps.data(), 0.01, h->ev.capacity, ca2_batch, ca2_pre, h, fret.data(), it.data(),
                              ev.data()));
    for (int q = 0; q < nprob; ++q) {
        const int i = h->prob2part[q];
        h_cost[i] = fret[q]; h_iter[i] = it[q]; h_evals[i] = ev[q];
        // L523-540: a search that ends on the barrier, or at a positive correlation cost, is disabled and keeps its input variables
        if (fret[q] > 1e30 || (fret[q] > 0 && !h->l1)) h_enabled[i] = -1;
        else
            for (int k = 0; k < nact; ++k) h_vars[13 * (size_t)i + h->active[k]] = p[(size_t)q * nact + k];
        // L654-655 (the reference adds p(11) to the old defocus U as well; kept)
        const Particle &pt = h->parts[i];
        if (pt.hasCTF && (pt.ctf.DeltafU + h_vars[13 * (size_t)i + 10] < 0 || pt.ctf.DeltafU + h_vars[13 * (size_t)i + 11] < 0)) h_enabled[i] = -1;
    }
    h->ev.t_total = XhRowEval::since(t0);
    return XH_OK;
}

int xh_ca2_stats(const xh_ca2 *h, double *h_stats)
{
    XH_CHECK(h && h_stats, XH_ERR_ARG, "xh_ca2_stats: null argument");
    h->ev.stats(h_stats);
    return XH_OK;
}

}  // extern "C"
