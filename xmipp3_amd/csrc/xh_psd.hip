// xh_psd.hip -- the power spectrum of a micrograph by periodogram averaging over overlapping pieces, the device side of two programs:
//   double  xmipp_ctf_estimate_from_micrograph --dont_estimate_ctf (reconstruction/ctf_estimate_from_micrograph.cpp, run() :289-584)
//   float   xmipp_psd_estimate (reconstruction/psd_estimator.cpp, estimatePSD :74-148)
// One kernel set templated on the element type, no FMA contraction: every value is formed with the reference's roundings, and the
// deviation of normalize_ramp feeds a comparison (> 1e-6).
//
// The micrograph stays on the device in its file type, float32; float -> double is exact, so it is widened on load and no piece is ever
// copied out. Pieces arrive as a list of top-left corners and run `capacity` at a time.
//
//   k_psd_stats  one workgroup per piece, straight out of the micrograph window, every sum through the fixed tree of xh_reduce.h:
//                pass 1  sum and sum of squares -> statisticsAdjust(0, 1): avg0, stddev0 with the N / (N - 1) of computeAvgStdev,
//                        a = 1 / stddev0 (0 for a constant piece), b = 0 - a avg0; a value becomes (T)(a x + b);
//                pass 2  (double) the right-hand side of the plane fit z = pA j + pB i + pC over the adjusted values and the logical
//                        coordinates of setXmippOrigin (normalize.cpp:355-358); the inverse of the normal matrix depends on the piece
//                        side alone and comes from the host;
//                pass 3  (double) sum1, sum2 of the residual, stddevbg = sqrt(|sum2 / N - avg^2| N / (N - 1)), the factor 1.0 / stddevbg
//                        where stddevbg > 1e-6 (normalize.cpp:419-424), 1 elsewhere.
//   k_psd_rows   the value is formed on load: adjust, subtract the plane, scale, then times the taper (1 * maskY[i]) * maskX[j], one
//                rounding, as constructPieceSmoother (:143-189) builds it. Two real rows ride one complex line of xh_plan.h; an odd piece
//                has one unpaired row. Out: the half spectrum, px / 2 + 1 columns.
//   k_psd_cols   a workgroup owns PS_STRIP columns of the half spectrum for the whole batch: it transforms the strip of piece 0, then
//                piece 1, .., forms the PSD value and adds it (in double its square too) to the running sums it holds in registers, in
//                piece order; the sums are read before and written after, so they carry across launches. No atomics, and the order of
//                every sum is the piece order whatever the capacity. In stack mode it writes each piece's own PSD instead.
//                double: m = hypot(re, im) / (py px), value = m * (m * pieceDim^2) (:435-438); float: sqrt(re re + im im) of the
//                un-normalised transform (psd_estimator.cpp:112-116), added in float as `magnitudes[n] += mag` adds it.
//   k_psd_whole  avg = sum * (1 / n), std = sqrt(max(0, sum2 * (1 / n) - avg^2)) (:572-583) and the mirror of the half into the whole by
//                the index rule of half2whole (psd_estimator.h:52-73), which for a real input is what completeFourierTransform yields.
//
// statisticsAdjust is xmippCore code outside the tree: it is stated here with the N / (N - 1) deviation of computeAvgStdev, sums in
// double, a and b doubles, the result cast to the element type. least_squares_plane_fit_All_Points is outside the tree as well: stated as
// the normal equations, solved through the adjugate inverse (the test of test_geometry_main.cpp:140-166 pins its answer).
#include "xh_plan.h"
#include "xh_reduce.h"
#include "xh_volume.h"
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace {

constexpr int PS_STRIP = 4;                       // columns of the half spectrum that one workgroup of the column pass owns
constexpr int PS_MAXSIDE = 1024;
constexpr int PS_ACC = PS_STRIP * PS_MAXSIDE / 256;      // running sums one thread holds
constexpr size_t PS_LDS = 64 * 1024;
enum { PS_ADJUST = 1, PS_RAMP = 2 };
enum { PS_T_STATS = 0, PS_T_ROWS, PS_T_COLS, PS_T_FINISH, PS_NT };

struct PsPar { double a, b, pA, pB, pC, scale; };
struct PsFit { double inv[9]; };                  // inverse of the plane fit's normal matrix

// the value of pixel (i, j) of the piece at (cy, cx), as the reference has it before the transform
template <typename T>
__device__ __forceinline__ T ps_value(const float *__restrict__ mic, int X, int cy, int cx, int i, int j, const PsPar &P, int ramp,
                                      const T *__restrict__ tapY, const T *__restrict__ tapX, int py, int px)
{
    const double x = (double)mic[(size_t)(cy + i) * X + (cx + j)];
    T v = (T)(P.a * x + P.b);
    if (ramp) {
        const int li = i - py / 2, lj = j - px / 2;
        const double aux = P.pB * li + P.pC;
        double d = (double)v;
        d -= P.pA * lj + aux;
        d *= P.scale;
        v = (T)d;
    }
    const T taper = tapY[i] * tapX[j];
    return v * taper;
}

// grid (pieces). par[p] of the piece at corners[p]
__global__ void __launch_bounds__(256)
k_psd_stats(const float *__restrict__ mic, int X, const int2 *__restrict__ corners, int py, int px, int flags, PsFit fit, PsPar *__restrict__ par)
{
    __shared__ double red[3][256];
    const int p = blockIdx.x, cy = corners[p].x, cx = corners[p].y, N = py * px;
    const float *w = mic + (size_t)cy * X + cx;
    PsPar P = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    if (flags & PS_ADJUST) {
        double v[3] = {0.0, 0.0, 0.0};
        for (int n = threadIdx.x; n < N; n += 256) {
            const int i = n / px, j = n - i * px;
            const double x = (double)w[(size_t)i * X + j];
            v[0] += x;
            v[1] += x * x;
        }
        xh_tree256(red, v);
        const double avg0 = red[0][0] / N;
        double stddev0 = 0.0;
        if (N > 1) {
            stddev0 = red[1][0] / N - avg0 * avg0;
            stddev0 *= (double)N / (double)(N - 1);
            stddev0 = sqrt(fabs(stddev0));
        }
        P.a = stddev0 != 0.0 ? 1.0 / stddev0 : 0.0;
        P.b = 0.0 - P.a * avg0;
        __syncthreads();
    }
    if (flags & PS_RAMP) {
        double v[3] = {0.0, 0.0, 0.0};
        for (int n = threadIdx.x; n < N; n += 256) {
            const int i = n / px, j = n - i * px;
            const double z = P.a * (double)w[(size_t)i * X + j] + P.b;
            v[0] += (double)(j - px / 2) * z;
            v[1] += (double)(i - py / 2) * z;
            v[2] += z;
        }
        xh_tree256(red, v);
        const double b0 = red[0][0], b1 = red[1][0], b2 = red[2][0];
        P.pA = fit.inv[0] * b0 + fit.inv[1] * b1 + fit.inv[2] * b2;
        P.pB = fit.inv[3] * b0 + fit.inv[4] * b1 + fit.inv[5] * b2;
        P.pC = fit.inv[6] * b0 + fit.inv[7] * b1 + fit.inv[8] * b2;
        __syncthreads();
        v[0] = v[1] = v[2] = 0.0;
        for (int n = threadIdx.x; n < N; n += 256) {
            const int i = n / px, j = n - i * px;
            double z = P.a * (double)w[(size_t)i * X + j] + P.b;
            const double aux = P.pB * (i - py / 2) + P.pC;
            z -= P.pA * (j - px / 2) + aux;
            v[0] += z;
            v[1] += z * z;
        }
        xh_tree256(red, v);
        const double avgbg = red[0][0] / N;
        const double stddevbg = sqrt(fabs(red[1][0] / N - avgbg * avgbg) * N / (N - 1));
        if (stddevbg > 1e-6) P.scale = 1.0 / stddevbg;
    }
    if (threadIdx.x == 0) par[p] = P;
}

// grid (pixels / 256, pieces): the prepared pieces [m][py][px] (test hook)
template <typename T>
__global__ void __launch_bounds__(256)
k_psd_piece(const float *__restrict__ mic, int X, const int2 *__restrict__ corners, const PsPar *__restrict__ par, int ramp,
            const T *__restrict__ tapY, const T *__restrict__ tapX, int py, int px, T *__restrict__ out)
{
    const int p = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= py * px) return;
    const int i = n / px, j = n - i * px;
    out[(size_t)p * py * px + n] = ps_value<T>(mic, X, corners[p].x, corners[p].y, i, j, par[p], ramp, tapY, tapX, py, px);
}

// grid (row pairs / lpb, pieces), lpb lines of (1 << plan.logM) complex numbers in dynamic LDS. H [m][py][hx]
template <typename T>
__global__ void __launch_bounds__(256)
k_psd_rows(const float *__restrict__ mic, int X, const int2 *__restrict__ corners, const PsPar *__restrict__ par, int ramp,
           const T *__restrict__ tapY, const T *__restrict__ tapX, XhPlan<T> plan, int py, int px, int lpb, xh_c2<T> *__restrict__ H)
{
    extern __shared__ __align__(16) unsigned char ps_smem[];
    xh_c2<T> *s = reinterpret_cast<xh_c2<T> *>(ps_smem);
    const int M = 1 << plan.logM, hx = px / 2 + 1, npairs = (py + 1) / 2;
    const int p = blockIdx.y, pair0 = blockIdx.x * lpb, tid = threadIdx.x;
    const int cy = corners[p].x, cx = corners[p].y;
    const PsPar P = par[p];
    for (int n = tid; n < lpb * px; n += 256) {
        const int l = n / px, e = n - l * px;            // consecutive threads -> consecutive pixels of a row
        const int r0 = 2 * (pair0 + l), r1 = r0 + 1;
        xh_c2<T> v = xh_c2<T>{0, 0};
        if (pair0 + l < npairs) {
            v.x = ps_value<T>(mic, X, cy, cx, r0, e, P, ramp, tapY, tapX, py, px);
            if (r1 < py) v.y = ps_value<T>(mic, X, cy, cx, r1, e, P, ramp, tapY, tapX, py, px);
        }
        s[l * M + xh_plan_pos(plan, e)] = v;
    }
    __syncthreads();
    xh_plan_exec<T, false>(s, plan, lpb, tid, 256);
    xh_c2<T> *Hp = H + (size_t)p * py * hx;
    const T half = (T)0.5;
    for (int n = tid; n < lpb * hx; n += 256) {
        const int l = n / hx, k = n - l * hx;
        const int r0 = 2 * (pair0 + l), r1 = r0 + 1;
        if (pair0 + l >= npairs) continue;
        const xh_c2<T> a = s[l * M + k], b = s[l * M + (k ? px - k : 0)];
        Hp[(size_t)r0 * hx + k] = xh_c2<T>{(a.x + b.x) * half, (a.y - b.y) * half};
        if (r1 < py) Hp[(size_t)r1 * hx + k] = xh_c2<T>{(a.y + b.y) * half, (b.x - a.x) * half};
    }
}

template <typename T> __device__ __forceinline__ T ps_psd(xh_c2<T> z, double size, double pd2);
template <> __device__ __forceinline__ double ps_psd<double>(xh_cd z, double size, double pd2)
{
    const double m = hypot(z.x, z.y) / size;              // FFT_magnitude takes the modulus before it is squared
    return m * (m * pd2);
}
template <> __device__ __forceinline__ float ps_psd<float>(xh_cf z, double, double)
{
    return sqrtf((z.x * z.x) + (z.y * z.y));
}

// grid (strips). H [m][py][hx]; sum, sum2 [py][hx] (sum2 nullable); stack [m][py][hx] (nullable: the pieces are added)
template <typename T>
__global__ void __launch_bounds__(256)
k_psd_cols(const xh_c2<T> *__restrict__ H, XhPlan<T> plan, int py, int hx, int m, int lpb, double size, double pd2, T *__restrict__ sum,
           T *__restrict__ sum2, T *__restrict__ stack)
{
    extern __shared__ __align__(16) unsigned char ps_smem[];
    xh_c2<T> *s = reinterpret_cast<xh_c2<T> *>(ps_smem);
    const int M = 1 << plan.logM, tid = threadIdx.x;
    const int cb = blockIdx.x * PS_STRIP, nc = min(PS_STRIP, hx - cb), E = PS_STRIP * py;
    T acc[PS_ACC], acc2[PS_ACC];
#pragma unroll
    for (int q = 0; q < PS_ACC; ++q) {
        const int e = tid + 256 * q, r = e / PS_STRIP, c = e - r * PS_STRIP;
        const bool live = e < E && c < nc && !stack;
        acc[q] = live ? sum[(size_t)r * hx + cb + c] : (T)0;
        acc2[q] = live && sum2 ? sum2[(size_t)r * hx + cb + c] : (T)0;
    }
    for (int p = 0; p < m; ++p) {
        const xh_c2<T> *Hp = H + (size_t)p * py * hx;
        for (int c0 = 0; c0 < nc; c0 += lpb) {
            const int nl = min(lpb, nc - c0);
            for (int n = tid; n < lpb * py; n += 256) {
                const int r = n / lpb, l = n - r * lpb;      // consecutive threads -> consecutive columns
                s[l * M + xh_plan_pos(plan, r)] = l < nl ? Hp[(size_t)r * hx + cb + c0 + l] : xh_c2<T>{0, 0};
            }
            __syncthreads();
            xh_plan_exec<T, false>(s, plan, lpb, tid, 256);
#pragma unroll
            for (int q = 0; q < PS_ACC; ++q) {
                const int e = tid + 256 * q, r = e / PS_STRIP, c = e - r * PS_STRIP;
                if (e < E && c >= c0 && c < c0 + nl) {
                    const T v = ps_psd<T>(s[(c - c0) * M + r], size, pd2);
                    if (stack) stack[((size_t)p * py + r) * hx + cb + c] = v;
                    else {
                        acc[q] += v;
                        acc2[q] += v * v;
                    }
                }
            }
            __syncthreads();                                   // the lines are read before the next ones arrive
        }
    }
    if (stack) return;
#pragma unroll
    for (int q = 0; q < PS_ACC; ++q) {
        const int e = tid + 256 * q, r = e / PS_STRIP, c = e - r * PS_STRIP;
        if (e < E && c < nc) {
            sum[(size_t)r * hx + cb + c] = acc[q];
            if (sum2) sum2[(size_t)r * hx + cb + c] = acc2[q];
        }
    }
}

// grid (pixels / 256, images). half [n][py][hx] -> out [n][py][px] by half2whole's index rule. stats: out = avg, out2 = std from the sums
template <typename T>
__global__ void __launch_bounds__(256)
k_psd_whole(const T *__restrict__ half, const T *__restrict__ half2, int py, int px, int stats, double idiv, T *__restrict__ out, T *__restrict__ out2)
{
    const int p = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x, hx = px / 2 + 1;
    if (n >= py * px) return;
    const int y = n / px, x = n - y * px;
    const bool mirror = x >= hx;
    const int xS = mirror ? px - x : x, yS = mirror ? (y == 0 ? 0 : py - y) : y;
    const size_t src = ((size_t)p * py + yS) * hx + xS, dst = (size_t)p * py * px + n;
    if (!stats) {
        out[dst] = half[src];
        return;
    }
    double avg = (double)half[src], sd = half2 ? (double)half2[src] : 0.0;
    avg *= idiv;
    sd *= idiv;
    sd -= avg * avg;
    sd = sd < 0 ? 0.0 : sqrt(sd);
    out[dst] = (T)avg;
    if (out2) out2[dst] = (T)sd;
}

// constructPieceSmoother's factor of one axis: n entries, fractions taken against `ysize` on both axes as the reference takes them
template <typename T> void ps_taper(int n, int ysize, std::vector<T> &m)
{
    m.assign((size_t)n, (T)1);
    const T iHalfsize = (T)2 / ysize;
    const T alpha = 0.025;
    const T alpha1 = 1 - alpha;
    const T ialpha = 1.0 / alpha;
    for (int k = 0; k < n; ++k) {
        const int i = k - n / 2;
        const T fraction = std::fabs(i * iHalfsize);
        if (fraction > alpha1) m[k] = (T)(0.5 * (1 + std::cos(3.14159265358979323846 * ((fraction - 1) * ialpha + 1))));
    }
}

// xmippCore's CEIL
int ps_ceil(double x) { return x == (int)x ? (int)x : (x > 0 ? (int)(x + 1) : (int)x); }

}  // namespace

struct xh_psd {
    xh_ctx *ctx = nullptr;
    int Y = 0, X = 0, py = 0, px = 0, hx = 0, capacity = 0;
    bool dbl = false, loaded = false;
    size_t esize = 4;
    int64_t count = 0;
    PsFit fit = {};
    XhPlanBufs<float> fx, fy;
    XhPlanBufs<double> dx, dy;
    XhBuf mic, tapY, tapX, H, par, corners, sum, sum2, stack, whole;
    XhLapTimer<PS_NT> tm;
    void finish()
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    ~xh_psd() { finish(); }
};

namespace {

template <typename T> XhPlanBufs<T> &ps_plan(xh_psd *h, bool y);
template <> XhPlanBufs<float> &ps_plan<float>(xh_psd *h, bool y) { return y ? h->fy : h->fx; }
template <> XhPlanBufs<double> &ps_plan<double>(xh_psd *h, bool y) { return y ? h->dy : h->dx; }

template <typename T> int ps_create(xh_psd *h)
{
    xh_ctx *ctx = h->ctx;
    XH_TRY(xh_plan_create<T>(ctx, h->px, ps_plan<T>(h, false)));
    XH_TRY(xh_plan_create<T>(ctx, h->py, ps_plan<T>(h, true)));
    XH_CHECK((sizeof(xh_c2<T>) << ps_plan<T>(h, false).plan.logM) <= PS_LDS && (sizeof(xh_c2<T>) << ps_plan<T>(h, true).plan.logM) <= PS_LDS,
             XH_ERR_UNSUPPORTED, "xh_psd_create: a line of %d x %d does not fit the LDS", h->py, h->px);
    std::vector<T> mY, mX;
    ps_taper<T>(h->py, h->py, mY);
    ps_taper<T>(h->px, h->py, mX);
    XH_TRY(xh_buf_upload(ctx, h->tapY, mY.data(), sizeof(T) * mY.size()));
    XH_TRY(xh_buf_upload(ctx, h->tapX, mX.data(), sizeof(T) * mX.size()));
    return XH_OK;
}

// the batch's statistics: par[0 .. m) of corners[c0 .. c0 + m)
int ps_stats(xh_psd *h, int c0, int m, int flags)
{
    hipLaunchKernelGGL(k_psd_stats, dim3((unsigned)m), dim3(256), 0, h->ctx->stream, (const float *)h->mic.p, h->X, (const int2 *)h->corners.p + c0,
                       h->py, h->px, flags, h->fit, (PsPar *)h->par.p);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

int ps_check_corners(const xh_psd *h, const char *who, const int32_t *c, int n, int flags)
{
    XH_CHECK(h->loaded, XH_ERR_STATE, "%s: no micrograph (xh_psd_load comes first)", who);
    XH_CHECK((flags & ~(PS_ADJUST | PS_RAMP)) == 0, XH_ERR_ARG, "%s: flags %d", who, flags);
    XH_CHECK(!(flags & PS_RAMP) || h->dbl, XH_ERR_ARG, "%s: the ramp belongs to the double path", who);
    for (int i = 0; i < n; ++i)
        XH_CHECK(c[2 * i] >= 0 && c[2 * i] <= h->Y - h->py && c[2 * i + 1] >= 0 && c[2 * i + 1] <= h->X - h->px, XH_ERR_ARG,
                 "%s: piece %d at (%d, %d) leaves the micrograph of %d x %d", who, i, c[2 * i], c[2 * i + 1], h->Y, h->X);
    return XH_OK;
}

template <typename T> int ps_add(xh_psd *h, const int32_t *h_corners, int n, int flags, T *h_stack)
{
    xh_ctx *ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const int py = h->py, px = h->px, hx = h->hx;
    const XhPlan<T> planX = ps_plan<T>(h, false).plan, planY = ps_plan<T>(h, true).plan;
    const int lx = xh_plan_lpb(planX, PS_LDS, 16), ly = xh_plan_lpb(planY, PS_LDS, PS_STRIP);
    const size_t smx = ((size_t)lx * sizeof(xh_c2<T>)) << planX.logM, smy = ((size_t)ly * sizeof(xh_c2<T>)) << planY.logM;
    const int npairs = (py + 1) / 2, ramp = (flags & PS_RAMP) ? 1 : 0;
    const double size = (double)py * (double)px, pd2 = size;
    XH_TRY(xh_buf_reserve(ctx, h->corners, sizeof(int2) * (size_t)n));
    XH_HIP(hipMemcpyAsync(h->corners.p, h_corners, sizeof(int2) * (size_t)n, hipMemcpyHostToDevice, st));
    if (h_stack) {
        XH_TRY(xh_buf_reserve(ctx, h->stack, sizeof(T) * (size_t)h->capacity * py * hx));
        XH_TRY(xh_buf_reserve(ctx, h->whole, sizeof(T) * (size_t)std::max(2, h->capacity) * py * px));
    }
    for (int i0 = 0; i0 < n; i0 += h->capacity) {
        const int m = std::min(h->capacity, n - i0);
        const int2 *cor = (const int2 *)h->corners.p + i0;
        XH_TRY(h->tm.start());
        XH_TRY(ps_stats(h, i0, m, flags));
        XH_TRY(h->tm.lap(PS_T_STATS));
        hipLaunchKernelGGL((k_psd_rows<T>), dim3((unsigned)((npairs + lx - 1) / lx), (unsigned)m), dim3(256), smx, st, (const float *)h->mic.p, h->X, cor,
                           (const PsPar *)h->par.p, ramp, (const T *)h->tapY.p, (const T *)h->tapX.p, planX, py, px, lx, (xh_c2<T> *)h->H.p);
        XH_LAUNCH_CHECK();
        XH_TRY(h->tm.lap(PS_T_ROWS));
        hipLaunchKernelGGL((k_psd_cols<T>), dim3((unsigned)((hx + PS_STRIP - 1) / PS_STRIP)), dim3(256), smy, st, (const xh_c2<T> *)h->H.p, planY, py, hx, m, ly,
                           size, pd2, (T *)h->sum.p, (T *)h->sum2.p, h_stack ? (T *)h->stack.p : (T *)nullptr);
        XH_LAUNCH_CHECK();
        XH_TRY(h->tm.lap(PS_T_COLS));
        if (h_stack) {
            hipLaunchKernelGGL((k_psd_whole<T>), dim3((unsigned)((py * px + 255) / 256), (unsigned)m), dim3(256), 0, st, (const T *)h->stack.p, (const T *)nullptr, py,
                               px, 0, 0.0, (T *)h->whole.p, (T *)nullptr);
            XH_LAUNCH_CHECK();
            XH_TRY(h->tm.lap(PS_T_FINISH));
            XH_HIP(hipMemcpyAsync(h_stack + (size_t)i0 * py * px, h->whole.p, sizeof(T) * (size_t)m * py * px, hipMemcpyDeviceToHost, st));
        } else
            h->count += m;
    }
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

template <typename T> int ps_piece(xh_psd *h, const int32_t *h_corners, int n, int flags, T *h_out)
{
    xh_ctx *ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const int py = h->py, px = h->px;
    XH_TRY(xh_buf_reserve(ctx, h->corners, sizeof(int2) * (size_t)n));
    XH_HIP(hipMemcpyAsync(h->corners.p, h_corners, sizeof(int2) * (size_t)n, hipMemcpyHostToDevice, st));
    XH_TRY(xh_buf_reserve(ctx, h->whole, sizeof(T) * (size_t)std::max(2, h->capacity) * py * px));
    for (int i0 = 0; i0 < n; i0 += h->capacity) {
        const int m = std::min(h->capacity, n - i0);
        XH_TRY(ps_stats(h, i0, m, flags));
        hipLaunchKernelGGL((k_psd_piece<T>), dim3((unsigned)((py * px + 255) / 256), (unsigned)m), dim3(256), 0, st, (const float *)h->mic.p, h->X,
                           (const int2 *)h->corners.p + i0, (const PsPar *)h->par.p, (flags & PS_RAMP) ? 1 : 0, (const T *)h->tapY.p, (const T *)h->tapX.p, py, px,
                           (T *)h->whole.p);
        XH_LAUNCH_CHECK();
        XH_HIP(hipMemcpyAsync(h_out + (size_t)i0 * py * px, h->whole.p, sizeof(T) * (size_t)m * py * px, hipMemcpyDeviceToHost, st));
    }
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

template <typename T> int ps_result(xh_psd *h, T *h_avg, T *h_std)
{
    xh_ctx *ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const int py = h->py, px = h->px;
    const size_t PP = (size_t)py * px;
    XH_TRY(xh_buf_reserve(ctx, h->whole, sizeof(T) * (size_t)std::max(2, h->capacity) * PP));
    T *avg = (T *)h->whole.p, *sd = avg + PP;
    XH_TRY(h->tm.start());
    // the double program divides by the pieces it added (:572-583); the float one keeps the sum of the magnitudes (psd_estimator.cpp:115)
    hipLaunchKernelGGL((k_psd_whole<T>), dim3((unsigned)((PP + 255) / 256), 1u), dim3(256), 0, st, (const T *)h->sum.p, (const T *)h->sum2.p, py, px, h->dbl ? 1 : 0,
                       1.0 / (double)h->count, avg, h->dbl ? sd : (T *)nullptr);
    XH_LAUNCH_CHECK();
    XH_TRY(h->tm.lap(PS_T_FINISH));
    XH_HIP(hipMemcpyAsync(h_avg, avg, sizeof(T) * PP, hipMemcpyDeviceToHost, st));
    if (h_std && h->dbl) XH_HIP(hipMemcpyAsync(h_std, sd, sizeof(T) * PP, hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    if (h_std && !h->dbl) std::fill(h_std, h_std + PP, (T)0);
    return XH_OK;
}

}  // namespace

extern "C" {

int xh_psd_create(xh_ctx *ctx, int32_t Y, int32_t X, int32_t py, int32_t px, int32_t capacity, int32_t is_double, xh_psd **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_psd_create: null argument");
    XH_CHECK(py >= 2 && px >= 2, XH_ERR_ARG, "xh_psd_create: bad piece size %d x %d", py, px);
    XH_CHECK(py <= PS_MAXSIDE && px <= PS_MAXSIDE, XH_ERR_UNSUPPORTED, "xh_psd_create: piece sides above 1024 are not supported (%d x %d)", py, px);
    XH_CHECK(!is_double || py == px, XH_ERR_ARG, "xh_psd_create: the double path takes square pieces (%d x %d)", py, px);
    XH_CHECK(Y >= py && X >= px && (int64_t)Y * X <= ((int64_t)1 << 31) - 1, XH_ERR_ARG, "xh_psd_create: a micrograph of %d x %d for pieces of %d x %d", Y, X, py, px);
    XH_CHECK(capacity >= 1 && capacity <= 65535, XH_ERR_ARG, "xh_psd_create: capacity %d (1 .. 65535)", capacity);
    std::unique_ptr<xh_psd> h(new xh_psd);
    XH_HIP(hipSetDevice(ctx->device));
    h->ctx = ctx;
    h->Y = Y; h->X = X; h->py = py; h->px = px; h->hx = px / 2 + 1;
    h->capacity = capacity;
    h->dbl = is_double != 0;
    h->esize = h->dbl ? sizeof(double) : sizeof(float);
    if (h->dbl) XH_TRY(ps_create<double>(h.get()));
    else XH_TRY(ps_create<float>(h.get()));
    // the normal matrix of z = pA j + pB i + pC over the logical coordinates: integers, exact; its inverse through the adjugate
    {
        double sxx = 0, syy = 0, sxy = 0, sx = 0, sy = 0;
        for (int i = -(py / 2); i < py - py / 2; ++i)
            for (int j = -(px / 2); j < px - px / 2; ++j) {
                sxx += (double)j * j; syy += (double)i * i; sxy += (double)i * j; sx += j; sy += i;
            }
        const double A[9] = {sxx, sxy, sx, sxy, syy, sy, sx, sy, (double)py * px};
        double *I = h->fit.inv;
        I[0] = A[8] * A[4] - A[7] * A[5];
        I[1] = -(A[8] * A[1] - A[7] * A[2]);
        I[2] = A[5] * A[1] - A[4] * A[2];
        I[3] = -(A[8] * A[3] - A[6] * A[5]);
        I[4] = A[8] * A[0] - A[6] * A[2];
        I[5] = -(A[5] * A[0] - A[3] * A[2]);
        I[6] = A[7] * A[3] - A[6] * A[4];
        I[7] = -(A[7] * A[0] - A[6] * A[1]);
        I[8] = A[4] * A[0] - A[3] * A[1];
        const double det = A[0] * I[0] + A[3] * I[1] + A[6] * I[2];
        for (int c = 0; c < 9; ++c) I[c] /= det;
    }
    const size_t HH = (size_t)py * h->hx;
    XH_TRY(xh_buf_alloc(ctx, h->mic, sizeof(float) * (size_t)Y * X));
    XH_TRY(xh_buf_alloc(ctx, h->H, 2 * h->esize * HH * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->par, sizeof(PsPar) * capacity));
    XH_TRY(xh_buf_alloc(ctx, h->sum, h->esize * HH));
    if (h->dbl) XH_TRY(xh_buf_alloc(ctx, h->sum2, h->esize * HH));
    XH_TRY(h->tm.create(ctx));
    XH_HIP(hipMemsetAsync(h->sum.p, 0, h->esize * HH, ctx->stream));
    if (h->dbl) XH_HIP(hipMemsetAsync(h->sum2.p, 0, h->esize * HH, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    *out = h.release();
    return XH_OK;
}

int xh_psd_destroy(xh_psd *h)
{
    delete h;
    return XH_OK;
}

int xh_psd_reset(xh_psd *h)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_psd_reset: null handle");
    XH_HIP(hipSetDevice(h->ctx->device));
    const size_t HH = (size_t)h->py * h->hx;
    XH_HIP(hipMemsetAsync(h->sum.p, 0, h->esize * HH, h->ctx->stream));
    if (h->dbl) XH_HIP(hipMemsetAsync(h->sum2.p, 0, h->esize * HH, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    h->count = 0;
    return XH_OK;
}

int xh_psd_load(xh_psd *h, const float *micrograph)
{
    XH_CHECK(h && micrograph, XH_ERR_ARG, "xh_psd_load: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(h->mic.p, micrograph, sizeof(float) * (size_t)h->Y * h->X, hipMemcpyDefault, h->ctx->stream));
    XH_HIP(hipStreamSynchronize(h->ctx->stream));
    h->loaded = true;
    return XH_OK;
}

int xh_psd_add(xh_psd *h, const int32_t *h_corners, int32_t n, int32_t flags, void *h_stack)
{
    XH_CHECK(h && (n == 0 || h_corners), XH_ERR_ARG, "xh_psd_add: null argument");
    XH_CHECK(n >= 0, XH_ERR_ARG, "xh_psd_add: %d pieces", n);
    XH_TRY(ps_check_corners(h, "xh_psd_add", h_corners, n, flags));
    if (n == 0) return XH_OK;
    XH_HIP(hipSetDevice(h->ctx->device));
    return h->dbl ? ps_add<double>(h, h_corners, n, flags, (double *)h_stack) : ps_add<float>(h, h_corners, n, flags, (float *)h_stack);
}

int xh_psd_result(xh_psd *h, void *h_avg, void *h_std, int64_t *n)
{
    XH_CHECK(h && h_avg, XH_ERR_ARG, "xh_psd_result: null argument");
    XH_CHECK(h->count > 0, XH_ERR_STATE, "xh_psd_result: no piece has been added");
    XH_HIP(hipSetDevice(h->ctx->device));
    if (n) *n = h->count;
    return h->dbl ? ps_result<double>(h, (double *)h_avg, (double *)h_std) : ps_result<float>(h, (float *)h_avg, (float *)h_std);
}

int xh_psd_smoother(xh_psd *h, void *h_out)
{
    XH_CHECK(h && h_out, XH_ERR_ARG, "xh_psd_smoother: null argument");
    XH_HIP(hipSetDevice(h->ctx->device));
    // the two factors as the kernels read them; their product is formed here as the kernels form it, one rounding
    std::vector<unsigned char> y(h->esize * h->py), x(h->esize * h->px);
    XH_HIP(hipMemcpy(y.data(), h->tapY.p, y.size(), hipMemcpyDeviceToHost));
    XH_HIP(hipMemcpy(x.data(), h->tapX.p, x.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->py; ++i)
        for (int j = 0; j < h->px; ++j)
            if (h->dbl) ((double *)h_out)[(size_t)i * h->px + j] = ((const double *)y.data())[i] * ((const double *)x.data())[j];
            else ((float *)h_out)[(size_t)i * h->px + j] = ((const float *)y.data())[i] * ((const float *)x.data())[j];
    return XH_OK;
}

int xh_psd_piece(xh_psd *h, const int32_t *h_corners, int32_t n, int32_t flags, void *h_out)
{
    XH_CHECK(h && h_corners && h_out && n >= 1, XH_ERR_ARG, "xh_psd_piece: bad argument");
    XH_TRY(ps_check_corners(h, "xh_psd_piece", h_corners, n, flags));
    XH_HIP(hipSetDevice(h->ctx->device));
    return h->dbl ? ps_piece<double>(h, h_corners, n, flags, (double *)h_out) : ps_piece<float>(h, h_corners, n, flags, (float *)h_out);
}

int xh_psd_strip(void) { return PS_STRIP; }

int xh_psd_set_timing(xh_psd *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_psd_set_timing: null handle");
    h->tm.set(on != 0);
    return XH_OK;
}

int xh_psd_stage_ms(const xh_psd *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_psd_stage_ms: null argument");
    h->tm.read(h_ms);
    return XH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- host only
int xh_psd_pieces(int32_t Y, int32_t X, int32_t pieceDim, double overlap, int32_t skipBorders, int32_t mode, const int64_t *h_pos, int32_t npos,
                  int32_t *h_corners, int32_t *h_slots, int32_t capacity, int32_t *n, int32_t *div_number)
{
    XH_CHECK(n, XH_ERR_ARG, "xh_psd_pieces: null argument");
    XH_CHECK(mode >= 0 && mode <= 2, XH_ERR_ARG, "xh_psd_pieces: mode %d (0 micrograph, 1 regions, 2 particles)", mode);
    XH_CHECK(pieceDim >= 2 && pieceDim <= PS_MAXSIDE, XH_ERR_UNSUPPORTED, "xh_psd_pieces: a piece side of %d (2 .. 1024)", pieceDim);
    XH_CHECK(Y >= pieceDim && X >= pieceDim, XH_ERR_ARG, "xh_psd_pieces: the micrograph of %d x %d is smaller than a piece of %d", Y, X, pieceDim);
    XH_CHECK(std::isfinite(overlap) && overlap >= 0 && overlap < 1, XH_ERR_ARG, "xh_psd_pieces: an overlap of %g (0 <= overlap < 1)", overlap);
    XH_CHECK(skipBorders >= 0, XH_ERR_ARG, "xh_psd_pieces: skipBorders %d", skipBorders);
    XH_CHECK(mode != 2 || (npos >= 0 && (npos == 0 || h_pos)), XH_ERR_ARG, "xh_psd_pieces: particles mode without positions");
    // :310-327
    int64_t div_Number = 0;
    int div_NumberX = 1, div_NumberY = 1;
    if (mode == 2) div_Number = npos;
    else if (mode == 0) {
        div_NumberX = ps_ceil((double)X / (pieceDim * (1 - overlap))) - 1;
        div_NumberY = ps_ceil((double)Y / (pieceDim * (1 - overlap))) - 1;
        div_Number = (int64_t)div_NumberX * div_NumberY;
    } else {
        div_NumberX = ps_ceil((double)X / pieceDim);
        div_NumberY = ps_ceil((double)Y / pieceDim);
        XH_CHECK(!(div_NumberX <= 2 * skipBorders || div_NumberY <= 2 * skipBorders), XH_ERR_ARG,
                 "xh_psd_pieces: The micrograph is not big enough to skip %d pieces on each side", skipBorders);
        div_Number = (int64_t)div_NumberX * div_NumberY;
    }
    XH_CHECK(div_Number <= (1 << 26), XH_ERR_ARG, "xh_psd_pieces: %lld pieces", (long long)div_Number);
    int count = 0;
    for (int64_t N = 1; N <= div_Number; ++N) {
        bool skip = false;
        int64_t piecei, piecej;
        if (mode == 2) {
            // :381-393: the reference subtracts in unsigned arithmetic and its `< 0` tests never hold
            piecej = h_pos[2 * (N - 1)];
            piecei = h_pos[2 * (N - 1) + 1];
            XH_CHECK(piecej >= pieceDim / 2 && piecei >= pieceDim / 2, XH_ERR_ARG,
                     "xh_psd_pieces: particle %lld at (x %lld, y %lld) is nearer than pieceDim / 2 = %d to the left or top edge, where the reference's unsigned subtraction wraps",
                     (long long)N, (long long)piecej, (long long)piecei, pieceDim / 2);
            piecej -= pieceDim / 2;
            piecei -= pieceDim / 2;
        } else {
            int step = pieceDim;
            if (mode == 0) step = (int)((1 - overlap) * step);
            const int blocki = (int)((N - 1) / div_NumberX), blockj = (int)((N - 1) % div_NumberX);
            if (blocki < skipBorders || blockj < skipBorders || blocki > (div_NumberY - skipBorders - 1) || blockj > (div_NumberX - skipBorders - 1)) skip = true;
            piecei = (int64_t)blocki * step;
            piecej = (int64_t)blockj * step;
        }
        if (piecei + pieceDim > Y) piecei = Y - pieceDim;
        if (piecej + pieceDim > X) piecej = X - pieceDim;
        if (skip) continue;
        if (h_corners && h_slots) {
            XH_CHECK(count < capacity, XH_ERR_ARG, "xh_psd_pieces: more pieces than the capacity of %d", capacity);
            h_corners[2 * count] = (int32_t)piecei;
            h_corners[2 * count + 1] = (int32_t)piecej;
            h_slots[count] = (int32_t)N;
        }
        ++count;
    }
    XH_CHECK(count > 0, XH_ERR_ARG, "xh_psd_pieces: no piece is left (%d x %d divisions, skipBorders %d), where the reference divides by zero",
             mode == 2 ? (int)div_Number : div_NumberX, mode == 2 ? 1 : div_NumberY, skipBorders);
    *n = count;
    if (div_number) *div_number = (int32_t)div_Number;
    return XH_OK;
}

int xh_psd_patches(int32_t Y, int32_t X, int32_t py, int32_t px, int32_t borderX, int32_t borderY, float overlap, int32_t *h_corners, int32_t capacity, int32_t *n)
{
    XH_CHECK(n, XH_ERR_ARG, "xh_psd_patches: null argument");
    XH_CHECK(px >= 1 && py >= 1 && borderX >= 0 && borderY >= 0, XH_ERR_ARG, "xh_psd_patches: bad patch or border");
    XH_CHECK(X >= px && Y >= py, XH_ERR_ARG, "xh_psd_patches: the patch of %d x %d is larger than the micrograph of %d x %d", py, px, Y, X);
    XH_CHECK((int64_t)2 * borderX + px <= X && (int64_t)2 * borderY + py <= Y, XH_ERR_ARG, "xh_psd_patches: the borders leave no room for a patch");
    XH_CHECK(overlap >= 0.f && overlap < 1.f, XH_ERR_ARG, "xh_psd_patches: an overlap of %g (0 <= overlap < 1)", (double)overlap);
    // getPatchesLocation, psd_estimator.cpp:35-71
    const size_t stepX = (size_t)std::max((1 - overlap) * px, 1.f), stepY = (size_t)std::max((1 - overlap) * py, 1.f);
    const size_t maxX = (size_t)X - borderX - px, maxY = (size_t)Y - borderY - py;
    int count = 0;
    for (size_t y = (size_t)borderY; y < maxY + stepY; y += stepY) {
        const size_t ys = std::min(y, maxY);
        for (size_t x = (size_t)borderX; x < maxX + stepX; x += stepX) {
            const size_t xs = std::min(x, maxX);
            if (h_corners) {
                XH_CHECK(count < capacity, XH_ERR_ARG, "xh_psd_patches: more patches than the capacity of %d", capacity);
                h_corners[2 * count] = (int32_t)ys;
                h_corners[2 * count + 1] = (int32_t)xs;
            }
            ++count;
        }
    }
    *n = count;
    return XH_OK;
}

}  // extern "C"
