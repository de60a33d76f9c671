// xh_ldb.hip -- the device side of xmipp_volume_local_sharpening, LocalDeblur (reconstruction/volume_local_sharpening.{h,cpp},
// ProgLocSharpening; the reference has no GPU version), fp64. It consumes the local resolution map of xmipp_resolution_monogenic_signal.
//
// The handle owns every buffer of a Z x Y x X volume, the plans and the spectra of a batch of resolution bands. The operator L
// (localfiltering :219-283) of a volume is
//   forward    r2c of the volume, 1 / N in the row kernel (the reference's forward transform carries the 1 / N);
//   split      one kernel reads the spectrum once and writes the band-passed spectra of the batch's bands (bandPassFilterFunction
//              :181-217: w_inf <= un <= wL kept, times the raised cosine; un comes from the index). Band b is zero where un > wL_b, so only
//              the columns j < jcount_b of its spectrum are written (values or zeros); nothing reads the others;
//   y, z       the line passes of the batch's inverse transforms, one launch per pass: the launch enumerates only the lines of each band
//              that can hold a non-zero element, from the per-band table (kmax, kcount, jcount). A y line (k, j) is all zeros unless
//              |uz| <= wL and ux <= wL, a z line (i, j) unless ux <= wL; the transform of a zero line is a zero line, so no value changes.
//              The table is conservative: one index beyond floor(wL size) on each axis;
//   rows       the x lines of the whole batch: the Hermitian lines of two bands are one complex line in LDS (A + i B gives a + i b); the
//              imaginary parts of the DC and Nyquist elements are dropped first, as FFTW's c2r does. Elements j >= jcount_b are taken as
//              zero without a read. The row of the resolution map is read once; per band, filtered times exp(-K (res - resVol)^2) is
//              added to the running sum strictly in band order, product and sum rounded separately; the accumulator is touched once
//              per batch. The filtered volumes never exist in memory;
//   finishing  the division by lastweight where it is > 0, fused with Vorig - op and the partial sums of |op|^2 (first operator of an
//              iteration) or with Vk + lambda filtered and the floor (second operator).
// lastweight depends on the map and the band list alone: it is computed once per load, the bands added in band order. The weights
// themselves are recomputed where they are used.
// Bands 2m and 2m + 1 of the band list are always partners in a complex line, whatever the batch: a batch holds an even number of
// spectra (the constructor's `batch` rounded up), so every batch size gives the same bytes.
// run (:285-407): the host reads one small record per iteration (the two sums of squares) while the second operator already runs, and
// takes the stop and lambda decisions as :345-364 and :391-397 do. Sums use the fixed-order reduction (xh_reduce.h).
//
// Reference behaviours kept as written:
//  - maxRes is taken before the clamp, over every voxel, starting from 1e-38 (:112, :132-149);
//  - res advances by repeated addition of 0.2 (:231);
//  - the band de-duplication uses the Z size (:235);
//  - both branches of the filter use the same expression (:197-205): the band is w_inf <= un <= wL;
//  - 1e-38 at the origin (:98), so DC enters a band when w_inf <= 0;
//  - the floor at -4 desvOutside, desvOutside = 0 included (:381);
//  - lambda == 1 is the "estimate it" switch (:360);
//  - -n (the threads of the reference's transforms) is accepted by the program and unused;
//  - the output is written whether or not the stop rule fired (:403-405).
// Refused, each where the reference divides by zero or reads what it never wrote:
//  - a sampling rate with 2 sampling - 0.2 <= 0 (wL of the first band);
//  - a resolution map with no voxel >= 2 sampling (norm = 0, porc = 0 / 0), or with a maximum that is not finite;
//  - Niter < 1 (the sharpened map is never assigned).
#include "xh_volume.h"
#include "xh_reduce.h"
#include <cmath>
#include <cstring>

namespace {

// one resolution band: the filter's constants and the table of the lines that can be non-zero
struct LdbBand {
    double res, w, wL, w_inf, ideltal;
    int kmax, kcount, jcount, idx;
};

constexpr int LDB_EPT = 4;             // rows kernel: output elements per thread (rpb X <= 256 LDB_EPT)
constexpr int LDB_MAX_LPB = 8;
constexpr double LDB_STEP = 0.2;
enum { LDB_T_FORWARD = 0, LDB_T_SPLIT, LDB_T_YZ, LDB_T_ROWS, LDB_T_FINISH, LDB_NT };

// produceSideInfo :81-102: sqrt((uz^2 + uy^2) + ux^2), 1e-38 at the origin
__device__ __forceinline__ double ldb_un(int k, int i, int j, XhDims d)
{
    if (k == 0 && i == 0 && j == 0) return 1e-38;
    const double uz = d_digfreq(k, d.Z), uy = d_digfreq(i, d.Y), ux = d_digfreq(j, d.X);
    const double uz2 = uz * uz;
    const double uz2y2 = uz2 + uy * uy;
    const double u2 = uz2y2 + ux * ux;
    return sqrt(u2);
}

// localfiltering :256
__device__ __forceinline__ double ldb_weight(double K, double res, double res_map) { return exp(-K * (res - res_map) * (res - res_map)); }

// ---------------------------------------------------------------- side info
// maxMinResolution (:132-149) before the clamp, the clamp (:115-123), and N, sum, sum2 of vol over resVol < 2 sampling (:151-171).
// The maximum starts from 1e-38, so only positive values compete: their bits order as they do, and an integer maximum has no order
__global__ void __launch_bounds__(256)
k_ldb_side(double *__restrict__ res, const double *__restrict__ vol, size_t N, double twoS, unsigned long long *__restrict__ maxbits, double *__restrict__ partials)
{
    double acc[3] = {0, 0, 0};
    unsigned long long mx = 0;
    XH_GRID_LOOP(n, N) {
        double r = res[n];
        if (r > 1e-38) mx = max(mx, (unsigned long long)__double_as_longlong(r));
        if (r < twoS && r > 0) {
            r = twoS;
            res[n] = r;
        }
        if (r < twoS) {
            const double v = vol[n];
            acc[0] += 1; acc[1] += v; acc[2] += v * v;
        }
    }
    if (mx) atomicMax(maxbits, mx);
    xh_block_partials(acc, partials);
}

// lastweight (:263): the weights of every band added in band order; 0 where resVol < 2 sampling (the weight is never touched there)
__global__ void __launch_bounds__(256)
k_ldb_lastweight(const double *__restrict__ res, double *__restrict__ lw, size_t N, const LdbBand *__restrict__ bands, int nbands, double twoS, double K)
{
    XH_GRID_LOOP(n, N) {
        const double r = res[n];
        double s = 0;
        if (!(r < twoS))
            for (int b = 0; b < nbands; ++b) s += ldb_weight(K, bands[b].res, r);
        lw[n] = s;
    }
}

// ---------------------------------------------------------------- one batch of bands
// bandPassFilterFunction :189-206 for the bands b0 .. b0 + nb - 1: F -> FB[s], columns j < jcount only
__global__ void __launch_bounds__(256)
k_ldb_split(const xh_cd *__restrict__ F, xh_cd *__restrict__ FB, size_t NF, XhDims d, const LdbBand *__restrict__ bands, int b0, int nb)
{
    XH_GRID_LOOP(e, NF) {
        int k, i, j;
        xh_kij(e, d, k, i, j);
        const double un = ldb_un(k, i, j, d);
        xh_cd f = xh_cd{0.0, 0.0};
        bool have = false;
        for (int s = 0; s < nb; ++s) {
            const LdbBand &B = bands[b0 + s];
            if (j >= B.jcount) continue;
            xh_cd o = xh_cd{0.0, 0.0};
            if (B.w_inf <= un && un <= B.wL) {
                if (!have) { f = F[e]; have = true; }
                const double H = 0.5 * (1 + cos((un - B.w) * B.ideltal));
                o = xh_cd{f.x * H, f.y * H};
            }
            FB[(size_t)s * NF + e] = o;
        }
    }
}

// the y (PASS 0) or z (PASS 1) lines of the batch's inverse transforms, in place, un-normalised: only the lines of the per-band table.
// Line l of band s: PASS 0 (a, j) with a < kcount standing for k = a (a <= kmax) or Z - (kcount - a); PASS 1 (i, j); j < jcount
template <int PASS>
__global__ void __launch_bounds__(256)
k_ldb_lines(xh_cd *__restrict__ FB, XhPlan<double> plan, const LdbBand *__restrict__ bands, int b0, int nb, XhDims d, size_t NF, int lpb)
{
    extern __shared__ __align__(16) unsigned char ldb_lines_smem[];
    __shared__ long long base[LDB_MAX_LPB];
    xh_cd *s = reinterpret_cast<xh_cd *>(ldb_lines_smem);
    const int n = plan.n, M = 1 << plan.logM;
    const int tid = threadIdx.x, nth = blockDim.x;
    if (tid < lpb) {
        size_t l = (size_t)blockIdx.x * lpb + tid;
        long long bs = -1;
        for (int b = 0; b < nb; ++b) {
            const LdbBand &B = bands[b0 + b];
            const size_t cnt = (size_t)(PASS == 0 ? B.kcount : d.Y) * B.jcount;
            if (l < cnt) {
                const int a = (int)(l / B.jcount), j = (int)(l - (size_t)a * B.jcount);
                if (PASS == 0) {
                    const int k = a <= B.kmax ? a : d.Z - (B.kcount - a);
                    bs = (long long)((size_t)b * NF + (size_t)k * d.Y * d.xh + j);
                } else bs = (long long)((size_t)b * NF + (size_t)a * d.xh + j);
                break;
            }
            l -= cnt;
        }
        base[tid] = bs;
    }
    __syncthreads();
    const size_t stride = PASS == 0 ? (size_t)d.xh : (size_t)d.Y * d.xh;
    for (int i = tid; i < lpb * n; i += nth) {
        const int e = i / lpb, l = i - e * lpb;  // consecutive threads -> consecutive lines
        xh_cd v = xh_cd{0.0, 0.0};
        if (base[l] >= 0) v = FB[(size_t)base[l] + (size_t)e * stride];
        s[l * M + xh_plan_pos(plan, e)] = v;
    }
    __syncthreads();
    xh_plan_exec<double, true>(s, plan, lpb, tid, nth);
    for (int i = tid; i < lpb * n; i += nth) {
        const int e = i / lpb, l = i - e * lpb;
        if (base[l] >= 0) FB[(size_t)base[l] + (size_t)e * stride] = s[l * M + e];
    }
}

// the x lines of the batch and the weighted accumulation (:246-262). rpb rows per workgroup (rpb X <= 256 LDB_EPT); the pairs of the
// batch go through LDS ppc at a time, rpb ppc complex lines of M elements
__global__ void __launch_bounds__(256)
k_ldb_rows(const xh_cd *__restrict__ FB, const double *__restrict__ res, double *__restrict__ acc, const LdbBand *__restrict__ bands, XhPlan<double> plan,
           size_t nrows, size_t NF, int X, int xh, int rpb, int ppc, int b0, int nb, int first, double twoS, double K)
{
    extern __shared__ __align__(16) unsigned char ldb_rows_smem[];
    xh_cd *s = reinterpret_cast<xh_cd *>(ldb_rows_smem);
    const int M = 1 << plan.logM;
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * rpb;
    const int nr = (int)min((size_t)rpb, nrows - row0);
    const int nout = nr * X;
    double rv[LDB_EPT], a[LDB_EPT];
#pragma unroll
    for (int u = 0; u < LDB_EPT; ++u) {
        const int q = tid + u * 256;
        rv[u] = 0.0;
        a[u] = 0.0;
        if (q < nout) {
            rv[u] = res[row0 * X + q];
            if (!first) a[u] = acc[row0 * X + q];
        }
    }
    const int npairs = (nb + 1) >> 1;
    for (int p0 = 0; p0 < npairs; p0 += ppc) {
        const int pc = min(ppc, npairs - p0);
        for (int q = tid; q < rpb * pc * X; q += 256) {
            const int l = q / X, e = q - l * X, r = l / pc, pp = l - r * pc;
            xh_cd v = xh_cd{0.0, 0.0};
            if (r < nr) {
                const int src = e < xh ? e : X - e;
                const int sA = 2 * (p0 + pp), sB = sA + 1;
                const size_t at = (row0 + r) * xh + src;
                xh_cd A = xh_cd{0.0, 0.0}, B = xh_cd{0.0, 0.0};
                if (src < bands[b0 + sA].jcount) A = FB[(size_t)sA * NF + at];
                if (sB < nb && src < bands[b0 + sB].jcount) B = FB[(size_t)sB * NF + at];
                if (src == 0 || 2 * src == X) { A.y = 0.0; B.y = 0.0; }
                if (e >= xh) { A.y = -A.y; B.y = -B.y; }
                v = xh_cd{A.x - B.y, A.y + B.x};
            }
            s[l * M + xh_plan_pos(plan, e)] = v;
        }
        __syncthreads();
        xh_plan_exec<double, true>(s, plan, rpb * pc, tid, 256);
#pragma unroll
        for (int u = 0; u < LDB_EPT; ++u) {
            const int q = tid + u * 256;
            if (q < nout && !(rv[u] < twoS)) {
                const int r = q / X, e = q - r * X;
                for (int pp = 0; pp < pc; ++pp) {
                    const xh_cd c = s[(r * pc + pp) * M + e];
                    const int sA = 2 * (p0 + pp);
                    const double fa = c.x * ldb_weight(K, bands[b0 + sA].res, rv[u]);
                    a[u] += fa;
                    if (sA + 1 < nb) {
                        const double fb = c.y * ldb_weight(K, bands[b0 + sA + 1].res, rv[u]);
                        a[u] += fb;
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < LDB_EPT; ++u) {
        const int q = tid + u * 256;
        if (q < nout) acc[row0 * X + q] = a[u];
    }
}

// ---------------------------------------------------------------- finishing
// :270-274
__device__ __forceinline__ double ldb_div(double v, double lw) { return lw > 0 ? v / lw : v; }

__global__ void __launch_bounds__(256) k_ldb_divide(const double *__restrict__ acc, const double *__restrict__ lw, double *__restrict__ out, size_t N)
{
    XH_GRID_LOOP(n, N) out[n] = ldb_div(acc[n], lw[n]);
}

// the first operator of an iteration (:320-341): op = acc / lastweight, filt = Vorig - op, partial sums of op^2 and Vorig^2
__global__ void __launch_bounds__(256)
k_ldb_first(const double *__restrict__ acc, const double *__restrict__ lw, const double *__restrict__ vorig, double *__restrict__ filt, size_t N,
            double *__restrict__ partials)
{
    double s[2] = {0, 0};
    XH_GRID_LOOP(n, N) {
        const double op = ldb_div(acc[n], lw[n]), v = vorig[n];
        filt[n] = v - op;
        s[0] += op * op;
        s[1] += v * v;
    }
    xh_block_partials(s, partials);
}

// the second operator (:375-383): sharp = Vk + lambda (acc / lastweight), floored. Vk is sharp itself after the first iteration
__global__ void __launch_bounds__(256)
k_ldb_second(const double *__restrict__ acc, const double *__restrict__ lw, const double *vk, double *sharp, size_t N, double lambda, double floorv)
{
    XH_GRID_LOOP(n, N) {
        const double f = ldb_div(acc[n], lw[n]);
        const double t = lambda * f;
        double v = vk[n] + t;
        if (v < floorv) v = floorv;
        sharp[n] = v;
    }
}

double ldb_round_idx(double x) { return x > 0 ? (double)(int)(x + 0.5) : (double)(int)(x - 0.5); }

// DIGFREQ2FFT_IDX (xmippCore xmipp_fft.h)
int ldb_freq2idx(double freq, int size)
{
    int idx = (int)ldb_round_idx((double)size * freq);
    if (idx < 0) idx += size;
    return idx;
}

// the loop of localfiltering (:231-244, :264-265) without the transforms
int ldb_band_list(int zsize, double sampling, double maxRes, std::vector<LdbBand> &out)
{
    out.clear();
    const double minRes = 2 * sampling, step = LDB_STEP;
    XH_CHECK(sampling > 0 && minRes - step > 0, XH_ERR_ARG, "local sharpening: a sampling rate of %g makes the first band's wL = sampling / (2 sampling - 0.2) undefined",
             sampling);
    XH_CHECK(std::isfinite(maxRes), XH_ERR_ARG, "local sharpening: the largest resolution %g is not finite", maxRes);
    int lastidx = -1;
    for (double res = minRes; res < maxRes; res += step) {
        const double freq = sampling / res;
        const int idx = ldb_freq2idx(freq, zsize);
        if (idx == lastidx) continue;
        LdbBand b;
        std::memset(&b, 0, sizeof(b));
        b.res = res;
        b.w = freq;
        b.wL = sampling / (res - step);
        const double delta = b.wL - b.w;
        b.w_inf = b.w - delta;
        b.ideltal = 3.14159265358979323846 / delta;
        b.idx = idx;
        out.push_back(b);
        lastidx = idx;
    }
    return XH_OK;
}

// the lines of a band that can hold an element with un <= wL: one index beyond floor(wL size) on each axis
void ldb_band_table(LdbBand &b, int Z, int X, int xh)
{
    const double kz = std::floor(b.wL * Z) + 1, jx = std::floor(b.wL * X) + 1;
    b.kmax = (int)std::min<double>(Z / 2, kz);
    b.kcount = std::min(Z, 2 * b.kmax + 1);
    b.jcount = (int)std::min<double>(xh, jx + 1);
}

}  // namespace

struct xh_ldb : XhVolume {
    unsigned grid = 0;
    int nbuf = 2, rpb = 1, ppc = 1;
    XhBuf F, FB, Vorig, res, lw, acc, filt, sharp, bands, partials, result, maxbits;
    XhPinned host;
    XhLapTimer<LDB_NT> tm;
    XhEvent evRec;
    bool loaded = false;
    std::vector<LdbBand> list;
    double sampling = 1, K = 0.025, maxRes = 0, desvOutside = 0;
    int64_t noutside = 0;
    ~xh_ldb() { finish(); }
};

namespace {

const LdbBand *bp(xh_ldb *h) { return (const LdbBand *)h->bands.p; }

// L without its division: the weighted band sum of d_in into h->acc
int ldb_filter(xh_ldb *h, const double *d_in)
{
    hipStream_t st = h->ctx->stream;
    const XhDims d = h->d;
    const int nbands = (int)h->list.size();
    XH_TRY(h->tm.start());
    XH_TRY(h->fft.r2c(d_in, cp(h->F), 1.0 / (double)h->N));
    XH_TRY(h->tm.lap(LDB_T_FORWARD));
    const XhPlan<double> &py = h->fft.py.plan, &pz = h->fft.pz.plan, &px = h->fft.px.plan;
    const int lpy = xh_plan_lpb(py, 64 * 1024, LDB_MAX_LPB), lpz = xh_plan_lpb(pz, 64 * 1024, LDB_MAX_LPB);
    for (int b0 = 0; b0 < nbands; b0 += h->nbuf) {
        const int nb = std::min(h->nbuf, nbands - b0);
        XH_LAUNCH256(h->ctx, k_ldb_split, h->grid, (const xh_cd *)h->F.p, cp(h->FB), h->NF, d, bp(h), b0, nb);
        XH_TRY(h->tm.lap(LDB_T_SPLIT));
        size_t ny = 0, nz = 0;
        for (int b = b0; b < b0 + nb; ++b) {
            ny += (size_t)h->list[b].kcount * h->list[b].jcount;
            nz += (size_t)d.Y * h->list[b].jcount;
        }
        hipLaunchKernelGGL(k_ldb_lines<0>, dim3((unsigned)((ny + lpy - 1) / lpy)), dim3(256), ((size_t)lpy * sizeof(xh_cd)) << py.logM, st, cp(h->FB), py, bp(h), b0, nb, d,
                           h->NF, lpy);
        XH_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_ldb_lines<1>, dim3((unsigned)((nz + lpz - 1) / lpz)), dim3(256), ((size_t)lpz * sizeof(xh_cd)) << pz.logM, st, cp(h->FB), pz, bp(h), b0, nb, d,
                           h->NF, lpz);
        XH_LAUNCH_CHECK();
        XH_TRY(h->tm.lap(LDB_T_YZ));
        const size_t nrows = (size_t)d.Z * d.Y;
        const size_t smem = ((size_t)h->rpb * h->ppc * sizeof(xh_cd)) << px.logM;
        hipLaunchKernelGGL(k_ldb_rows, dim3((unsigned)((nrows + h->rpb - 1) / h->rpb)), dim3(256), smem, st, (const xh_cd *)h->FB.p, (const double *)h->res.p, dp(h->acc),
                           bp(h), px, nrows, h->NF, d.X, d.xh, h->rpb, h->ppc, b0, nb, b0 == 0 ? 1 : 0, 2 * h->sampling, h->K);
        XH_LAUNCH_CHECK();
        XH_TRY(h->tm.lap(LDB_T_ROWS));
    }
    return XH_OK;
}

}  // namespace

extern "C" {

int xh_ldb_bands(int32_t zsize, double sampling, double max_res, double *h_bands, int32_t cap, int32_t *n)
{
    XH_CHECK(n && zsize >= 1 && cap >= 0 && (h_bands || cap == 0), XH_ERR_ARG, "xh_ldb_bands: bad argument");
    std::vector<LdbBand> list;
    XH_TRY(ldb_band_list(zsize, sampling, max_res, list));
    *n = (int32_t)list.size();
    for (int b = 0; b < std::min<int>(cap, *n); ++b) {
        h_bands[4 * b] = list[b].res; h_bands[4 * b + 1] = list[b].w; h_bands[4 * b + 2] = list[b].wL; h_bands[4 * b + 3] = list[b].idx;
    }
    return XH_OK;
}

int xh_ldb_create(xh_ctx *ctx, int32_t Z, int32_t Y, int32_t X, int32_t batch, xh_ldb **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_ldb_create: null argument");
    XH_CHECK(Z >= 2 && Y >= 2 && X >= 2, XH_ERR_ARG, "xh_ldb_create: bad size %d x %d x %d", Z, Y, X);
    XH_CHECK(Z <= 1024 && Y <= 1024 && X <= 1024, XH_ERR_UNSUPPORTED, "xh_ldb_create: sizes above 1024 are not supported (%d x %d x %d)", Z, Y, X);
    XH_CHECK(batch >= 1 && batch <= 64, XH_ERR_ARG, "xh_ldb_create: a batch of %d bands (1 .. 64)", batch);
    std::unique_ptr<xh_ldb> h(new xh_ldb);
    XH_TRY(h->init(ctx, Z, Y, X));
    h->grid = xh_grid256(h->NF, ctx->num_cus, 4);
    h->nbuf = (batch + 1) & ~1;
    const size_t lineBytes = sizeof(xh_cd) << h->fft.px.plan.logM;
    XH_CHECK(lineBytes <= 64 * 1024, XH_ERR_UNSUPPORTED, "xh_ldb_create: a row of %d points does not fit the LDS of the row kernel", X);
    h->rpb = std::max(1, std::min(8, 256 * LDB_EPT / X));
    h->ppc = (int)std::max<size_t>(1, std::min<size_t>((size_t)h->nbuf / 2, 32 * 1024 / (lineBytes * h->rpb)));
    XH_CHECK((size_t)h->rpb * h->ppc * lineBytes <= 64 * 1024 && h->rpb * X <= 256 * LDB_EPT, XH_ERR_UNSUPPORTED, "xh_ldb_create: the row kernel's tile does not fit (%d)", X);
    const size_t vb = sizeof(double) * h->N, fb = sizeof(xh_cd) * h->NF;
    for (XhBuf *b : {&h->Vorig, &h->res, &h->lw, &h->acc, &h->filt, &h->sharp}) XH_TRY(xh_buf_alloc(ctx, *b, vb));
    XH_TRY(xh_buf_alloc(ctx, h->F, fb));
    XH_TRY(xh_buf_alloc(ctx, h->FB, (size_t)h->nbuf * fb));
    XH_TRY(xh_buf_alloc(ctx, h->partials, sizeof(double) * 3 * h->grid));
    XH_TRY(xh_buf_alloc(ctx, h->result, sizeof(double) * 4));
    XH_TRY(xh_buf_alloc(ctx, h->maxbits, sizeof(unsigned long long)));
    XH_TRY(xh_pinned_alloc(ctx, h->host, sizeof(double) * 8));
    XH_TRY(h->tm.create(ctx));
    XH_TRY(xh_event_create(h->evRec, false));
    *out = h.release();
    return XH_OK;
}

int xh_ldb_destroy(xh_ldb *h)
{
    delete h;
    return XH_OK;
}

int xh_ldb_load(xh_ldb *h, const double *d_vol, const double *d_res, double sampling, double K)
{
    XH_CHECK(h && d_vol && d_res, XH_ERR_ARG, "xh_ldb_load: null argument");
    XH_CHECK(sampling > 0 && 2 * sampling - LDB_STEP > 0, XH_ERR_ARG,
             "xh_ldb_load: a sampling rate of %g makes the first band's wL = sampling / (2 sampling - 0.2) undefined", sampling);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    h->loaded = false;
    h->sampling = sampling;
    h->K = K;
    XH_HIP(hipMemcpyAsync(h->Vorig.p, d_vol, h->Vorig.bytes, hipMemcpyDeviceToDevice, st));
    XH_HIP(hipMemcpyAsync(h->res.p, d_res, h->res.bytes, hipMemcpyDeviceToDevice, st));
    // produceSideInfo :112-127
    const double floorMax = 1e-38;
    unsigned long long *hb = (unsigned long long *)(h->host.f64() + 4);
    std::memcpy(hb, &floorMax, sizeof(double));
    XH_HIP(hipMemcpyAsync(h->maxbits.p, hb, sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    XH_LAUNCH256(h->ctx, k_ldb_side, h->grid, dp(h->res), (const double *)h->Vorig.p, h->N, 2 * sampling, (unsigned long long *)h->maxbits.p, dp(h->partials));
    XH_LAUNCH256(h->ctx, xh_k_reduce_final, 1, (const double *)h->partials.p, (int)h->grid, 3, dp(h->result));
    double *hp = h->host.f64();
    XH_HIP(hipMemcpyAsync(hp, h->result.p, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
    XH_HIP(hipMemcpyAsync(hp + 5, h->maxbits.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    XH_HIP(hipStreamSynchronize(st));
    std::memcpy(&h->maxRes, hp + 5, sizeof(double));
    {   // computeAvgStdev_within_binary_mask :173-178
        const double Nd = hp[0], sum1 = hp[1], sum2 = hp[2];
        h->noutside = (int64_t)Nd;
        const double avg = sum1 / Nd;
        h->desvOutside = Nd > 1 ? std::sqrt(std::fabs(sum2 / Nd - avg * avg) * Nd / (Nd - 1)) : 0.0;
    }
    XH_CHECK((size_t)h->noutside < h->N, XH_ERR_ARG, "xh_ldb_load: the resolution map has no voxel at or above 2 sampling = %g", 2 * sampling);
    // run :297-298
    XH_TRY(ldb_band_list(h->d.Z, sampling, h->maxRes + 2, h->list));
    XH_CHECK(!h->list.empty(), XH_ERR_ARG, "xh_ldb_load: no resolution band between %g and %g", 2 * sampling, h->maxRes + 2);
    for (LdbBand &b : h->list) ldb_band_table(b, h->d.Z, h->d.X, h->d.xh);
    XH_TRY(xh_buf_reserve(h->ctx, h->bands, sizeof(LdbBand) * h->list.size()));
    XH_HIP(hipMemcpy(h->bands.p, h->list.data(), sizeof(LdbBand) * h->list.size(), hipMemcpyHostToDevice));
    XH_LAUNCH256(h->ctx, k_ldb_lastweight, h->grid, (const double *)h->res.p, dp(h->lw), h->N, bp(h), (int)h->list.size(), 2 * sampling, K);
    XH_HIP(hipStreamSynchronize(st));
    h->loaded = true;
    return XH_OK;
}

int xh_ldb_info(const xh_ldb *h, double *maxRes, double *desvOutside, int64_t *noutside, int32_t *nbands, double *h_bands, int32_t cap)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_ldb_info: null handle");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_ldb_info: nothing is loaded");
    XH_CHECK(cap >= 0 && (h_bands || cap == 0), XH_ERR_ARG, "xh_ldb_info: bad capacity");
    if (maxRes) *maxRes = h->maxRes;
    if (desvOutside) *desvOutside = h->desvOutside;
    if (noutside) *noutside = h->noutside;
    if (nbands) *nbands = (int32_t)h->list.size();
    for (int b = 0; b < std::min<int>(cap, (int)h->list.size()); ++b) {
        const LdbBand &B = h->list[b];
        double *o = h_bands + 6 * b;
        o[0] = B.res; o[1] = B.w; o[2] = B.wL; o[3] = B.idx; o[4] = B.kcount; o[5] = B.jcount;
    }
    return XH_OK;
}

int xh_ldb_resmap(xh_ldb *h, double *d_out)
{
    XH_CHECK(h && d_out, XH_ERR_ARG, "xh_ldb_resmap: null argument");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_ldb_resmap: nothing is loaded");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_HIP(hipMemcpyAsync(d_out, h->res.p, h->res.bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
    return XH_OK;
}

int xh_ldb_localfilter(xh_ldb *h, const double *d_in, double *d_out)
{
    XH_CHECK(h && d_in && d_out, XH_ERR_ARG, "xh_ldb_localfilter: null argument");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_ldb_localfilter: nothing is loaded");
    XH_HIP(hipSetDevice(h->ctx->device));
    XH_TRY(ldb_filter(h, d_in));
    XH_LAUNCH256(h->ctx, k_ldb_divide, h->grid, (const double *)h->acc.p, (const double *)h->lw.p, d_out, h->N);
    XH_TRY(h->tm.lap(LDB_T_FINISH));
    return XH_OK;
}

int xh_ldb_run(xh_ldb *h, double lambda, int32_t niter, xh_ldb_iter *h_iters, int32_t max_iters, int32_t *n_iters, int32_t *stopped, double *lambda_out,
               double *d_out)
{
    XH_CHECK(h && n_iters && stopped && lambda_out && d_out, XH_ERR_ARG, "xh_ldb_run: null argument");
    XH_CHECK(!h_iters || max_iters >= 0, XH_ERR_ARG, "xh_ldb_run: bad record capacity");
    XH_CHECK(h->loaded, XH_ERR_STATE, "xh_ldb_run: nothing is loaded");
    XH_CHECK(niter >= 1, XH_ERR_ARG, "xh_ldb_run: %d iterations: the sharpened map would never be assigned", niter);
    XH_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const size_t N = h->N;
    *n_iters = 0;
    *stopped = 0;
    h->tm.zero();
    double lastnorm = 0, lastporc = 1, normOrig = 0;
    int bool1 = 1;
    const double floorv = -4 * h->desvOutside;
    double *hp = h->host.f64();
    for (int32_t i = 1; i <= niter; ++i) {
        // :315-341
        XH_TRY(ldb_filter(h, i == 1 ? (const double *)h->Vorig.p : (const double *)h->sharp.p));
        XH_LAUNCH256(h->ctx, k_ldb_first, h->grid, (const double *)h->acc.p, (const double *)h->lw.p, (const double *)h->Vorig.p, dp(h->filt), N, dp(h->partials));
        XH_LAUNCH256(h->ctx, xh_k_reduce_final, 1, (const double *)h->partials.p, (int)h->grid, 2, dp(h->result));
        XH_HIP(hipMemcpyAsync(hp, h->result.p, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
        XH_HIP(hipEventRecord(h->evRec, st));
        XH_TRY(h->tm.lap(LDB_T_FINISH));
        // :367-368: the second operator does not need the record
        XH_TRY(ldb_filter(h, (const double *)h->filt.p));
        XH_HIP(hipEventSynchronize(h->evRec));
        if (i == 1) normOrig = std::sqrt(hp[1]);
        const double norm = std::sqrt(hp[0]);
        // :345-364
        const double porc = lastnorm * 100 / norm;
        const double subst = porc - lastporc;
        if ((subst < 1) && (bool1 == 1) && (i > 2)) bool1 = 2;
        lastnorm = norm;
        lastporc = porc;
        if (i == 1 && lambda == 1) lambda = (normOrig / norm) / 12;
        // :370-389
        XH_LAUNCH256(h->ctx, k_ldb_second, h->grid, (const double *)h->acc.p, (const double *)h->lw.p, i == 1 ? (const double *)h->Vorig.p : (const double *)h->sharp.p,
                     dp(h->sharp), N, lambda, floorv);
        XH_TRY(h->tm.lap(LDB_T_FINISH));
        xh_ldb_iter rec;
        std::memset(&rec, 0, sizeof(rec));
        rec.norm = norm; rec.porc = porc; rec.subst = subst; rec.lambda = lambda; rec.stop = bool1 == 2 ? 1 : 0;
        if (h_iters && *n_iters < max_iters) h_iters[*n_iters] = rec;
        ++*n_iters;
        if (bool1 == 2) { *stopped = 1; break; }
    }
    *lambda_out = lambda;
    XH_HIP(hipMemcpyAsync(d_out, h->sharp.p, h->sharp.bytes, hipMemcpyDeviceToDevice, st));
    XH_HIP(hipStreamSynchronize(st));
    return XH_OK;
}

int xh_ldb_set_timing(xh_ldb *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_ldb_set_timing: null handle");
    h->tm.set(on != 0);
    return XH_OK;
}

int xh_ldb_stage_ms(const xh_ldb *h, double *h_ms)
{
    XH_CHECK(h && h_ms, XH_ERR_ARG, "xh_ldb_stage_ms: null argument");
    h->tm.read(h_ms);
    return XH_OK;
}

}  // extern "C"
