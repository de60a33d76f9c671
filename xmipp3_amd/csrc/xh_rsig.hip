// xh_rsig.hip -- the device side of xmipp_reconstruct_significant (reconstruction/reconstruct_significant.cpp): xmippCore's general 2-D
// aligner alignImagesConsideringMirrors (data/filters.cpp:2047-2178) for every (image, gallery projection) pair, imedDistance of every
// pair (filters.cpp:1269-1318), and the two significance weightings of the program (:288-369 per image, :439-492 per direction).
//
// The unit of work is a chain: one (pair, mirror, order) triple, order 0 = shift then rotate (SR), order 1 = rotate then shift (RS).
// Chain c = (pair . mirrors + mirror) . 2 + order, pair = image . G + projection. A batch holds whole pairs. The reference runs the two
// orders of a pair interleaved, but they share nothing except the read-only inputs, so a batch runs three rounds of two phases:
// phase 0 is the shift step of the SR chains and the rotation step of the RS chains, phase 1 the other way round. Before a phase a
// kernel tests every chain's last increment against the thresholds (0.95 px, 1 degree) and writes the chains that take each step into
// a compacted list; the step's kernels run over that list only, and the host reads the two counts to size them. After round one most
// chains are under both thresholds.
//
// Everything is double precision; the file is built without FMA contraction, because values feed comparisons (thresholds, arg-max picks,
// corr > bestCorr, RS against SR, mirror against plain).
#include "xh_estimators.h"
#include <chrono>

namespace {
const double kPi = 3.14159265358979323846;
const double kAcc = 1e-6;       // XMIPP_EQUAL_ACCURACY

// trace bits of a chain: for round r (0 .. 2) bit 3 r = its shift step ran, 3 r + 1 = its rotation step ran, 3 r + 2 = a non-wrapping
// alternative replaced bestShift's answer in that shift step
enum { RS_TR_SHIFT = 1, RS_TR_ROT = 2, RS_TR_NONWRAP = 4 };

struct RsChain { int img, g, mirror, order; };
__device__ __forceinline__ RsChain rs_chain(long long c, int cpp, int G)
{
    const long long pair = c / cpp;
    const int w = (int)(c - pair * cpp);
    return RsChain{(int)(pair / G), (int)(pair % G), w >> 1, w & 1};
}

// pixel (n, m) of an image or of its mirror (selfReverseX then setXmippOrigin: the columns reversed in place)
__device__ __forceinline__ double rs_pix(const double *__restrict__ img, int D, int mirror, int n, int m) { return img[(size_t)n * D + (mirror ? D - 1 - m : m)]; }

// Matrix2D::inv of a 3 x 3 matrix (M3x3_INV): cofactors, the reciprocal of the first-column expansion of the determinant
__device__ __forceinline__ void rs_inverse(const double *m, double *o)
{
    o[0] = m[8] * m[4] - m[7] * m[5]; o[1] = -(m[8] * m[1] - m[7] * m[2]); o[2] = m[5] * m[1] - m[4] * m[2];
    o[3] = -(m[8] * m[3] - m[6] * m[5]); o[4] = m[8] * m[0] - m[6] * m[2]; o[5] = -(m[5] * m[0] - m[3] * m[2]);
    o[6] = m[7] * m[3] - m[6] * m[4]; o[7] = -(m[7] * m[0] - m[6] * m[1]); o[8] = m[4] * m[0] - m[3] * m[1];
    const double t = 1.0 / (m[0] * o[0] + m[3] * o[1] + m[6] * o[2]);
    for (int q = 0; q < 9; ++q) o[q] *= t;
}

// Matrix2D::isIdentity: every element within XMIPP_EQUAL_ACCURACY of the identity's (applyGeometry then copies its input)
__device__ __forceinline__ bool rs_is_identity(const double *m)
{
    for (int q = 0; q < 9; ++q)
        if (fabs(m[q] - (q % 4 == 0 ? 1.0 : 0.0)) > kAcc) return false;
    return true;
}

// applyGeometry's LINEAR branch of xh_image2d.h at pixel (i, j), reading an image or its mirror
__device__ __forceinline__ double rs_linear(const double *__restrict__ V1, int D, int mirror, const double *A, int i, int j)
{
    const int cen = D / 2;
    const double minp = -cen - kAcc, maxp = (D - cen - 1) + kAcc;
    const double x = (double)(j - cen), y = (double)(i - cen);
    const double xp = x * A[0] + y * A[1] + A[2], yp = x * A[3] + y * A[4] + A[5];
    if (!(xp >= minp && xp <= maxp && yp >= minp && yp <= maxp)) return 0.0;
    double wx = xp + cen;
    const int m1 = (int)wx;
    wx = wx - m1;
    const int m2 = m1 + 1;
    double wy = yp + cen;
    const int n1 = (int)wy;
    wy = wy - n1;
    const int n2 = n1 + 1;
    const double wx_1 = 1 - wx, wy_1 = 1 - wy;
    double aux2 = wy_1 * wx_1;
    double tmp = aux2 * rs_pix(V1, D, mirror, n1, m1);
    if (wx != 0 && m2 < D) tmp += (wy_1 - aux2) * rs_pix(V1, D, mirror, n1, m2);
    if (wy != 0 && n2 < D) {
        aux2 = wy * wx_1;
        tmp += aux2 * rs_pix(V1, D, mirror, n2, m1);
        if (wx != 0 && m2 < D) tmp += (wy - aux2) * rs_pix(V1, D, mirror, n2, m2);
    }
    return tmp;
}

// alignImages :2053-2066: identity matrices, the initial thresholds 1.95 px and 2 degrees as the last increments, an empty trace
__global__ void __launch_bounds__(256) k_rs_init(double *__restrict__ M, double *__restrict__ last, int *__restrict__ trace, int m)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= m) return;
    for (int q = 0; q < 9; ++q) M[9 * (size_t)b + q] = (q % 4 == 0) ? 1.0 : 0.0;
    last[3 * (size_t)b] = 0.95 + 1.0; last[3 * (size_t)b + 1] = 0.95 + 1.0; last[3 * (size_t)b + 2] = 2.0;
    trace[b] = 0;
}

// IauxSR = IauxRS = I: every chain starts from its image (or the image's mirror)
__global__ void __launch_bounds__(256) k_rs_start(const double *__restrict__ images, long long c0, int cpp, int G, int D, double *__restrict__ cur)
{
    const int per = D * D;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= per) return;
    const int b = blockIdx.y;
    const RsChain c = rs_chain(c0 + b, cpp, G);
    cur[(size_t)b * per + t] = rs_pix(images + (size_t)c.img * per, D, c.mirror, t / D, t % D);
}

// The stopping rule of :2072-2110 for one phase of one round, one workgroup: chain b of the batch takes the shift step when it is an SR
// chain in phase 0 (an RS chain in phase 1) and its last shift left +-0.95 px on either axis; it takes the rotation step when it is an
// RS chain in phase 0 (an SR chain in phase 1) and its last angle is above 1 degree. The takers go, in chain order, to list [0][..]
// (shift) and list [1][..] (rotation) of stride `cap`; count [0 .. 1] get their numbers.
__global__ void __launch_bounds__(256) k_rs_select(const double *__restrict__ last, long long c0, int m, int phase, int round, int cap, int *__restrict__ list,
                                                   int *__restrict__ count, int *__restrict__ trace)
{
    __shared__ int scan[2][256];
    __shared__ int base[2];
    if (threadIdx.x < 2) base[threadIdx.x] = 0;
    __syncthreads();
    for (int b0 = 0; b0 < m; b0 += 256) {
        const int b = b0 + threadIdx.x;
        int take[2] = {0, 0};
        if (b < m) {
            const int order = (int)((c0 + b) & 1);
            const double sx = last[3 * (size_t)b], sy = last[3 * (size_t)b + 1], rot = last[3 * (size_t)b + 2];
            if (order == phase) take[0] = ((sx > 0.95) || (sx < -0.95)) || ((sy > 0.95) || (sy < -0.95));
            else take[1] = rot > 1.0;
        }
        scan[0][threadIdx.x] = take[0]; scan[1][threadIdx.x] = take[1];
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            int v[2] = {0, 0};
            if ((int)threadIdx.x >= o) { v[0] = scan[0][threadIdx.x - o]; v[1] = scan[1][threadIdx.x - o]; }
            __syncthreads();
            scan[0][threadIdx.x] += v[0]; scan[1][threadIdx.x] += v[1];
            __syncthreads();
        }
        for (int k = 0; k < 2; ++k)
            if (take[k]) list[(size_t)k * cap + base[k] + scan[k][threadIdx.x] - 1] = b;
        if (b < m && (take[0] || take[1])) trace[b] |= (take[0] ? RS_TR_SHIFT : RS_TR_ROT) << (3 * round);
        __syncthreads();
        if (threadIdx.x < 2) base[threadIdx.x] += scan[threadIdx.x][255];
        __syncthreads();
    }
    if (threadIdx.x < 2) count[threadIdx.x] = base[threadIdx.x];
}

// the current images of the listed chains as complex doubles, list order
__global__ void __launch_bounds__(256) k_rs_gather_complex(const double *__restrict__ cur, const int *__restrict__ list, int per, xh_cd *__restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= per) return;
    out[(size_t)blockIdx.y * per + t] = xh_cd{cur[(size_t)list[blockIdx.y] * per + t], 0.0};
}

// the forward transform with FourierTransformer's normalisation (divided by the size)
__global__ void __launch_bounds__(256) k_rs_scale(xh_cd *__restrict__ F, size_t total, double size)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    F[t] = xh_cd{F[t].x / size, F[t].y / size};
}

// correlation_matrix (filters.cpp: FFT1 . conj(FFT2) . size, both transforms divided by the size) of each listed chain's image against its
// projection's spectrum; the (-1)^(x + y) is CenterFFT(R, true) for an even size, applied before the inverse transform
__global__ void __launch_bounds__(256) k_rs_correlate(xh_cd *__restrict__ W, const xh_cd *__restrict__ galSpec, const int *__restrict__ list, long long c0, int cpp, int G, int D)
{
    const int per = D * D;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    const RsChain ch = rs_chain(c0 + list[blockIdx.y], cpp, G);
    const double dSize = (double)per;
    const xh_cd f1 = galSpec[(size_t)ch.g * per + e];
    xh_cd f2 = W[(size_t)blockIdx.y * per + e];
    f2.x /= dSize; f2.y /= dSize;
    const double a = f1.x, b = f1.y, c = f2.x * dSize, d = f2.y * (-dSize);
    xh_cd v = xh_cd{a * c - b * d, b * c + a * d};
    if (((e / D) + (e % D)) & 1) { v.x = -v.x; v.y = -v.y; }
    W[(size_t)blockIdx.y * per + e] = v;
}

// bestShift (filters.cpp:1593-1719, no mask, maxShift = -1) on the centred correlation map of each listed chain (the real parts of W):
// statisticsAdjust(0, 1), the first maximum in raster order, the square that grows around it while every value stays above max / 1.414
// and inside the map, its centre of mass. The growth is found in one pass as in xh_pm.hip: the squares are nested, so the one the
// reference stops at is the smallest Chebyshev distance from the maximum to a value below the threshold or to the border. Where the
// sum of the square is 0 the reference leaves the shifts as they came in: the chain's last increment.
__global__ void __launch_bounds__(256) k_rs_bestshift(const xh_cd *__restrict__ W, const int *__restrict__ list, const double *__restrict__ last, int D, double *__restrict__ shifts)
{
    __shared__ double red[1][256];
    __shared__ double sv[256];
    __shared__ int si[256];
    const int n = D * D, cen = D / 2;
    const xh_cd *R = W + (size_t)blockIdx.x * n;
    double s1 = 0, s2 = 0;
    for (int t = threadIdx.x; t < n; t += 256) { const double v = R[t].x; s1 += v; s2 += v * v; }
    const double S1 = xh_block_sum(s1, red), S2 = xh_block_sum(s2, red);
    const double avg = S1 / n;
    const double sd = sqrt(fabs(S2 / n - avg * avg));
    const double a = sd != 0 ? 1.0 / sd : 0.0, b = sd != 0 ? -avg * a : 0.0;
    double bv = -1.0e300;
    int bi = 0x7fffffff;
    for (int t = threadIdx.x; t < n; t += 256) {
        const double v = a * R[t].x + b;
        if (v > bv || (v == bv && t < bi)) { bv = v; bi = t; }
    }
    sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double ov = sv[threadIdx.x + o];
            const int oi = si[threadIdx.x + o];
            if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    const int tmax = si[0];
    const double mx = sv[0], thr = mx / 1.414;
    __syncthreads();
    const int start = -cen, fin = start + D - 1;
    const int imax = tmax / D + start, jmax = tmax % D + start;
    int nf = min(min(imax - start, fin - imax), min(jmax - start, fin - jmax)) + 1;
    for (int t = threadIdx.x; t < n; t += 256) {
        const double v = a * R[t].x + b;
        if (thr > v) nf = min(nf, max(abs(t / D + start - imax), abs(t % D + start - jmax)));
    }
    si[threadIdx.x] = nf;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) si[threadIdx.x] = min(si[threadIdx.x], si[threadIdx.x + o]);
        __syncthreads();
    }
    int n_max = si[0];
    // :1693-1700 (the x tests compare against the y limits there; the map is square)
    if (imax - n_max < start) n_max = min(imax - start, n_max);
    if (imax + n_max > fin) n_max = min(fin - imax, n_max);
    if (jmax - n_max < start) n_max = min(jmax - start, n_max);
    if (jmax + n_max > fin) n_max = min(fin - jmax, n_max);
    double xmax = 0, ymax = 0, sumcorr = 0;
    const int wd = 2 * n_max + 1;
    for (int t = threadIdx.x; t < wd * wd; t += 256) {
        const int ia = t / wd - n_max + imax, ja = t % wd - n_max + jmax;
        const double val = a * R[(size_t)(ia - start) * D + (ja - start)].x + b;
        ymax += ia * val;
        xmax += ja * val;
        sumcorr += val;
    }
    const double YM = xh_block_sum(ymax, red), XM = xh_block_sum(xmax, red), SC = xh_block_sum(sumcorr, red);
    if (threadIdx.x == 0) {
        const int c = list[blockIdx.x];
        double ox = last[3 * (size_t)c], oy = last[3 * (size_t)c + 1];
        if (SC != 0) { ox = XM / SC; oy = YM / SC; }
        shifts[2 * (size_t)blockIdx.x] = ox; shifts[2 * (size_t)blockIdx.x + 1] = oy;
    }
}

// The rest of bestNonwrappingShift (filters.cpp:1910-1984) and the shift's place in the chain (:2076-2077), one workgroup per listed
// chain. The projection is translated by bestShift's answer and by the three answers a full period away on x, on y and on both
// (translate LINEAR, DONT_WRAP: by -shift, through its inverse), each copy correlated with the chain's image by fastCorrelation. The
// four copies are built pixel by pixel from one pass over the projection. As written in the reference, every alternative is compared
// with the first copy's correlation, never with an earlier alternative's, and replaces on a strict >.
__global__ void __launch_bounds__(256) k_rs_nonwrap(const double *__restrict__ gal, const double *__restrict__ cur, const int *__restrict__ list, const double *__restrict__ shifts,
                                                    long long c0, int cpp, int G, int D, int round, double *__restrict__ M, double *__restrict__ last, int *__restrict__ trace)
{
    __shared__ double red[4][256];
    const int per = D * D;
    const int b = list[blockIdx.x];
    const RsChain ch = rs_chain(c0 + b, cpp, G);
    const double *ref = gal + (size_t)ch.g * per, *img = cur + (size_t)b * per;
    const double sx = shifts[2 * (size_t)blockIdx.x], sy = shifts[2 * (size_t)blockIdx.x + 1];
    const double tX = (sx > 0) ? (sx - D) : (sx + D), tY = (sy > 0) ? (sy - D) : (sy + D);
    const double cx[4] = {sx, tX, sx, tX}, cy[4] = {sy, sy, tY, tY};
    double acc[4] = {0, 0, 0, 0};
    for (int t = threadIdx.x; t < per; t += 256) {
        const double v = img[t];
        for (int q = 0; q < 4; ++q) {
            // translation2DMatrix(-shift) inverted is the translation by +shift; within XMIPP_EQUAL_ACCURACY of the identity the copy is exact
            const double A[6] = {1.0, 0.0, cx[q], 0.0, 1.0, cy[q]};
            const bool ident = fabs(cx[q]) <= kAcc && fabs(cy[q]) <= kAcc;
            acc[q] += v * (ident ? ref[t] : rs_linear(ref, D, 0, A, t / D, t % D));
        }
    }
    xh_tree256(red, acc);
    if (threadIdx.x == 0) {
        const double best = red[0][0] / per;
        double fx = sx, fy = sy;
        if (red[1][0] / per > best) fx = tX;
        if (red[2][0] / per > best) fy = tY;
        if (red[3][0] / per > best) { fx = tX; fy = tY; }
        if (fx != sx || fy != sy) trace[b] |= RS_TR_NONWRAP << (3 * round);
        M[9 * (size_t)b + 2] += fx;
        M[9 * (size_t)b + 5] += fy;
        last[3 * (size_t)b] = fx; last[3 * (size_t)b + 1] = fy;
    }
}

// applyGeometry(LINEAR, Iaux, I, A, IS_NOT_INV, DONT_WRAP) of :2078 / :2089: each listed chain's ORIGINAL image (or its mirror) through
// the inverse of the accumulated matrix
__global__ void __launch_bounds__(256) k_rs_apply(const double *__restrict__ images, const int *__restrict__ list, const double *__restrict__ M, long long c0, int cpp, int G,
                                                  int D, double *__restrict__ cur)
{
    __shared__ double A[9];
    __shared__ int ident;
    const int per = D * D;
    const int b = list[blockIdx.y];
    if (threadIdx.x == 0) {
        ident = rs_is_identity(M + 9 * (size_t)b);
        rs_inverse(M + 9 * (size_t)b, A);
    }
    __syncthreads();
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= per) return;
    const RsChain ch = rs_chain(c0 + b, cpp, G);
    const double *src = images + (size_t)ch.img * per;
    cur[(size_t)b * per + t] = ident ? rs_pix(src, D, ch.mirror, t / D, t % D) : rs_linear(src, D, ch.mirror, A, t / D, t % D);
}

// getPolarFromCartesianBSpline(.., BsplineOrder 1) as k_es_polar_linear samples it, of double images picked through a list (null: image
// blockIdx.y itself)
__global__ void __launch_bounds__(256) k_rs_polar(const double *__restrict__ imgs, const int *__restrict__ list, const float *__restrict__ sx, const float *__restrict__ sy,
                                                  int nsamples, int D, double *__restrict__ rings)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nsamples) return;
    const double *img = imgs + (size_t)(list ? list[blockIdx.y] : (int)blockIdx.y) * D * D;
    const int first = -(D / 2), last = first + D - 1;
    const double minp = first, maxp = last;
    double xp = (double)sx[t], yp = (double)sy[t];
    if (xp < minp - 1e-6 || xp > maxp + 1e-6) xp = d_realwrap<double>(xp, minp - 0.5, maxp + 0.5);
    if (yp < minp - 1e-6 || yp > maxp + 1e-6) yp = d_realwrap<double>(yp, minp - 0.5, maxp + 0.5);
    const int x0 = (int)floor(xp), y0 = (int)floor(yp);
    const double fx = xp - x0, fy = yp - y0;
    auto at = [&](int i, int j) -> double { return (j < first || j > last || i < first || i > last) ? 0.0 : img[(size_t)(i - first) * D + (j - first)]; };
    const double d00 = at(y0, x0), d01 = at(y0, x0 + 1), d10 = at(y0 + 1, x0), d11 = at(y0 + 1, x0 + 1);
    const double d0 = d00 + (d01 - d00) * fx, d1 = d10 + (d11 - d10) * fx;
    rings[(size_t)blockIdx.y * nsamples + t] = d0 + (d1 - d0) * fy;
}

// Polar::computeAverageAndStddev and normalize (polar.h:488-546), one workgroup per transform: ring r's samples weigh 2 pi r / nsam,
// wsum is the sum of all the weights
__global__ void __launch_bounds__(256) k_rs_polar_normalize(double *__restrict__ rings, const EsRing *__restrict__ ringTab, int nrings, int nsamples, double wsum)
{
    __shared__ double red[2][256];
    double *x = rings + (size_t)blockIdx.x * nsamples;
    double acc[2] = {0, 0};
    for (int r = 0; r < nrings; ++r) {
        const EsRing R = ringTab[r];
        const double w = R.w / (double)R.nsam;
        for (int s = threadIdx.x; s < R.nsam; s += 256) {
            const double aux = x[R.soff + s], waux = w * aux;
            acc[0] += waux;
            acc[1] += waux * aux;
        }
    }
    xh_tree256(red, acc);
    const double avg = red[0][0] / wsum;
    const double stddev = sqrt(fabs(red[1][0] / wsum - avg * avg));
    const double istddev = 1.0 / stddev;
    for (int s = threadIdx.x; s < nsamples; s += 256) x[s] = (x[s] - avg) * istddev;
}

// rotationalCorrelation's ring sum (polar.cpp:122-135) of each listed chain against its projection's transform
__global__ void __launch_bounds__(256) k_rs_rot_fsum(const double2 *__restrict__ Fref, const double2 *__restrict__ F, const EsRing *__restrict__ ringTab, int nrings, int ncoefs,
                                                     int nh, const int *__restrict__ list, long long c0, int cpp, int G, double2 *__restrict__ Fsum)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nh) return;
    const RsChain ch = rs_chain(c0 + list[blockIdx.y], cpp, G);
    Fsum[(size_t)blockIdx.y * nh + k] = es_rot_fsum_at(Fref + (size_t)ch.g * ncoefs, F + (size_t)blockIdx.y * ncoefs, ringTab, nrings, k);
}

// best_rotation's angle (polar.cpp:145-147, 230) and :2087-2088 / :2098-2099: A = rotation2DMatrix(angle) . A
__global__ void __launch_bounds__(256) k_rs_pose_rotate(const int *__restrict__ imax, int len, const int *__restrict__ list, int count, double *__restrict__ M,
                                                        double *__restrict__ last)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const int b = list[k];
    const double Kaux = 360. / len;
    const double rot = (double)imax[k] * Kaux;
    const double ang = rot * kPi / 180.0;
    const double c = cos(ang), s = sin(ang);
    const double r[9] = {c, s, 0, -s, c, 0, 0, 0, 1};
    double *p = M + 9 * (size_t)b, o[9];
    for (int i = 0; i < 3; ++i)
        for (int q = 0; q < 3; ++q) o[3 * i + q] = r[3 * i] * p[q] + r[3 * i + 1] * p[3 + q] + r[3 * i + 2] * p[6 + q];
    for (int q = 0; q < 9; ++q) p[q] = o[q];
    last[3 * (size_t)b + 2] = rot;
}

// correlationIndex(Iaux, Iref) of :2113-2114 (no mask: population statistics, two passes) and imedDistance(projection, Iaux) of the
// program (:221; filters.cpp:1269-1318, the 7 x 7 weights exp(-(x^2 + y^2) / 2) / sqrt(2 pi) from their formula), one workgroup per chain
__global__ void __launch_bounds__(256) k_rs_chain_final(const double *__restrict__ gal, const double *__restrict__ cur, long long c0, int cpp, int G, int D,
                                                        double *__restrict__ corr, double *__restrict__ imed)
{
    __shared__ double red4[4][256];
    __shared__ double red[1][256];
    __shared__ double w[49];
    const int per = D * D;
    const int b = blockIdx.x;
    const RsChain ch = rs_chain(c0 + b, cpp, G);
    const double *x = cur + (size_t)b * per, *y = gal + (size_t)ch.g * per;
    if (threadIdx.x < 49) {
        const int u = (int)threadIdx.x / 7 - 3, v = (int)threadIdx.x % 7 - 3;
        w[threadIdx.x] = exp(-0.5 * (u * u + v * v)) / sqrt(2.0 * kPi);
    }
    double acc[4] = {0, 0, 0, 0};
    for (int t = threadIdx.x; t < per; t += 256) { const double p = x[t], q = y[t]; acc[0] += p; acc[1] += q; acc[2] += p * p; acc[3] += q * q; }
    xh_tree256(red4, acc);
    const double n = (double)per;
    const double mx = red4[0][0] / n, my = red4[1][0] / n;
    const double sx = sqrt(fabs(red4[2][0] / n - mx * mx)), sy = sqrt(fabs(red4[3][0] / n - my * my));
    double r = 0;
    for (int t = threadIdx.x; t < per; t += 256) r += (x[t] - mx) * (y[t] - my);
    r = xh_block_sum(r, red);
    double e = 0;
    const int mid = D / 2, R2max = mid * mid;
    for (int t = threadIdx.x; t < per; t += 256) {
        const int i = t / D, j = t % D;
        if (i < 3 || i >= D - 3 || j < 3 || j >= D - 3) continue;
        if ((i - mid) * (i - mid) + (j - mid) * (j - mid) > R2max) continue;
        const double diffi = y[t] - x[t];
        for (int ii = -3; ii <= 3; ++ii) {
            double aux = 0;
            for (int jj = -3; jj <= 3; ++jj) { const int u = t + ii * D + jj; aux += w[(ii + 3) * 7 + (jj + 3)] * (y[u] - x[u]); }
            e += aux * diffi;
        }
    }
    e = xh_block_sum(e, red);
    if (threadIdx.x == 0) {
        corr[b] = (fabs(sx) < kAcc || fabs(sy) < kAcc) ? 0.0 : r / ((sx * sy) * n);
        imed[b] = sqrt(e);
    }
}

// :2116-2127 and :2168-2177, thread per pair of the batch: corrRS > corrSR picks the order, corrMirror > corr the mirror (first column
// of the matrix negated). The pair's trace: bit 0 the mirror won, bit 1 RS won, bits 2 .. 10 the winning mirror's SR chain, bits 11 .. 19
// its RS chain. With chain outputs given, every chain's matrix, correlation, imed and trace are written as well.
__global__ void __launch_bounds__(256) k_rs_pair_final(const double *__restrict__ M, const double *__restrict__ corr, const double *__restrict__ imed, const int *__restrict__ trace,
                                                       int pairs, int cpp, double *__restrict__ oM, double *__restrict__ oCorr, double *__restrict__ oImed, int *__restrict__ oTrace,
                                                       double *__restrict__ cM, double *__restrict__ cCorr, double *__restrict__ cImed, int *__restrict__ cTrace)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    int win[2], rs[2];
    for (int mir = 0; mir < cpp / 2; ++mir) {
        const int sr = p * cpp + 2 * mir;
        rs[mir] = corr[sr + 1] > corr[sr];
        win[mir] = sr + rs[mir];
    }
    int mir = 0;
    if (cpp == 4 && corr[win[1]] > corr[win[0]]) mir = 1;
    const int b = win[mir];
    for (int q = 0; q < 9; ++q) oM[9 * (size_t)p + q] = (mir && (q == 0 || q == 3)) ? -M[9 * (size_t)b + q] : M[9 * (size_t)b + q];
    oCorr[p] = corr[b];
    oImed[p] = imed[b];
    if (oTrace) oTrace[p] = mir | (rs[mir] << 1) | (trace[p * cpp + 2 * mir] << 2) | (trace[p * cpp + 2 * mir + 1] << 11);
    if (cM)
        for (int c = p * cpp; c < (p + 1) * cpp; ++c) {
            for (int q = 0; q < 9; ++q) cM[9 * (size_t)c + q] = M[9 * (size_t)c + q];
            cCorr[c] = corr[c]; cImed[c] = imed[c]; cTrace[c] = trace[c];
        }
}

// ---- the weights
// transformationMatrix2Parameters2D of M.inv() (:216-219): the shifts only
__device__ __forceinline__ void rs_shifts_of(const double *M, double &shiftX, double &shiftY)
{
    double A[9];
    rs_inverse(M, A);
    const bool flip = (A[0] * A[4] - A[1] * A[3]) < 0;
    const int sgn = flip ? -1 : 1;
    const double cosine = sgn * A[0], sine = sgn * A[1];
    const double scale = sqrt(cosine * cosine + sine * sine);
    const double invScale = 1 / scale;
    shiftX = A[2] * invScale; shiftY = A[5] * invScale;
}

// :222-226: a pair shifted beyond maxShift on either axis has its correlation divided by 3 and its imed multiplied by 3, in place
__global__ void __launch_bounds__(256) k_rs_penalty(const double *__restrict__ M, size_t pairs, double maxShift, double *__restrict__ cc, double *__restrict__ imed)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    double sx, sy;
    rs_shifts_of(M + 9 * p, sx, sy);
    if (fabs(sx) > maxShift || fabs(sy) > maxShift) { cc[p] /= 3; imed[p] *= 3; }
}

// The weights of one image (:288-369), one workgroup per image over its G pairs: bestCorr and bestImed, the Fisher limit, the two
// cumulative density functions (cdf (i) = the 1-based ascending rank of element i over G, equal values ranked by position, counted
// through LDS tiles), the selection, the maxShift rejection, the weight. Pairs not selected keep weight 0.
__global__ void __launch_bounds__(256) k_rs_image_weights(const double *__restrict__ M, const double *__restrict__ cc, const double *__restrict__ imed, int G, double oneAlpha,
                                                          double fisherTerm, int applyFisher, int useImed, double maxShift, double *__restrict__ weight)
{
    __shared__ double tc[256], ti[256];
    __shared__ double red[2][256];
    const size_t base = (size_t)blockIdx.x * G;
    double bc = -2, bi = 1e38;
    for (int g = threadIdx.x; g < G; g += 256) {
        if (cc[base + g] > bc) bc = cc[base + g];
        if (imed[base + g] < bi) bi = imed[base + g];
    }
    red[0][threadIdx.x] = bc; red[1][threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            if (red[0][threadIdx.x + o] > red[0][threadIdx.x]) red[0][threadIdx.x] = red[0][threadIdx.x + o];
            if (red[1][threadIdx.x + o] < red[1][threadIdx.x]) red[1][threadIdx.x] = red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    const double bestCorr = red[0][0], bestImed = red[1][0];
    const double rl = bestCorr * oneAlpha;
    const double z = 0.5 * log((1 + rl) / (1 - rl));
    const double ccl = tanh(z - fisherTerm);
    for (int g0 = 0; g0 < G; g0 += 256) {
        const int g = g0 + threadIdx.x;
        const double vc = g < G ? cc[base + g] : 0.0, vi = g < G ? imed[base + g] : 0.0;
        int rc = 0, ri = 0;
        for (int t0 = 0; t0 < G; t0 += 256) {
            const int wdt = min(256, G - t0);
            __syncthreads();
            if ((int)threadIdx.x < wdt) { tc[threadIdx.x] = cc[base + t0 + threadIdx.x]; ti[threadIdx.x] = imed[base + t0 + threadIdx.x]; }
            __syncthreads();
            for (int k = 0; k < wdt; ++k) {
                rc += (tc[k] < vc || (tc[k] == vc && t0 + k < g)) ? 1 : 0;
                ri += (ti[k] < vi || (ti[k] == vi && t0 + k < g)) ? 1 : 0;
            }
        }
        if (g >= G) continue;
        const double cdfcc = (double)(rc + 1) / (double)G, cdfimed = (double)(ri + 1) / (double)G;
        double wgt = 0;
        bool condition = (applyFisher && vc >= ccl) || !applyFisher;
        condition = condition && cdfcc >= oneAlpha;
        if (condition && maxShift > 0) {
            double sx, sy;
            rs_shifts_of(M + 9 * (base + g), sx, sy);
            if (fabs(sx) > maxShift || fabs(sy) > maxShift) condition = false;
        }
        if (condition) {
            wgt = cdfcc * (vc / bestCorr);
            if (useImed) wgt *= (1 - cdfimed) * (bestImed / vi);
        }
        weight[base + g] = wgt;
    }
}

// The reweighting of one direction (:439-492), one workgroup row per direction g over the N images: as written, the neighbour loop
// re-reads the direction's own correlations, so the list is the N values repeated 1 + k [g] times, k the number of directions of the
// same volume closer than --angDistance. The cdf of image i's first copy in that list is ((1 + k) less (i) + equalBefore (i) + 1) /
// ((1 + k) N): one ranking of N values, never the list itself.
__global__ void __launch_bounds__(256) k_rs_direction_max(const double *__restrict__ cc, int N, int G, double *__restrict__ best)
{
    __shared__ double red[256];
    const int g = blockIdx.x;
    double b = -2;
    for (int i = threadIdx.x; i < N; i += 256)
        if (cc[(size_t)i * G + g] > b) b = cc[(size_t)i * G + g];
    red[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && red[threadIdx.x + o] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) best[g] = red[0];
}

__global__ void __launch_bounds__(256) k_rs_direction_weights(const double *__restrict__ cc, const int *__restrict__ nbr, const double *__restrict__ best, int N, int G,
                                                              double oneAlpha, int strict, double *__restrict__ weight)
{
    __shared__ double tile[256];
    const int g = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double v = i < N ? cc[(size_t)i * G + g] : 0.0;
    long long less = 0, eqBefore = 0;
    for (int t0 = 0; t0 < N; t0 += 256) {
        const int wdt = min(256, N - t0);
        __syncthreads();
        if ((int)threadIdx.x < wdt) tile[threadIdx.x] = cc[(size_t)(t0 + threadIdx.x) * G + g];
        __syncthreads();
        for (int k = 0; k < wdt; ++k) {
            less += tile[k] < v ? 1 : 0;
            eqBefore += (tile[k] == v && t0 + k < i) ? 1 : 0;
        }
    }
    if (i >= N) return;
    const long long copies = 1 + nbr[g];
    const double cdf = (double)(copies * less + eqBefore + 1) / (double)(copies * N);
    const double iBestCorr = 1.0 / best[g];
    double &w = weight[(size_t)i * G + g];
    if ((cdf >= oneAlpha || !strict) && w > 0) w *= v * iBestCorr * cdf;
    else w = 0;
}
}  // namespace

struct xh_rsig {
    xh_ctx *ctx = nullptr;
    int D = 0, maxG = 0, cap = 0, G = 0;
    double wsum = 0;                  // the sum of the polar sample weights (computeAverageAndStddev's N)
    EsRotation rot;
    XhFft2d64 fft;
    XhBuf gal, galSpec, Fref;         // per projection: pixels, FourierTransformer spectrum, normalised polar ring DFT
    XhBuf cur, work, M, last, trace, list, count, shifts, corr, imed;
    XhPinned hcount;
    XhEvent ev0, ev1;
    double stats[13] = {};            // steps, shift chains of rounds 1 .. 3, rotation chains of rounds 1 .. 3, seconds of align, of the two weightings, of the shift and rotation steps (timed runs), host seconds of the weights' neighbour count
    XhBuf wNbr, wBest;                // of the weights: neighbours per direction, best correlation per direction (grow-only)
    int timing = 0;                   // a timed run brackets every step with events and waits for it
    XhEvent evS0, evS1;
    ~xh_rsig()
    {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
};

static unsigned rs_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// polarFourierTransform<true>(.., conjugated, D / 5, D / 2, BsplineOrder 1) of n images (through a list, or images 0 .. n - 1)
static int rs_polar_transform(xh_rsig *h, const double *d_imgs, const int *d_list, int n, int conjugate, double2 *d_coefs)
{
    xh_ctx *ctx = h->ctx;
    EsRotation &R = h->rot;
    hipLaunchKernelGGL(k_rs_polar, dim3(rs_blocks(R.nsamples), n), dim3(256), 0, ctx->stream, d_imgs, d_list, (const float *)R.sx.p, (const float *)R.sy.p, R.nsamples, R.D,
                       (double *)R.rings.p);
    XH_LAUNCH256(ctx, k_rs_polar_normalize, n, (double *)R.rings.p, (const EsRing *)R.ringTab.p, R.nrings, R.nsamples, h->wsum);
    const size_t smem = sizeof(double) * (size_t)(R.maxNsam + (R.maxNsam & 1)) + sizeof(double2) * (size_t)R.maxNsam;
    hipLaunchKernelGGL(k_es_ring_dft, dim3(R.nrings, n), dim3(256), smem, ctx->stream, (const double *)R.rings.p, (const EsRing *)R.ringTab.p, R.nsamples, R.ncoefs, conjugate, d_coefs);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

// bestNonwrappingShift and its place in the chain for the `count` chains of list [0]
static int rs_step_shift(xh_rsig *h, const double *d_images, long long c0, int cpp, int count, int round)
{
    xh_ctx *ctx = h->ctx;
    const int D = h->D, per = D * D;
    const int *list = (const int *)h->list.p;
    xh_cd *w = (xh_cd *)h->work.p;
    hipLaunchKernelGGL(k_rs_gather_complex, dim3(rs_blocks(per), count), dim3(256), 0, ctx->stream, (const double *)h->cur.p, list, per, w);
    XH_TRY(xh_fft2d64(ctx, h->fft, w, count, false));
    hipLaunchKernelGGL(k_rs_correlate, dim3(rs_blocks(per), count), dim3(256), 0, ctx->stream, w, (const xh_cd *)h->galSpec.p, list, c0, cpp, h->G, D);
    XH_TRY(xh_fft2d64(ctx, h->fft, w, count, true));
    XH_LAUNCH256(ctx, k_rs_bestshift, count, (const xh_cd *)w, list, (const double *)h->last.p, D, (double *)h->shifts.p);
    XH_LAUNCH256(ctx, k_rs_nonwrap, count, (const double *)h->gal.p, (const double *)h->cur.p, list, (const double *)h->shifts.p, c0, cpp, h->G, D, round, (double *)h->M.p,
                 (double *)h->last.p, (int *)h->trace.p);
    hipLaunchKernelGGL(k_rs_apply, dim3(rs_blocks(per), count), dim3(256), 0, ctx->stream, d_images, list, (const double *)h->M.p, c0, cpp, h->G, D, (double *)h->cur.p);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

// the rotation step for the `count` chains of list [1]
static int rs_step_rotation(xh_rsig *h, const double *d_images, long long c0, int cpp, int count)
{
    xh_ctx *ctx = h->ctx;
    EsRotation &R = h->rot;
    const int *list = (const int *)h->list.p + h->cap;
    XH_TRY(rs_polar_transform(h, (const double *)h->cur.p, list, count, 1, (double2 *)R.coefs.p));
    hipLaunchKernelGGL(k_rs_rot_fsum, dim3(rs_blocks(R.N), count), dim3(256), 0, ctx->stream, (const double2 *)h->Fref.p, (const double2 *)R.coefs.p, (const EsRing *)R.ringTab.p,
                       R.nrings, R.ncoefs, R.N, list, c0, cpp, h->G, (double2 *)R.Fsum.p);
    hipLaunchKernelGGL(k_es_rot_corr, dim3(rs_blocks(R.len), count), dim3(256), sizeof(double2) * (size_t)R.N, ctx->stream, (const double2 *)R.Fsum.p, R.N, R.len, (double *)R.corr.p);
    XH_LAUNCH256(ctx, k_es_first_max, count, (const double *)R.corr.p, R.len, (int *)R.imax.p);
    XH_LAUNCH256(ctx, k_rs_pose_rotate, rs_blocks(count), (const int *)R.imax.p, R.len, list, count, (double *)h->M.p, (double *)h->last.p);
    hipLaunchKernelGGL(k_rs_apply, dim3(rs_blocks((size_t)h->D * h->D), count), dim3(256), 0, ctx->stream, d_images, list, (const double *)h->M.p, c0, cpp, h->G, h->D,
                       (double *)h->cur.p);
    XH_LAUNCH_CHECK();
    return XH_OK;
}

extern "C" {

int xh_rsig_destroy(xh_rsig *h)
{
    delete h;
    return XH_OK;
}

int xh_rsig_create(xh_ctx *ctx, int32_t D, int32_t max_gallery, int32_t batch_chains, xh_rsig **out)
{
    XH_CHECK(ctx && out, XH_ERR_ARG, "xh_rsig_create: bad argument");
    XH_CHECK(D >= 16 && (D & 1) == 0, XH_ERR_ARG, "xh_rsig_create: images of %d pixels (an even size of at least 16)", D);
    XH_CHECK(max_gallery >= 1, XH_ERR_ARG, "xh_rsig_create: %d gallery projections (at least 1)", max_gallery);
    XH_CHECK(batch_chains >= 1 && batch_chains <= 65532, XH_ERR_ARG, "xh_rsig_create: %d chains per batch (1 .. 65532)", batch_chains);
    XH_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<xh_rsig> h(new xh_rsig);
    h->ctx = ctx; h->D = D; h->maxG = max_gallery;
    h->cap = std::max(batch_chains, 4);          // a batch holds whole pairs: at least the four chains of one
    const size_t per = (size_t)D * D, B = (size_t)h->cap;
    XH_TRY(es_rotation_plan(ctx, D, D / 5, D / 2, h->rot));
    XH_TRY(xh_fft2d64_create(ctx, D, D, h->fft, "xh_rsig_create"));
    EsRotation &R = h->rot;
    // computeAverageAndStddev adds every sample's weight, ring after ring
    for (int r = 0; r < R.nrings; ++r) {
        const double radius = (float)r + (float)R.first;
        const int nsam = std::max(1, 2 * (int)(0.5 * 1.0 * 6.2831853071795864769 * (float)radius));
        const double w = (2. * kPi * radius) / (double)nsam;
        for (int s = 0; s < nsam; ++s) h->wsum += w;
    }
    XH_TRY(xh_buf_alloc(ctx, h->gal, sizeof(double) * per * max_gallery));
    XH_TRY(xh_buf_alloc(ctx, h->galSpec, sizeof(xh_cd) * per * max_gallery));
    XH_TRY(xh_buf_alloc(ctx, h->Fref, sizeof(double2) * (size_t)R.ncoefs * max_gallery));
    XH_TRY(xh_buf_alloc(ctx, R.coefs, sizeof(double2) * (size_t)R.ncoefs * B));
    XH_TRY(xh_buf_alloc(ctx, R.Fsum, sizeof(double2) * (size_t)R.N * B));
    XH_TRY(xh_buf_alloc(ctx, R.corr, sizeof(double) * (size_t)R.len * B));
    XH_TRY(xh_buf_alloc(ctx, R.imax, sizeof(int) * B));
    XH_TRY(xh_buf_alloc(ctx, R.rings, sizeof(double) * (size_t)R.nsamples * B));
    XH_TRY(xh_buf_alloc(ctx, h->cur, sizeof(double) * per * B));
    XH_TRY(xh_buf_alloc(ctx, h->work, sizeof(xh_cd) * per * B));
    XH_TRY(xh_buf_alloc(ctx, h->M, sizeof(double) * 9 * B));
    XH_TRY(xh_buf_alloc(ctx, h->last, sizeof(double) * 3 * B));
    XH_TRY(xh_buf_alloc(ctx, h->trace, sizeof(int) * B));
    XH_TRY(xh_buf_alloc(ctx, h->list, sizeof(int) * 2 * B));
    XH_TRY(xh_buf_alloc(ctx, h->count, sizeof(int) * 2));
    XH_TRY(xh_buf_alloc(ctx, h->shifts, sizeof(double) * 2 * B));
    XH_TRY(xh_buf_alloc(ctx, h->corr, sizeof(double) * B));
    XH_TRY(xh_buf_alloc(ctx, h->imed, sizeof(double) * B));
    XH_TRY(xh_pinned_alloc(ctx, h->hcount, sizeof(int) * 2));
    XH_TRY(xh_event_create(h->ev0));
    XH_TRY(xh_event_create(h->ev1));
    XH_TRY(xh_event_create(h->evS0));
    XH_TRY(xh_event_create(h->evS1));
    *out = h.release();
    return XH_OK;
}

int xh_rsig_load_gallery(xh_rsig *h, const double *d_gallery, int32_t G)
{
    XH_CHECK(h && d_gallery && G >= 1 && G <= h->maxG, XH_ERR_ARG, "xh_rsig_load_gallery: %d projections (1 .. %d)", G, h ? h->maxG : 0);
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const size_t per = (size_t)h->D * h->D, total = per * G;
    EsRotation &R = h->rot;
    XH_HIP(hipMemcpyAsync(h->gal.p, d_gallery, sizeof(double) * total, hipMemcpyDeviceToDevice, ctx->stream));
    XH_LAUNCH256(ctx, xh_k_to_complex64<double>, rs_blocks(total), d_gallery, (xh_cd *)h->galSpec.p, total);
    XH_TRY(xh_fft2d64(ctx, h->fft, (xh_cd *)h->galSpec.p, G, false));
    XH_LAUNCH256(ctx, k_rs_scale, rs_blocks(total), (xh_cd *)h->galSpec.p, total, (double)per);
    // the polar transforms in slices of the batch capacity: the ring samples pass through the batch's buffer
    for (int g0 = 0; g0 < G; g0 += h->cap) {
        const int n = std::min(h->cap, G - g0);
        XH_TRY(rs_polar_transform(h, d_gallery + per * g0, nullptr, n, 0, (double2 *)h->Fref.p + (size_t)R.ncoefs * g0));
    }
    XH_HIP(hipStreamSynchronize(ctx->stream));
    h->G = G;
    return XH_OK;
}

int xh_rsig_align(xh_rsig *h, const double *d_images, int32_t N, int32_t check_mirrors, double *d_M, double *d_corr, double *d_imed, int32_t *d_trace, double *d_chain_M,
                  double *d_chain_corr, double *d_chain_imed, int32_t *d_chain_trace)
{
    XH_CHECK(h && d_images && N >= 1 && d_M && d_corr && d_imed, XH_ERR_ARG, "xh_rsig_align: bad argument");
    XH_CHECK((!d_chain_M && !d_chain_corr && !d_chain_imed && !d_chain_trace) || (d_chain_M && d_chain_corr && d_chain_imed && d_chain_trace), XH_ERR_ARG,
             "xh_rsig_align: the chain outputs come together or not at all");
    XH_CHECK(h->G >= 1, XH_ERR_STATE, "xh_rsig_align: no gallery loaded");
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const int cpp = check_mirrors ? 4 : 2, D = h->D, per = D * D;
    const long long pairs = (long long)N * h->G;
    const int ppb = h->cap / cpp;
    int *hc = (int *)h->hcount.p;
    for (int q = 0; q < 8; ++q) h->stats[q] = 0;
    h->stats[10] = h->stats[11] = 0;
    XH_HIP(hipEventRecord(h->ev0, ctx->stream));
    for (long long p0 = 0; p0 < pairs; p0 += ppb) {
        const int np = (int)std::min<long long>(ppb, pairs - p0), m = np * cpp;
        const long long c0 = p0 * cpp;
        XH_LAUNCH256(ctx, k_rs_init, rs_blocks(m), (double *)h->M.p, (double *)h->last.p, (int *)h->trace.p, m);
        hipLaunchKernelGGL(k_rs_start, dim3(rs_blocks(per), m), dim3(256), 0, ctx->stream, d_images, c0, cpp, h->G, D, (double *)h->cur.p);
        XH_LAUNCH_CHECK();
        for (int round = 0; round < 3; ++round)
            for (int phase = 0; phase < 2; ++phase) {
                XH_LAUNCH256(ctx, k_rs_select, 1, (const double *)h->last.p, c0, m, phase, round, h->cap, (int *)h->list.p, (int *)h->count.p, (int *)h->trace.p);
                XH_HIP(hipMemcpyAsync(hc, h->count.p, sizeof(int) * 2, hipMemcpyDeviceToHost, ctx->stream));
                XH_HIP(hipStreamSynchronize(ctx->stream));
                const int ns = hc[0], nr = hc[1];
                XH_CHECK(ns >= 0 && nr >= 0 && ns + nr <= m, XH_ERR_STATE, "xh_rsig_align: %d + %d chains selected of %d", ns, nr, m);
                for (int kind = 0; kind < 2; ++kind) {
                    const int cnt = kind ? nr : ns;
                    if (!cnt) continue;
                    if (h->timing) XH_HIP(hipEventRecord(h->evS0, ctx->stream));
                    if (kind) XH_TRY(rs_step_rotation(h, d_images, c0, cpp, cnt));
                    else XH_TRY(rs_step_shift(h, d_images, c0, cpp, cnt, round));
                    h->stats[0] += 1; h->stats[1 + 3 * kind + round] += cnt;
                    if (h->timing) {
                        float ms = 0;
                        XH_HIP(hipEventRecord(h->evS1, ctx->stream));
                        XH_HIP(hipEventSynchronize(h->evS1));
                        XH_HIP(hipEventElapsedTime(&ms, h->evS0, h->evS1));
                        h->stats[10 + kind] += ms * 1e-3;
                    }
                }
            }
        XH_LAUNCH256(ctx, k_rs_chain_final, m, (const double *)h->gal.p, (const double *)h->cur.p, c0, cpp, h->G, D, (double *)h->corr.p, (double *)h->imed.p);
        XH_LAUNCH256(ctx, k_rs_pair_final, rs_blocks(np), (const double *)h->M.p, (const double *)h->corr.p, (const double *)h->imed.p, (const int *)h->trace.p, np, cpp, d_M + 9 * p0,
                     d_corr + p0, d_imed + p0, d_trace ? d_trace + p0 : nullptr, d_chain_M ? d_chain_M + 9 * c0 : nullptr, d_chain_M ? d_chain_corr + c0 : nullptr,
                     d_chain_M ? d_chain_imed + c0 : nullptr, d_chain_M ? d_chain_trace + c0 : nullptr);
    }
    XH_HIP(hipEventRecord(h->ev1, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    XH_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->stats[7] = ms * 1e-3;
    return XH_OK;
}

int xh_rsig_weights(xh_rsig *h, const double *d_M, double *d_cc, double *d_imed, int32_t N, int32_t n_vols, int32_t n_dirs, const double *h_rot, const double *h_tilt,
                    double ang_distance, double one_alpha, int32_t apply_fisher, int32_t use_imed, int32_t strict, double max_shift, double *d_weight)
{
    XH_CHECK(h && d_M && d_cc && d_imed && d_weight && h_rot && h_tilt && N >= 1 && n_vols >= 1 && n_dirs >= 1, XH_ERR_ARG, "xh_rsig_weights: bad argument");
    XH_CHECK((long long)n_vols * n_dirs <= 0x7fffffffLL / 9 && n_vols * n_dirs <= 65535, XH_ERR_ARG, "xh_rsig_weights: %d x %d directions (at most 65535)", n_vols, n_dirs);
    xh_ctx *ctx = h->ctx;
    XH_HIP(hipSetDevice(ctx->device));
    const int G = n_vols * n_dirs;
    const size_t pairs = (size_t)N * G;
    // Euler_distanceBetweenAngleSets(rot1, tilt1, 0, rot2, tilt2, 0, true): the angle between the projection directions, in degrees;
    // k [g] = the directions of the same volume sharply closer than ang_distance (:456-473)
    const auto th0 = std::chrono::steady_clock::now();
    std::vector<double> dir(3 * (size_t)G);
    for (int g = 0; g < G; ++g) {
        const double a = h_rot[g] * kPi / 180., b = h_tilt[g] * kPi / 180.;
        dir[3 * g] = std::sin(b) * std::cos(a); dir[3 * g + 1] = std::sin(b) * std::sin(a); dir[3 * g + 2] = std::cos(b);
    }
    std::vector<int> nbr(G, 0);
    for (int v = 0; v < n_vols; ++v)
        for (int d1 = 0; d1 < n_dirs; ++d1)
            for (int d2 = 0; d2 < n_dirs; ++d2) {
                if (d1 == d2) continue;
                const double *p = &dir[3 * (size_t)(v * n_dirs + d1)], *q = &dir[3 * (size_t)(v * n_dirs + d2)];
                const double dot = p[0] * q[0] + p[1] * q[1] + p[2] * q[2];
                const double ang = std::acos(std::min(1.0, std::max(-1.0, dot))) * 180. / kPi;
                if (ang < ang_distance) ++nbr[v * n_dirs + d1];
            }
    h->stats[12] = std::chrono::duration<double>(std::chrono::steady_clock::now() - th0).count();
    XH_TRY(xh_buf_reserve(ctx, h->wNbr, sizeof(int) * nbr.size()));
    XH_TRY(xh_buf_reserve(ctx, h->wBest, sizeof(double) * G));
    XH_HIP(hipMemcpyAsync(h->wNbr.p, nbr.data(), sizeof(int) * nbr.size(), hipMemcpyHostToDevice, ctx->stream));       // nbr lives until the wait below
    XH_HIP(hipEventRecord(h->ev0, ctx->stream));
    if (max_shift > 0) XH_LAUNCH256(ctx, k_rs_penalty, rs_blocks(pairs), d_M, pairs, max_shift, d_cc, d_imed);
    const double fisherTerm = 2.96 * std::sqrt(1.0 / ((double)h->D * h->D));
    XH_LAUNCH256(ctx, k_rs_image_weights, N, d_M, (const double *)d_cc, (const double *)d_imed, G, one_alpha, fisherTerm, apply_fisher, use_imed, max_shift, d_weight);
    XH_HIP(hipEventRecord(h->ev1, ctx->stream));
    XH_LAUNCH256(ctx, k_rs_direction_max, G, (const double *)d_cc, N, G, (double *)h->wBest.p);
    hipLaunchKernelGGL(k_rs_direction_weights, dim3(rs_blocks(N), G), dim3(256), 0, ctx->stream, (const double *)d_cc, (const int *)h->wNbr.p, (const double *)h->wBest.p, N, G, one_alpha,
                       strict, d_weight);
    XH_LAUNCH_CHECK();
    XH_HIP(hipEventRecord(h->evS1, ctx->stream));
    XH_HIP(hipStreamSynchronize(ctx->stream));
    float ms1 = 0, ms2 = 0;
    XH_HIP(hipEventElapsedTime(&ms1, h->ev0, h->ev1));
    XH_HIP(hipEventElapsedTime(&ms2, h->ev1, h->evS1));
    h->stats[8] = ms1 * 1e-3; h->stats[9] = ms2 * 1e-3;
    return XH_OK;
}

int xh_rsig_set_timing(xh_rsig *h, int32_t on)
{
    XH_CHECK(h, XH_ERR_ARG, "xh_rsig_set_timing: null handle");
    h->timing = on != 0;
    return XH_OK;
}

int xh_rsig_stats(const xh_rsig *h, double *h_stats)
{
    XH_CHECK(h && h_stats, XH_ERR_ARG, "xh_rsig_stats: bad argument");
    for (int q = 0; q < 13; ++q) h_stats[q] = h->stats[q];
    return XH_OK;
}

}  // extern "C"
