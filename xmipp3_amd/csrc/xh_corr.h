// xh_corr.h -- the masked correlationIndex of a fixed volume x against many volumes y in one pass over y, the one place where it is written:
// what depends on x alone (n, mean_x, stddev_x, S0 = sum (x - mean_x)), formed once on the host in raster order with compensated sums, and
// the index from a trial's sums sum y, sum y^2, sum (x - mean_x) y. Used by xh_valign.hip (xmipp_volume_align, COVARIANCE) and xh_fsym.hip
// (xmipp_volume_find_symmetry). The reference makes two passes over y (mean_y first, then sum (x - mean_x)(y - mean_y)); here
//   sum (x - mean_x)(y - mean_y) = sum (x - mean_x) y - mean_y sum (x - mean_x),   sum (y - mean_y)^2 = sum y^2 - n mean_y^2
// (the second is computeAvgStdev's own form, with its integer N / (N - 1): INTEGRATION.md 3n). The rounding difference between the two
// forms is what the tests' bounds are derived from. The callers are built with -ffp-contract=off.
#ifndef XH_CORR_H
#define XH_CORR_H
#include "xh_reduce.h"
#include <cmath>

namespace {

constexpr double XH_CORR_ACC = 1e-6;        // XMIPP_EQUAL_ACCURACY

struct XhCorrStats { double n, mean_x, stddev_x, S0; };

// A sum in raster order with its rounding errors carried along (Neumaier): a plain running sum of N terms drifts by about sqrt(N) ulp, which
// the deviation's cancellation (sum x^2 / n - mean^2) multiplies; at 16^3 that alone moved a fit by 1e-14
struct XhCompSum {
    double s = 0, c = 0;
    void add(double v)
    {
        const double t = s + v;
        c += std::fabs(s) >= std::fabs(v) ? (s - t) + v : (v - t) + s;
        s = t;
    }
    double value() const { return s + c; }
};

// computeAvgStdev of x within the mask (null: every element), then sum (x - mean_x); `what` names the volume in the refusal
int xh_corr_stats(const char *who, const char *what, const double *h_x, const int32_t *h_mask, size_t N, XhCorrStats &S)
{
    long long n = 0;
    XhCompSum sum, sum2, s0;
    for (size_t e = 0; e < N; ++e)
        if (!h_mask || h_mask[e] != 0) {
            const double x = h_x[e];
            XH_CHECK(std::isfinite(x), XH_ERR_ARG, "%s: %s has a value that is not finite", who, what);
            ++n;
            sum.add(x);
            sum2.add(x * x);
        }
    S = XhCorrStats{(double)n, 0, 0, 0};
    if (n > 0) {
        S.mean_x = sum.value() / n;
        if (n > 1) {
            double sd = sum2.value() / n - S.mean_x * S.mean_x;
            sd *= (double)(n / (n - 1));
            S.stddev_x = std::sqrt(std::fabs(sd));
        }
        for (size_t e = 0; e < N; ++e)
            if (!h_mask || h_mask[e] != 0) s0.add(h_x[e] - S.mean_x);
        S.S0 = s0.value();
    }
    return XH_OK;
}

// correlationIndex with computeAvgStdev's deviation of y: sqrt(|sum y^2 / n - mean_y^2| (n / (n - 1))), the quotient in integers; 0 where
// a deviation is below 1e-6 or n <= 1
__device__ __forceinline__ double xh_corr_index(double Sy, double Sy2, double Sxy, const XhCorrStats &S)
{
    double corr = 0.0;
    if (S.n > 1) {
        const double mean_y = Sy / S.n;
        double sd = Sy2 / S.n - mean_y * mean_y;
        sd *= (double)((long long)S.n / ((long long)S.n - 1));
        sd = sqrt(fabs(sd));
        if (!(fabs(S.stddev_x) < XH_CORR_ACC || fabs(sd) < XH_CORR_ACC)) corr = (Sxy - mean_y * S.S0) / ((S.stddev_x * sd) * S.n);
    }
    return corr;
}

// a trial's partial sums [nbricks][NK], one row per 8 x 8 x 4 brick, to its totals in red[c][0]: thread t adds bricks t, t + 256, .. in
// increasing order, then the fixed tree adds the 256 sums. The order depends on the number of bricks alone
template <int NK> __device__ __forceinline__ void xh_brick_totals(const double *__restrict__ p, int nbricks, double (&red)[NK][256])
{
    double v[NK];
    for (int c = 0; c < NK; ++c) v[c] = 0.0;
    for (int b = threadIdx.x; b < nbricks; b += 256)
        for (int c = 0; c < NK; ++c) v[c] += p[(size_t)b * NK + c];
    xh_tree256(red, v);
}

}  // namespace

#endif
