// xh_image2d.h -- the 2-D image pieces shared by the continuous assignment (xh_ca2.hip) and the Zernike3D alignment (xh_asa.hip):
// FourierFilter's raised-cosine low pass and applyGeometry's LINEAR branch, in doubles.
#ifndef XH_IMAGE2D_H
#define XH_IMAGE2D_H
#include "xh_common.h"

namespace {
const double kAcc = 1e-6;       // XMIPP_EQUAL_ACCURACY

// FourierFilter LOWPASS / RAISED_COSINE (fourier_filter.cpp:423-432) at the digital frequency absw
__device__ __forceinline__ double d_lowpass_raised_cosine(double absw, double w1, double raised_w)
{
    double m;
    if (absw < w1) m = 1;
    else if (absw < w1 + raised_w) m = (1 + cos(3.14159265358979323846 / raised_w * (absw - w1))) / 2;
    else m = 0;
    return m;
}

// applyGeometry's 2-D LINEAR branch at one output pixel (i, j), DONT_WRAP, outside 0; A is the matrix already inverted (rows 0 and 1).
// The same interpolation as xh_apply_geometry2d's, in doubles.
__device__ __forceinline__ double d_ca2_linear(const double *__restrict__ V1, int D, const double *A, int i, int j)
{
    const int cen = D / 2;
    const double minp = -cen - kAcc, maxp = (D - cen - 1) + kAcc;
    const double x = (double)(j - cen), y = (double)(i - cen);
    const double xp = x * A[0] + y * A[1] + A[2], yp = x * A[3] + y * A[4] + A[5];
    if (!(xp >= minp && xp <= maxp && yp >= minp && yp <= maxp)) return 0.0;      // a NaN coordinate is outside, too
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
    double tmp = aux2 * V1[(size_t)n1 * D + m1];
    if (wx != 0 && m2 < D) tmp += (wy_1 - aux2) * V1[(size_t)n1 * D + m2];
    if (wy != 0 && n2 < D) {
        aux2 = wy * wx_1;
        tmp += aux2 * V1[(size_t)n2 * D + m1];
        if (wx != 0 && m2 < D) tmp += (wy - aux2) * V1[(size_t)n2 * D + m2];
    }
    return tmp;
}
}  // namespace

#endif
