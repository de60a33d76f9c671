// xh_applygeo.h -- xmippCore's 3-D applyGeometry per output voxel, the one place where it is written: the per-axis range test (WRAP:
// realWRAP; DONT_WRAP: the outside value), the trilinear rule with the behaviours kept as written ((int) truncation, m2 >= dim -> 0 under
// wrap, the w != 0 && m2 < dim guards), the 4 x 4 x 4 mirrored cubic-spline taps, and the cofactor inverse the host forms for a matrix.
// Used by xh_sym.hip (xmipp_transform_symmetrize), xh_valign.hip (xmipp_volume_align) and xh_fsym.hip (xmipp_volume_find_symmetry); all are built with -ffp-contract=off, because
// the source coordinates feed comparisons. xmippCore is not in the reference tree: INTEGRATION.md 3m says what this restates.
#ifndef XH_APPLYGEO_H
#define XH_APPLYGEO_H
#include "xh_volume.h"
#include "xh_bspline.h"

namespace {

constexpr double SY_ACC = 1e-6;        // XMIPP_EQUAL_ACCURACY

__device__ __forceinline__ int sy_clamp(int v, int n) { return min(max(v, 0), n - 1); }
__device__ __forceinline__ int sy_mirror(int l, int n) { return sy_clamp(l < 0 ? -l - 1 : (l >= n ? 2 * n - l - 1 : l), n); }

// one axis of applyGeometry's range test: true = the voxel gets the outside value (DONT_WRAP only)
template <bool WRAP> __device__ __forceinline__ bool sy_axis(double &c, int dim)
{
    const int cen = dim / 2;
    const double lo = -cen, hi = dim - cen - 1;
    if (c < lo - SY_ACC || c > hi + SY_ACC) {
        if (!WRAP) return true;
        c = d_realwrap(c, lo - 0.5, hi + 0.5);
    }
    return false;
}

// the value of the source (degree 1: the volume; degree 3: its coefficients) at the logical point (xp, yp, zp), inside the range
template <int DEG, bool WRAP>
__device__ __forceinline__ double sy_interp3(const double *__restrict__ src, XhDims d, double xp, double yp, double zp)
{
    const size_t sy = d.X, sz = (size_t)d.Y * d.X;
    if (DEG == 1) {
        double wx = xp + d.X / 2;
        int m1 = (int)wx;
        wx = wx - m1;
        int m2 = m1 + 1;
        double wy = yp + d.Y / 2;
        int n1 = (int)wy;
        wy = wy - n1;
        int n2 = n1 + 1;
        double wz = zp + d.Z / 2;
        int o1 = (int)wz;
        wz = wz - o1;
        int o2 = o1 + 1;
        if (WRAP) {
            if (m2 >= d.X) m2 = 0;
            if (n2 >= d.Y) n2 = 0;
            if (o2 >= d.Z) o2 = 0;
        }
        m1 = sy_clamp(m1, d.X); n1 = sy_clamp(n1, d.Y); o1 = sy_clamp(o1, d.Z);      // in range already; a stray coordinate reads inside
        m2 = max(m2, 0); n2 = max(n2, 0); o2 = max(o2, 0);
        const bool mx = wx != 0 && m2 < d.X, my = wy != 0 && n2 < d.Y, mz = wz != 0 && o2 < d.Z;
        const double wx_1 = 1 - wx, wy_1 = 1 - wy, wz_1 = 1 - wz;
        double tmp = wz_1 * wy_1 * wx_1 * src[o1 * sz + n1 * sy + m1];
        if (mx) tmp += wz_1 * wy_1 * wx * src[o1 * sz + n1 * sy + m2];
        if (my) {
            tmp += wz_1 * wy * wx_1 * src[o1 * sz + n2 * sy + m1];
            if (mx) tmp += wz_1 * wy * wx * src[o1 * sz + n2 * sy + m2];
        }
        if (mz) {
            tmp += wz * wy_1 * wx_1 * src[o2 * sz + n1 * sy + m1];
            if (mx) tmp += wz * wy_1 * wx * src[o2 * sz + n1 * sy + m2];
            if (my) {
                tmp += wz * wy * wx_1 * src[o2 * sz + n2 * sy + m1];
                if (mx) tmp += wz * wy * wx * src[o2 * sz + n2 * sy + m2];
            }
        }
        return tmp;
    } else {
        const double x = xp + d.X / 2, y = yp + d.Y / 2, z = zp + d.Z / 2;
        const int l1 = (int)ceil(x - 2), m1 = (int)ceil(y - 2), n1 = (int)ceil(z - 2);
        double wx[4], wy[4], wz[4];
        d_bspline03_w4<double>(x, l1, wx);
        d_bspline03_w4<double>(y, m1, wy);
        d_bspline03_w4<double>(z, n1, wz);
        int el[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) el[t] = sy_mirror(l1 + t, d.X);
        double slices = 0;
#pragma unroll
        for (int tz = 0; tz < 4; ++tz) {
            const double *pz = src + sy_mirror(n1 + tz, d.Z) * sz;
            double columns = 0;
#pragma unroll
            for (int ty = 0; ty < 4; ++ty) {
                const double *ref = pz + sy_mirror(m1 + ty, d.Y) * sy;
                double rows = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) rows += ref[el[u]] * wx[u];
                columns += rows * wy[ty];
            }
            slices += columns * wz[tz];
        }
        return slices;
    }
}

// the inverse by cofactors: adjugate entries times 1 / det, det expanded along the first row (the tests' restatement forms it the same way)
void sy_inv3x3(const double *A, double *B)
{
    const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5], g = A[6], h = A[7], i = A[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    const double id = 1.0 / det;
    B[0] = (e * i - f * h) * id; B[1] = (c * h - b * i) * id; B[2] = (b * f - c * e) * id;
    B[3] = (f * g - d * i) * id; B[4] = (a * i - c * g) * id; B[5] = (c * d - a * f) * id;
    B[6] = (d * h - e * g) * id; B[7] = (b * g - a * h) * id; B[8] = (a * e - b * d) * id;
}

}  // namespace

#endif
