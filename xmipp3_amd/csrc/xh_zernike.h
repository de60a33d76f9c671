// xh_zernike.h -- the Zernike3D basis and the trilinear sampler shared by xmipp_volume_deform_sph (xh_vds.hip),
// xmipp_angular_sph_alignment (xh_asa.hip) and xmipp_forward_art_zernike3d (xh_faz.hip, the basis alone): the radial polynomials, the
// solid harmonics, the term count, the displacement of one voxel and interpolatedElement3D; and the host side the programs need before a
// launch: the degree check, the packing of a coefficient vector
// with its effective l2, and the table of compiled (L1, L2) pairs. The mathematics and the reference's S_4^0 exception are described at
// the head of xh_vds.hip.
#ifndef XH_ZERNIKE_H
#define XH_ZERNIKE_H
#include "xh_common.h"
#include <cmath>

#define VDS_MAX_L1 5
#define VDS_MAX_L2 4
#define VDS_MAXT 45          // terms of (5, 4)
#define VDS_PI 3.14159265358979323846
#define VDS_HD __host__ __device__ __forceinline__

// ---------------------------------------------------------------- the basis
// R_l1^n(r), r2 = r^2; 0 for a pair that is no radial polynomial (n > l1, l1 - n odd)
VDS_HD double vds_radial(int l1, int n, double r, double r2)
{
    switch (l1 * 8 + n) {
        case 0 * 8 + 0: return sqrt(3.0);
        case 1 * 8 + 1: return sqrt(5.0) * r;
        case 2 * 8 + 0: return sqrt(7.0) * (2.5 * r2 - 1.5);
        case 2 * 8 + 2: return sqrt(7.0) * r2;
        case 3 * 8 + 1: return 3.0 * r * (3.5 * r2 - 2.5);
        case 3 * 8 + 3: return 3.0 * r2 * r;
        case 4 * 8 + 0: return sqrt(11.0) * ((7.875 * r2 - 8.75) * r2 + 1.875);
        case 4 * 8 + 2: return sqrt(11.0) * r2 * (4.5 * r2 - 3.5);
        case 4 * 8 + 4: return sqrt(11.0) * r2 * r2;
        case 5 * 8 + 1: return sqrt(13.0) * r * ((12.375 * r2 - 15.75) * r2 + 4.375);
        case 5 * 8 + 3: return sqrt(13.0) * r2 * r * (5.5 * r2 - 4.5);
        case 5 * 8 + 5: return sqrt(13.0) * r2 * r2 * r;
        default: return 0.0;
    }
}

// S_l2^m(x, y, z), x2 = x^2 ...
VDS_HD double vds_harmonic(int l2, int m, double x, double y, double z, double x2, double y2, double z2)
{
    switch (l2 * 16 + m + l2) {
        case 0: return 0.5 * sqrt(1.0 / VDS_PI);
        case 16 + 0: return sqrt(0.75 / VDS_PI) * y;
        case 16 + 1: return sqrt(0.75 / VDS_PI) * z;
        case 16 + 2: return sqrt(0.75 / VDS_PI) * x;
        case 32 + 0: return 0.5 * sqrt(15.0 / VDS_PI) * x * y;
        case 32 + 1: return 0.5 * sqrt(15.0 / VDS_PI) * y * z;
        case 32 + 2: return 0.25 * sqrt(5.0 / VDS_PI) * (2.0 * z2 - x2 - y2);
        case 32 + 3: return 0.5 * sqrt(15.0 / VDS_PI) * x * z;
        case 32 + 4: return 0.25 * sqrt(15.0 / VDS_PI) * (x2 - y2);
        case 48 + 0: return 0.25 * sqrt(17.5 / VDS_PI) * y * (3.0 * x2 - y2);
        case 48 + 1: return 0.5 * sqrt(105.0 / VDS_PI) * x * y * z;
        case 48 + 2: return 0.25 * sqrt(10.5 / VDS_PI) * y * (4.0 * z2 - x2 - y2);
        case 48 + 3: return 0.25 * sqrt(7.0 / VDS_PI) * z * (2.0 * z2 - 3.0 * x2 - 3.0 * y2);
        case 48 + 4: return 0.25 * sqrt(10.5 / VDS_PI) * x * (4.0 * z2 - x2 - y2);
        case 48 + 5: return 0.25 * sqrt(105.0 / VDS_PI) * z * (x2 - y2);
        case 48 + 6: return 0.25 * sqrt(17.5 / VDS_PI) * x * (x2 - 3.0 * y2);
        case 64 + 0: return 0.75 * sqrt(35.0 / VDS_PI) * x * y * (x2 - y2);
        case 64 + 1: return 0.75 * sqrt(17.5 / VDS_PI) * y * z * (3.0 * x2 - y2);
        case 64 + 2: return 0.75 * sqrt(5.0 / VDS_PI) * x * y * (6.0 * z2 - x2 - y2);
        case 64 + 3: return 0.75 * sqrt(2.5 / VDS_PI) * y * z * (4.0 * z2 - 3.0 * (x2 + y2));
        case 64 + 4: return 0.1875 * sqrt(1.0 / VDS_PI) * ((35.0 * z2 - 30.0) * z2 + 3.0);   // the reference's form, see the header
        case 64 + 5: return 0.75 * sqrt(2.5 / VDS_PI) * x * z * (4.0 * z2 - 3.0 * (x2 + y2));
        case 64 + 6: return 0.375 * sqrt(5.0 / VDS_PI) * (x2 - y2) * (6.0 * z2 - x2 - y2);
        case 64 + 7: return 0.75 * sqrt(17.5 / VDS_PI) * x * z * (x2 - 3.0 * y2);
        case 64 + 8: return 0.1875 * sqrt(35.0 / VDS_PI) * (x2 * (x2 - 6.0 * y2) + y2 * y2);
        default: return 0.0;
    }
}

// numCoefficients: terms of degrees (l1, l2)
static int vds_num_terms(int l1, int l2)
{
    int n = 0;
    for (int h = 0; h <= l2; ++h)
        for (int l = h; l <= l1; l += 2) n += 2 * h + 1;
    return n;
}

namespace {

// what the sampler needs of a volume [Z][Y][X]; a kernel's geometry struct starts with it
struct ZkDims { int Z, Y, X; };

// term idx at c[3 idx + (0, 1, 2)] = (cx, cy, cz)
struct VdsCoef { double c[3 * VDS_MAXT]; };

// ---------------------------------------------------------------- the host side
inline int zk_check_degrees(const char *who, int L1, int L2)
{
    XH_CHECK(L1 >= 0 && L2 >= 0, XH_ERR_ARG, "%s: negative degree (l1 %d, l2 %d)", who, L1, L2);
    XH_CHECK(L1 <= VDS_MAX_L1 && L2 <= VDS_MAX_L2, XH_ERR_UNSUPPORTED, "%s: degrees l1 = %d, l2 = %d are not supported (l1 <= %d, l2 <= %d)", who, L1, L2,
             VDS_MAX_L1, VDS_MAX_L2);
    return XH_OK;
}

// x [3 vecSize] (cx, then cy, then cz) -> VdsCoef's layout at c [3 VDS_MAXT]. Returns the effective l2: the smallest h whose terms hold
// every non-zero coefficient, which names the instantiation that evaluates these coefficients.
inline int zk_pack(int L1, int L2, int vecSize, const double *x, double *c)
{
    int last = -1;
    for (int i = 0; i < 3 * VDS_MAXT; ++i) c[i] = 0.0;
    for (int idx = 0; idx < vecSize; ++idx)
        for (int d = 0; d < 3; ++d) {
            const double v = x[(size_t)d * vecSize + idx];
            c[3 * idx + d] = v;
            if (v != 0.0) last = idx;      // a NaN counts as non-zero
        }
    int e = 0;
    while (e < L2 && vds_num_terms(L1, e) <= last) ++e;
    return e;
}

// The compiled (L1, L2) pairs, written once: runs STMT(A, B) with the constants A == l1 and B == l2, STMT(-1, -1) (the run-time degrees)
// for any other pair.
#define ZK_CASE_(A, B, STMT) if (zk_l1_ == A && zk_l2_ == B) { STMT(A, B); } else
#define ZK_DISPATCH(l1, l2, STMT)                                                                       \
    do {                                                                                                \
        const int zk_l1_ = (l1), zk_l2_ = (l2);                                                         \
        ZK_CASE_(1, 0, STMT) ZK_CASE_(1, 1, STMT)                                                       \
        ZK_CASE_(2, 0, STMT) ZK_CASE_(2, 1, STMT) ZK_CASE_(2, 2, STMT)                                  \
        ZK_CASE_(3, 0, STMT) ZK_CASE_(3, 1, STMT) ZK_CASE_(3, 2, STMT) ZK_CASE_(3, 3, STMT)             \
        ZK_CASE_(4, 0, STMT) ZK_CASE_(4, 1, STMT) ZK_CASE_(4, 2, STMT) ZK_CASE_(4, 3, STMT) ZK_CASE_(4, 4, STMT) \
        ZK_CASE_(5, 0, STMT) ZK_CASE_(5, 1, STMT) ZK_CASE_(5, 2, STMT) ZK_CASE_(5, 3, STMT) ZK_CASE_(5, 4, STMT) \
        { STMT(-1, -1); }                                                                               \
    } while (0)

// ---------------------------------------------------------------- the device side
// The displacement of one voxel. L1 >= 0: compile-time degrees, everything unrolls; L1 < 0: the run-time degrees (l1, l2).
// At r = 0 only the l2 = 0 terms count.
template <int L1, int L2>
__device__ __forceinline__ void vds_disp(const VdsCoef &C, int l1, int l2, double xr, double yr, double zr, double rr, double &gx, double &gy, double &gz)
{
    const double r2 = rr * rr, x2 = xr * xr, y2 = yr * yr, z2 = zr * zr;
    gx = gy = gz = 0.0;
    if constexpr (L1 >= 0) {
        int idx = 0;
#pragma unroll
        for (int h = 0; h <= L2; ++h) {
            const bool on = h == 0 || rr > 0;
            double S[2 * VDS_MAX_L2 + 1];
#pragma unroll
            for (int m = 0; m < 2 * h + 1; ++m) S[m] = vds_harmonic(h, m - h, xr, yr, zr, x2, y2, z2);
#pragma unroll
            for (int l = h; l <= L1; l += 2) {
                const double R = on ? vds_radial(l, h, rr, r2) : 0.0;
#pragma unroll
                for (int m = 0; m < 2 * h + 1; ++m) {
                    const double zsh = R * S[m];
                    gx += C.c[3 * idx] * zsh;
                    gy += C.c[3 * idx + 1] * zsh;
                    gz += C.c[3 * idx + 2] * zsh;
                    ++idx;
                }
            }
        }
    } else {
        int idx = 0;
        for (int h = 0; h <= l2; ++h) {
            const bool on = h == 0 || rr > 0;
            for (int l = h; l <= l1; l += 2) {
                const double R = on ? vds_radial(l, h, rr, r2) : 0.0;
                for (int m = -h; m <= h; ++m) {
                    const double zsh = R * vds_harmonic(h, m, xr, yr, zr, x2, y2, z2);
                    gx += C.c[3 * idx] * zsh;
                    gy += C.c[3 * idx + 1] * zsh;
                    gz += C.c[3 * idx + 2] * zsh;
                    ++idx;
                }
            }
        }
    }
}

__device__ __forceinline__ double vds_lin(double a, double l, double h) { return l + (h - l) * a; }

// interpolatedElement3D at the logical position (x, y, z), 0 outside the volume. A position whose eight taps are all outside (and a
// NaN) returns 0 before anything is converted to an index.
__device__ __forceinline__ double vds_sample(const double *__restrict__ V, const ZkDims &g, double x, double y, double z)
{
    const double px = x + (double)(g.X / 2), py = y + (double)(g.Y / 2), pz = z + (double)(g.Z / 2);
    if (!(px > -1.0 && px < (double)g.X && py > -1.0 && py < (double)g.Y && pz > -1.0 && pz < (double)g.Z)) return 0.0;
    const double fx0 = floor(px), fy0 = floor(py), fz0 = floor(pz);
    const double ax = px - fx0, ay = py - fy0, az = pz - fz0;
    const int x0 = (int)fx0, y0 = (int)fy0, z0 = (int)fz0;
    const bool xa = x0 >= 0, xb = x0 + 1 < g.X, ya = y0 >= 0, yb = y0 + 1 < g.Y, za = z0 >= 0, zb = z0 + 1 < g.Z;
    const size_t sy = (size_t)g.X, sz = (size_t)g.X * g.Y;
    const double *p = V + ((ptrdiff_t)z0 * (ptrdiff_t)sz + (ptrdiff_t)y0 * (ptrdiff_t)sy + x0);
    const double d000 = (za && ya && xa) ? p[0] : 0.0;
    const double d001 = (za && ya && xb) ? p[1] : 0.0;
    const double d010 = (za && yb && xa) ? p[sy] : 0.0;
    const double d011 = (za && yb && xb) ? p[sy + 1] : 0.0;
    const double d100 = (zb && ya && xa) ? p[sz] : 0.0;
    const double d101 = (zb && ya && xb) ? p[sz + 1] : 0.0;
    const double d110 = (zb && yb && xa) ? p[sz + sy] : 0.0;
    const double d111 = (zb && yb && xb) ? p[sz + sy + 1] : 0.0;
    const double dx00 = vds_lin(ax, d000, d001), dx01 = vds_lin(ax, d100, d101);
    const double dx10 = vds_lin(ax, d010, d011), dx11 = vds_lin(ax, d110, d111);
    return vds_lin(az, vds_lin(ay, dx00, dx10), vds_lin(ay, dx01, dx11));
}

}  // namespace

#endif
