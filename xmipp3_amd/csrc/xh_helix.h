// xh_helix.h -- symmetry_Helical per output voxel (data/symmetries.cpp:1632-1705) and interpolatedElement3DHelical under it (:1577-1630),
// the one place where they are written: the record of a helix (sy_make_helix, the scalars of :1635-1644), the interpolation with its recursion
// written as two nested levels, and the sum over the helical, Cn and dihedral copies of one voxel with its edge weights (sy_helical_value).
// Used by xh_sym.hip (xmipp_transform_symmetrize: one helix, every voxel) and xh_fsym.hip (xmipp_volume_find_symmetry: many helices per
// pass, the voxels of a mask); both are built with -ffp-contract=off, because kp feeds the zFirst / zLast comparisons and the floors.
// How deep the recursion goes is the caller's business: xh_sym_helical_depth and xh_fsym_helical_depth say for which parameters one
// level is enough; a corner that would need a second level reads as zero.
#ifndef XH_HELIX_H
#define XH_HELIX_H
#include "xh_volume.h"
#include <cmath>

namespace {

struct SyHelix {
    double zHelical, izHelical, rotHelical, rot0, sinRot, cosRot;
    int zFirst, zLast, zHelical2, Llength, Cn, dihedral;
};

// interpolatedElement3DHelical (symmetries.cpp:1598-1630) with interpolatedElement3DHelicalInt (:1577-1596) for its corners. LEVEL 1 is
// the point a level-0 corner outside z was sent to; with the accepted parameters its corners lie inside z (sy_helical_depth), a corner
// that does not reads as zero. Corners of weight exactly 0 are not fetched: l + (h - l) * 0 is l for any finite h.
template <int LEVEL> __device__ double sy_helical_interp(const double *__restrict__ v, XhDims d, const SyHelix &H, double x, double y, double z);

template <int LEVEL> __device__ __forceinline__ double sy_helical_corner(const double *__restrict__ v, XhDims d, const SyHelix &H, int x, int y, int z)
{
    const int sx = -(d.X / 2), sy = -(d.Y / 2), sz = -(d.Z / 2);
    if (x < sx || x > sx + d.X - 1 || y < sy || y > sy + d.Y - 1) return 0.0;
    if (z >= sz && z <= sz + d.Z - 1) return v[((size_t)(z - sz) * d.Y + (y - sy)) * d.X + (x - sx)];
    if constexpr (LEVEL >= 1) return 0.0;
    else if (z < sz) {
        const double newx = H.cosRot * x - H.sinRot * y;
        const double newy = H.sinRot * x + H.cosRot * y;
        return sy_helical_interp<LEVEL + 1>(v, d, H, newx, newy, z + H.zHelical);
    } else {
        const double newx = H.cosRot * x + H.sinRot * y;
        const double newy = -H.sinRot * x + H.cosRot * y;
        return sy_helical_interp<LEVEL + 1>(v, d, H, newx, newy, z - H.zHelical);
    }
}

template <int LEVEL> __device__ double sy_helical_interp(const double *__restrict__ v, XhDims d, const SyHelix &H, double x, double y, double z)
{
    const int x0 = (int)floor(x), y0 = (int)floor(y), z0 = (int)floor(z);
    const double fx = x - x0, fy = y - y0, fz = z - z0;
    const int x1 = x0 + 1, y1 = y0 + 1, z1 = z0 + 1;
    const bool hx = fx != 0, hy = fy != 0, hz = fz != 0;
    constexpr int L = LEVEL;
    const double d000 = sy_helical_corner<L>(v, d, H, x0, y0, z0);
    const double d001 = hx ? sy_helical_corner<L>(v, d, H, x1, y0, z0) : 0.0;
    const double d010 = hy ? sy_helical_corner<L>(v, d, H, x0, y1, z0) : 0.0;
    const double d011 = hx && hy ? sy_helical_corner<L>(v, d, H, x1, y1, z0) : 0.0;
    const double d100 = hz ? sy_helical_corner<L>(v, d, H, x0, y0, z1) : 0.0;
    const double d101 = hz && hx ? sy_helical_corner<L>(v, d, H, x1, y0, z1) : 0.0;
    const double d110 = hz && hy ? sy_helical_corner<L>(v, d, H, x0, y1, z1) : 0.0;
    const double d111 = hz && hx && hy ? sy_helical_corner<L>(v, d, H, x1, y1, z1) : 0.0;
    // LIN_INTERP(a, l, h) = l + (h - l) * a; a skipped corner stands for its partner so that the product is an exact zero
    const double dx00 = hx ? d000 + (d001 - d000) * fx : d000;
    const double dx01 = hz ? (hx ? d100 + (d101 - d100) * fx : d100) : 0.0;
    const double dx10 = hy ? (hx ? d010 + (d011 - d010) * fx : d010) : 0.0;
    const double dx11 = hz && hy ? (hx ? d110 + (d111 - d110) * fx : d110) : 0.0;
    const double dxy0 = hy ? dx00 + (dx10 - dx00) * fy : dx00;
    const double dxy1 = hz ? (hy ? dx01 + (dx11 - dx01) * fy : dx01) : 0.0;
    return hz ? dxy0 + (dxy1 - dxy0) * fz : dxy0;
}

// the voxel (k, i, j) of symmetry_Helical's output (:1659-1703): rot = atan2(i, j) + rot0 and rho = sqrt(i^2 + j^2) come from the caller,
// who may form them once for many helices. Llength + 1 terms, the edge weights with zHelical2, the Cn copies from the sin / cos table, the
// dihedral copies at (jp, -ip, -kp), finalValue / L (L == 0 gives the reference's NaN)
__device__ __forceinline__ double sy_helical_value(const double *__restrict__ vin, XhDims d, const SyHelix &H, const double *__restrict__ sinCn,
                                                   const double *__restrict__ cosCn, int k, double rot, double rho)
{
    const int l0 = (int)ceil((-(d.Z / 2) - k) * H.izHelical);
    const int lF = l0 + H.Llength;
    double finalValue = 0, L = 0;
    for (int il = l0; il <= lF; ++il) {
        const double l = il;
        const double kp = k + l * H.zHelical;
        if (kp >= H.zFirst && kp <= H.zLast) {
            const double rotp = rot + l * H.rotHelical;
            const double ip = rho * sin(rotp);
            const double jp = rho * cos(rotp);
            double weight = 1.0;
            if (kp - H.zFirst <= H.zHelical2) weight = (kp - H.zFirst + 1) / (H.zHelical2 + 1);
            else if (H.zLast - kp <= H.zHelical2) weight = (H.zLast + 1 - kp) / (H.zHelical2 + 1);
            finalValue += weight * sy_helical_interp<0>(vin, d, H, jp, ip, kp);
            L += weight;
            for (int c = 1; c < H.Cn; ++c) {
                const double jpp = cosCn[c] * jp - sinCn[c] * ip;
                const double ipp = sinCn[c] * jp + cosCn[c] * ip;
                finalValue += weight * sy_helical_interp<0>(vin, d, H, jpp, ipp, kp);
                L += weight;
            }
            if (H.dihedral) {
                finalValue += weight * sy_helical_interp<0>(vin, d, H, jp, -ip, -kp);
                L += weight;
                for (int c = 1; c < H.Cn; ++c) {
                    const double jpp = cosCn[c] * jp - sinCn[c] * (-ip);
                    const double ipp = sinCn[c] * jp + cosCn[c] * (-ip);
                    finalValue += weight * sy_helical_interp<0>(vin, d, H, jpp, ipp, -kp);
                    L += weight;
                }
            }
        }
    }
    return finalValue / L;
}

// the scalars of :1635-1644 for a box of Z planes; zHelical in voxels, the angles in radians
inline SyHelix sy_make_helix(int Z, double zHelical, double rotHelical, double rot0, double heightFraction, int Cn, bool dihedral)
{
    SyHelix H;
    const long nz = std::lround(heightFraction * Z);              // round(heightFraction * ZSIZE), :1635-1636
    H.zFirst = -(int)(nz / 2);
    H.zLast = H.zFirst + (int)nz - 1;
    H.zHelical = zHelical;
    H.izHelical = 1.0 / zHelical;
    H.zHelical2 = (int)std::floor(0.5 * zHelical);
    H.rotHelical = rotHelical;
    H.rot0 = rot0;
    H.sinRot = std::sin(rotHelical);
    H.cosRot = std::cos(rotHelical);
    H.Llength = (int)std::ceil(Z * H.izHelical);
    H.Cn = Cn;
    H.dihedral = dihedral ? 1 : 0;
    return H;
}

// sinCn [Cn] then cosCn [Cn] (:1646-1653)
inline void sy_cn_table(int Cn, double *cs)
{
    constexpr double TWO_PI = 2 * 3.14159265358979323846;
    for (int n = 0; n < Cn; ++n) {
        cs[n] = std::sin(n * TWO_PI / Cn);
        cs[Cn + n] = std::cos(n * TWO_PI / Cn);
    }
}

}  // namespace

#endif
