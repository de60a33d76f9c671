// The tile list of k_rf_grid (xh_rf_grid.h): which tiles the launch visits, and in which order the ring hands them out.
// Plain C++, no HIP: xh_rf_create calls it, and so does tools/tile_order_dump.cpp, from which the schedule model
// (tools/sim_grid_schedule.py) and tests/test_rf_tile_order.py read the very order the device gets.
//
// A tile is 2 x 2 x 2 units (16 x 16 x 8 voxels), packed as tx | ty << 10 | tz << 20. The list holds the tiles a projection can
// reach (sphere of radius sizeX + blob around the origin of the Fourier volume, voxel mv / 2 on every axis), cut in raster order
// (z, y, x) into 8 contiguous z-slabs of equal estimated work, one class per XCD (block b runs on XCD b % 8: a projection's patch
// is pulled into one or two L2s instead of all eight). A tile at distance rho from the origin is crossed by a fraction ~1 / rho of
// all central planes: that is its weight in the split.
//
// Inside a class:
//   head       the heavy tiles, heaviest first (ties by Morton key). Every central slice passes through the origin, so the units
//              next to it are visited by every projection of a launch, and one wave owns a unit for the whole launch: such a unit
//              is a sizeable fraction of the mean load of a wave (0.6 of it at mv 512 with 3072 waves). Handed out late it ends
//              long after the rest of the chip has run dry; handed out first it is done well before.
//   remainder  Morton order (the waves of the chip work on a narrow band of consecutive tiles, and a compact band shares more of
//              the projections' patches in the L2 than a row of the raster).
// Stream j of a class takes its entries j, j + 8, ...: consecutive head tiles fall into different streams.
#ifndef XH_RF_TILES_H
#define XH_RF_TILES_H

#include <algorithm>
#include <cmath>
#include <vector>

// a tile is heavy when its heaviest unit is estimated at more than this fraction of the mean load of a wave
// (profiles/experiments/rf_tile_order_ab.txt has the sweep)
#ifndef XG_HEAVY_FRAC
#define XG_HEAVY_FRAC 0.05
#endif

struct XgTileList {
    std::vector<unsigned> tiles;    // packed, class by class
    int classOff[9];                // class c: tiles[classOff[c]] .. tiles[classOff[c + 1] - 1]
    int head[8];                    // heavy tiles at the start of class c
};

// Morton order; tiles are half as tall as wide: on (x, y, z / 2) with the low bit of z last
inline unsigned long long xg_tile_key(unsigned t)
{
    auto spread = [](unsigned v) { unsigned long long x = v & 0x3ff; x = (x | x << 16) & 0x30000ffULL; x = (x | x << 8) & 0x300f00fULL; x = (x | x << 4) & 0x30c30c3ULL; x = (x | x << 2) & 0x9249249ULL; return x; };
    return (spread(t & 0x3ff) | spread((t >> 10) & 0x3ff) << 1 | spread((t >> 21) & 0x1ff) << 2) << 1 | ((t >> 20) & 1);
}

// Estimated work of unit (sub & 1, sub >> 1 & 1, sub >> 2) of a tile, as the fraction of isotropic central planes that reach it:
// min(1, w / rho), rho the distance of the unit's centre from the origin, w the half-width of the kernel's cull test, blob radius
// + support of the box of voxel centres (half extents 3.5, 3.5, 1.5) along the plane's normal, here at its mean over isotropic
// normals, (3.5 + 3.5 + 1.5) / 2. Units past the sphere the kernel keeps do no work.
inline double xg_unit_estimate(unsigned t, int sub, int mv, double blobRadius)
{
    const int tx = t & 0x3ff, ty = (t >> 10) & 0x3ff, tz = (t >> 20) & 0x3ff;
    const double cx = tx * 16 + (sub & 1) * 8 + 3.5 - mv / 2, cy = ty * 16 + ((sub >> 1) & 1) * 8 + 3.5 - mv / 2, cz = tz * 8 + (sub >> 2) * 4 + 1.5 - mv / 2;
    const double rho = std::sqrt(cx * cx + cy * cy + cz * cz);
    if (rho > mv / 2 + blobRadius + 5.2) return 0.0;
    const double w = blobRadius + 4.25;
    return rho <= w ? 1.0 : w / rho;
}
// ... and of a tile: that of its heaviest unit (a unit is never shared, a tile's eight units go to eight waves)
inline double xg_tile_estimate(unsigned t, int mv, double blobRadius)
{
    double e = 0;
    for (int sub = 0; sub < 8; ++sub) e = std::max(e, xg_unit_estimate(t, sub, mv, blobRadius));
    return e;
}

// waves: the waves the launch keeps resident, CUs x XgCfg::NW
inline XgTileList xg_tile_list(int mv, double blobRadius, int waves, double heavyFrac = XG_HEAVY_FRAC)
{
    XgTileList L;
    const int tzs = 8;                                     // voxels per tile in z
    const int tpx = (mv + 1 + 15) / 16, tpz = (mv + 1 + tzs - 1) / tzs;
    const double hz = 0.5 * tzs - 0.5;
    const double R = mv / 2 + blobRadius + std::sqrt(2 * 7.5 * 7.5 + hz * hz) + 1.0;
    std::vector<unsigned> &packed = L.tiles;
    std::vector<double> wsum;
    double acc = 0;
    for (int tz = 0; tz < tpz; ++tz)
        for (int ty = 0; ty < tpx; ++ty)
            for (int tx = 0; tx < tpx; ++tx) {
                const double cx = tx * 16 + 7.5 - mv / 2, cy = ty * 16 + 7.5 - mv / 2, cz = tz * tzs + hz - mv / 2;
                const double d = std::sqrt(cx * cx + cy * cy + cz * cz);
                if (d <= R) { packed.push_back((unsigned)(tx | (ty << 10) | (tz << 20))); acc += 1.0 / std::max(d, 8.0); wsum.push_back(acc); }
            }
    L.classOff[0] = 0;
    for (int c = 1; c < 8; ++c)
        L.classOff[c] = (int)(std::lower_bound(wsum.begin(), wsum.end(), acc * c / 8.0) - wsum.begin());
    L.classOff[8] = (int)packed.size();
    // the mean load of a wave, in the unit of the estimate (1 = a unit that every projection visits)
    double total = 0;
    for (unsigned t : packed)
        for (int sub = 0; sub < 8; ++sub) total += xg_unit_estimate(t, sub, mv, blobRadius);
    const double heavy = heavyFrac * total / std::max(1, waves);
    auto est = [&](unsigned t) { return xg_tile_estimate(t, mv, blobRadius); };
    for (int c = 0; c < 8; ++c) {
        const auto b = packed.begin() + L.classOff[c], e = packed.begin() + L.classOff[c + 1];
        const auto mid = std::partition(b, e, [&](unsigned t) { return est(t) > heavy; });
        std::sort(b, mid, [&](unsigned u, unsigned w) { const double eu = est(u), ew = est(w); return eu != ew ? eu > ew : xg_tile_key(u) < xg_tile_key(w); });
        std::sort(mid, e, [&](unsigned u, unsigned w) { return xg_tile_key(u) < xg_tile_key(w); });
        L.head[c] = (int)(mid - b);
    }
    return L;
}

#endif
