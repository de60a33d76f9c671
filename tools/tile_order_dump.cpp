// Prints the tile list k_rf_grid gets (xmipp3_amd/csrc/xh_rf_tiles.h), for tools/sim_grid_schedule.py and tests/test_rf_tile_order.py:
//   c++ -O1 -std=c++17 -I xmipp3_amd/csrc tools/tile_order_dump.cpp -o tile_order_dump
//   tile_order_dump <mv> <blob radius> <waves> [heavy fraction | morton]
// "morton": no heads, every class in Morton order throughout (the order before the heads were introduced).
// Output: "mv M radius R waves W tiles N", "classOff" + 9 ints, "head" + 8 ints, then per tile "tx ty tz estimate" in list order.
#include "xh_rf_tiles.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s <mv> <blob radius> <waves> [heavy fraction | morton]\n", argv[0]); return 2; }
    const int mv = atoi(argv[1]), waves = atoi(argv[3]);
    const double radius = atof(argv[2]);
    if (mv < 2 || mv > 2048 || !(radius > 0) || waves < 1) { fprintf(stderr, "%s: bad argument\n", argv[0]); return 2; }
    double frac = XG_HEAVY_FRAC;
    if (argc > 4) frac = strcmp(argv[4], "morton") ? atof(argv[4]) : std::numeric_limits<double>::infinity();
    const XgTileList L = xg_tile_list(mv, radius, waves, frac);
    printf("mv %d radius %.17g waves %d tiles %zu\n", mv, radius, waves, L.tiles.size());
    printf("classOff");
    for (int c = 0; c < 9; ++c) printf(" %d", L.classOff[c]);
    printf("\nhead");
    for (int c = 0; c < 8; ++c) printf(" %d", L.head[c]);
    printf("\n");
    for (unsigned t : L.tiles) printf("%u %u %u %.17g\n", t & 0x3ff, (t >> 10) & 0x3ff, (t >> 20) & 0x3ff, xg_tile_estimate(t, mv, radius));
    return 0;
}
