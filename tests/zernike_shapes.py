"""The shapes at which the device tests of xmipp_angular_sph_alignment (xh_asa.hip) and xmipp_forward_art_zernike3d (xh_faz.hip) leave
the 16-, 17- and 33-pixel case, and a restatement of the quantities each shape is in the list for: the per-workgroup partials that
k_asa_cost and k_faz_errors add (`tiles`), the images of one chunk of faz_load, the k range of k_asa_project (kmin, kmax), the padded
length of a line transform and its lines per workgroup (xh_plan_lpb as xh_fft2d64 calls it), the brick list of xh_faz_create and the
origins of k_faz_splat's LDS tiles. check_reach() asserts from the restatement the property each shape is there for: a change of a
constant that takes a shape off its path fails there by name, not by silently un-covering the path."""
import math

import numpy as np

THREADS = 256                # every kernel of both files runs 256 threads; k_asa_cost and k_faz_errors stride the partials by 256
BRICK = 16                   # xh_faz.hip: kBrick, the side of a brick of k_faz_splat
TILE = 48                    # xh_faz.hip: kTile, the side of the LDS tile of (P, W) a brick keeps
LOAD_BYTES = 256 << 20       # xh_faz.hip: faz_load prepares particles in chunks of at most 256 MiB of spectra
CD = 16                      # sizeof(xh_cd)
FFT_LDS = 64 * 1024          # xh_plan.h: xh_fft2d64's budget per workgroup
FFT_LINES = 16               # xh_plan.h: xh_fft2d64 asks for at most 16 lines per workgroup

SMALL_ASA = (16, 17)         # the sizes of the older tests
SMALL_FAZ = (16, 17, 33)

# xh_zernike.h: the (L1, L2) pairs ZK_DISPATCH names; any other pair, (0, 0) among them, runs the kernels' run-time form
PAIRS = [(l1, l2) for l1 in range(1, 6) for l2 in range(0, min(l1, 4) + 1)]
RUN_TIME = (0, 0)

# ---- xh_asa.hip
ASA_TILES = (40, 41)         # 7 workgroups per row; the last holds 64 threads with a column at 40 and 145 at 41
ASA_RDEF = [(17, 5.5), (16, 11.3), (17, 12.6)]      # (D, RDef): a non-integer RDef inside the volume, and two beyond it (the clip binds)
ASA_ROWS = (16, 600)         # (D, rows in one step): grid.y = 600
LAP = 260                    # the smallest tested D with more than 256 partials per row: the second lap of both totals loops

# ---- xh_faz.hip
FAZ_TILES = (65, 80)         # LDS tiles that lie wholly inside the image, and tiles across each of its four edges
FAZ_EXACT = (80, LAP)        # the error value where it is exact
SEAM_D, SEAM_N = 32, 16384 + 6                       # one full chunk of faz_load and six images of the next


def tiles(D):
    """workgroups of 256 projection columns (k_asa_project) or pixels (k_faz_residual): the partials per row that the totals loop adds"""
    return (D * D + THREADS - 1) // THREADS


def last_tile_threads(D):
    """threads of the last workgroup that own a column"""
    return D * D - (tiles(D) - 1) * THREADS


def laps(n, threads=THREADS):
    """laps of `for (t = tid; t < n; t += 256)` in which some thread works"""
    return -(-n // threads)


def load_chunk(D, n):
    """faz_load: chunk = max(1, min(n, 256 MiB / (D D sizeof(xh_cd))))"""
    return max(1, min(n, LOAD_BYTES // (D * D * CD)))


def load_chunks(D, n):
    """the images of each lap of faz_load: for (i0 = 0; i0 < n; i0 += chunk)"""
    c = load_chunk(D, n)
    return [min(c, n - i0) for i0 in range(0, n, c)]


def k_range(D, RDef):
    """xh_asa_create: r^2 < RDef^2 needs |k| <= B = ceil(RDef) - 1; (kmin, kmax, B) with the range clipped to the volume's logical k"""
    B = int(min(2048.0, math.ceil(RDef))) - 1
    return max(-(D // 2), -B), min(D - 1 - D // 2, B), B


def is_pow2(n):
    return n & (n - 1) == 0


def plan_M(n):
    """xh_plan_create: the LDS stride of a line of n points, n itself for a power of two and else the power of two >= 2 n - 1"""
    M = 1
    while M < (n if is_pow2(n) else 2 * n - 1):
        M <<= 1
    return M


def plan_lpb(n):
    """xh_plan_lpb as xh_fft2d64 calls it: 64 KiB, at most 16 lines"""
    return max(1, min(FFT_LINES, FFT_LDS // (CD * plan_M(n))))


def brick_grid(D):
    return (D + BRICK - 1) // BRICK


def bricks(mask, step=1):
    """xh_faz_create's forward list for one sigma: the physical origins (z, y, x), z slowest, of the 16^3 bricks that hold a non-zero
    voxel of `mask` [D, D, D] on the step lattice"""
    D, nb = mask.shape[0], brick_grid(mask.shape[0])
    on = mask != 0
    if step > 1:
        lattice = np.zeros(D, bool)
        lattice[::step] = True
        on = on & lattice[:, None, None] & lattice[None, :, None] & lattice[None, None, :]
    return [(bz * BRICK, by * BRICK, bx * BRICK) for bz in range(nb) for by in range(nb) for bx in range(nb)
            if on[bz * BRICK:(bz + 1) * BRICK, by * BRICK:(by + 1) * BRICK, bx * BRICK:(bx + 1) * BRICK].any()]


def _round_half_away(x):
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def tile_origins(D, brick_list, px, py):
    """k_faz_splat: the physical pixel (row, column) of the first entry of each brick's tile, round(projection of the brick's deformed
    centre) - 24 + D / 2; px, py [D, D, D]: the projected coordinates of every voxel (the restatement's positions())"""
    out = []
    for z, y, x in brick_list:
        ck, ci, cj = (min(o + BRICK // 2, D - 1) for o in (z, y, x))
        cx, cy = float(px[ck, ci, cj]), float(py[ck, ci, cj])
        assert abs(cx) < 1e6 and abs(cy) < 1e6
        out.append((_round_half_away(cy) - TILE // 2 + D // 2, _round_half_away(cx) - TILE // 2 + D // 2))
    return out


def tile_census(D, origins):
    """how many tiles lie wholly inside the image, and how many hang over its top, bottom, left and right edge while holding pixels of it"""
    c = dict(inside=0, top=0, bottom=0, left=0, right=0)
    for oi, oj in origins:
        if oi + TILE <= 0 or oi >= D or oj + TILE <= 0 or oj >= D:
            continue                                          # no pixel of the image: nothing of it is flushed
        top, bottom, left, right = oi < 0, oi + TILE > D, oj < 0, oj + TILE > D
        c["inside"] += not (top or bottom or left or right)
        c["top"] += top
        c["bottom"] += bottom
        c["left"] += left
        c["right"] += right
    return c


def sphere(D, R):
    k, i, j = np.meshgrid(*(np.arange(D) - D // 2,) * 3, indexing="ij", sparse=True)
    return ((k * k + i * i + j * j) <= R * R).astype(np.int32)


def check_reach():
    """every shape reaches what it is listed for; the sizes of the older tests reach none of it"""
    assert len(PAIRS) == 19 and RUN_TIME not in PAIRS and (5, 4) in PAIRS and (5, 5) not in PAIRS
    for D in SMALL_ASA + SMALL_FAZ:
        assert tiles(D) <= 5 and laps(tiles(D)) == 1 and plan_lpb(D) == FFT_LINES
        assert k_range(D, D // 2) == (-(D // 2 - 1), D // 2 - 1, D // 2 - 1)              # the default RDef: the clip does not bind
        assert load_chunks(D, 6) == [6]
    assert [tiles(D) for D in SMALL_FAZ] == [1, 2, 5]

    # more than two workgroups per row, a last workgroup that is partly idle
    assert [tiles(D) for D in ASA_TILES] == [7, 7]
    assert [last_tile_threads(D) for D in ASA_TILES] == [64, 145]

    # RDef off the default
    D, R = ASA_RDEF[0]
    kmin, kmax, B = k_range(D, R)
    assert B == 5 == math.ceil(R) - 1 and (kmin, kmax) == (-5, 5) and R != int(R) and kmax < D // 2       # ceil(RDef) - 1, unclipped
    for D, R in ASA_RDEF[1:]:
        kmin, kmax, B = k_range(D, R)
        assert kmax < math.ceil(R) - 1 == B and kmin > -B, "the clip of kmin / kmax binds"
        assert (kmin, kmax) == (-(D // 2), D - 1 - D // 2)
    assert k_range(16, 11.3) == (-8, 7, 11) and k_range(17, 12.6) == (-8, 8, 12)

    # many rows in one step
    assert ASA_ROWS[1] > 8 and tiles(ASA_ROWS[0]) == 1

    # the second lap of the totals, and fewer than 16 lines per workgroup
    assert tiles(LAP) == 265 > THREADS and laps(tiles(LAP)) == 2
    assert all(tiles(D) <= THREADS for D in range(4, 256)) and LAP * LAP > 65536
    assert plan_M(LAP) == 1024 and plan_lpb(LAP) == 4 < FFT_LINES
    assert all(plan_lpb(D) == FFT_LINES for D in ASA_TILES + FAZ_TILES + (SEAM_D,))
    assert [plan_M(D) for D in ASA_TILES + FAZ_TILES + (SEAM_D,)] == [128, 128, 256, 256, 32]

    # two chunks of the particle load
    assert load_chunk(SEAM_D, SEAM_N) == 16384 and load_chunks(SEAM_D, SEAM_N) == [16384, 6]
    assert load_chunk(16, 6) == 6 and LOAD_BYTES // (16 * 16 * CD) == 65536

    # the brick list
    for D in FAZ_TILES:
        assert brick_grid(D) == 5
    assert len(bricks(sphere(65, 32.0))) == 67 and len(bricks(sphere(80, 40.0))) == 117 < 5 ** 3
    assert len(bricks(np.ones((80, 80, 80), np.int32))) == 125
    assert len(bricks(np.ones((LAP,) * 3, np.int8))) == 17 ** 3
