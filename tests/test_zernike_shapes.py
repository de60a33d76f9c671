"""The shapes of tests/zernike_shapes.py reach the laps, chunks, clips, tiles and bricks they are listed for (no device needed: the
restatement of the launch sizes and constants of xh_asa.hip, xh_faz.hip and xh_plan.h against the property each shape is there for)."""
import math

import numpy as np
import pytest

from tests import zernike_shapes as S


def test_shapes_reach_their_paths():
    S.check_reach()


def test_260_is_past_one_lap_of_the_totals_and_below_16_lines():
    assert S.tiles(S.LAP) == 265 > S.THREADS
    assert S.laps(S.tiles(S.LAP)) == 2 and S.laps(S.tiles(256)) == 1
    assert next(D for D in range(4, 400) if S.tiles(D) > S.THREADS) == 257
    assert S.plan_lpb(S.LAP) == 4 < S.FFT_LINES and S.plan_lpb(256) == S.FFT_LINES


def test_the_load_case_needs_two_chunks():
    chunks = S.load_chunks(S.SEAM_D, S.SEAM_N)
    assert len(chunks) > 1 and chunks == [16384, 6]
    assert S.load_chunks(S.SEAM_D, 16384) == [16384]


@pytest.mark.parametrize("D,RDef", S.ASA_RDEF[1:])
def test_the_large_rdef_cases_are_clipped(D, RDef):
    kmin, kmax, B = S.k_range(D, RDef)
    assert kmax < math.ceil(RDef) - 1 and kmin > -(math.ceil(RDef) - 1)
    k = np.arange(D) - D // 2
    assert (kmin, kmax) == (k[0], k[-1])


def test_the_small_rdef_case_takes_the_ceiling():
    D, RDef = S.ASA_RDEF[0]
    kmin, kmax, B = S.k_range(D, RDef)
    assert (kmin, kmax) == (-5, 5) and B == math.ceil(RDef) - 1
    assert 5 * 5 < RDef * RDef < 6 * 6                        # k = 5 is inside the ball and k = 6 is not: int(RDef) - 1 would lose a plane


@pytest.mark.parametrize("D", S.FAZ_TILES)
def test_tiles_inside_the_image_and_across_each_edge(oracle, D):
    """the generic case of the device tests: 48 x 48 tiles that no image edge clips, and tiles over every edge"""
    from tests.test_gpu_forward_art_zernike3d import GENERIC, Art, coefficients
    ref = Art(oracle, D, 3, 2)
    px, py = ref.positions(ref.rotations(GENERIC)[0], coefficients(ref, 5 + D, 1.5))
    listed = S.bricks(ref.maskf)
    census = S.tile_census(D, S.tile_origins(D, listed, px, py))
    print(f"D {D}: {len(listed)} of {S.brick_grid(D) ** 3} bricks, tiles {census}")
    assert census["inside"] >= 1
    for edge in ("top", "bottom", "left", "right"):
        assert census[edge] >= 1, edge
    assert len(listed) == {65: 67, 80: 117}[D]
    assert census["inside"] == {65: 8, 80: 23}[D]
    if D == 80:
        assert len(listed) < S.brick_grid(D) ** 3


@pytest.mark.parametrize("D", S.SMALL_FAZ)
def test_no_tile_of_the_older_sizes_lies_inside_the_image(D):
    assert D < S.TILE                                          # a 48 x 48 tile cannot fit
