"""The shapes of tests/subtract_shapes.py reach the loop laps, workgroup counts and chunks they are listed for (no device needed: the
restatement of the lengths and launch sizes of xh_sub.hip and xh_rsp.hip against the property each shape is there for)."""
import numpy as np

from tests import subtract_projection_ref as R
from tests import subtract_shapes as S


def test_shapes_reach_their_paths():
    S.check_reach()


def test_22_is_the_smallest_size_with_a_second_lap_of_the_model_loop():
    first = next(D for D in range(4, 64) if S.half_cells(D) > S.THREADS)
    assert first == S.LAP_MODELS == 22
    assert S.laps(S.half_cells(22)) == (2, 8)
    assert S.laps(S.half_cells(40)) == (4, 72) and S.laps(S.full_cells(40)) == (7, 64)


def test_168_has_a_bin_past_one_lap_and_160_has_none():
    cells = S.bin_cells(S.BIN)
    wi, maxwi = R.freq_map(S.BIN)
    assert len(cells) == maxwi + 1 and cells.sum() == ((wi > 0) & (wi < maxwi)).sum()
    assert cells.max() == 269 > S.THREADS
    assert S.bin_cells(S.BIN_BELOW).max() <= S.THREADS
    # counted by hand at a small size: wi of D = 4 is [[0 1 2] [1 1 2] [2 2 3] [1 1 2]], maxwi = round(4 / sqrt 2) = 3
    assert np.array_equal(S.bin_cells(4), [0, 5, 5, 0])


def test_65_particles_need_two_fit_blocks():
    assert S.fit_blocks(S.CHUNK_M) == 2 and S.fit_blocks(S.CHUNK_M - 1) == 1
    assert S.translate_blocks(S.CHUNK_M, 16) == 17


def test_4099_projections_need_two_chunks_with_a_seam_between_two_orientations():
    assert S.rsp_chunks(S.RSP_N) == [S.RSP_CHUNK, 3]
    rows, ang = S.rsp_rows(), S.rsp_angles()
    assert (rows[4095], rows[4096]) == (3, 4) and ang[3] != ang[4]
    assert S.rsp_blocks(S.RSP_CHUNK, S.RSP_D) == 4096


def test_padded_sizes():
    assert [S.padded(D) for D in (16, 17, 22, 40, 41)] == [31, 33, 43, 79, 81]
    assert S.padded(168, 1.0) == 168
    assert S.factors(81) == [3, 3, 3, 3] and S.factors(79) == [79] and S.factors(33) == [3, 11]
