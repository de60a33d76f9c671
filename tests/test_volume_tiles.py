"""The shapes of tests/volume_tiles.py reach the tiles they are listed for (no device needed: the restatement of the constructors' tile
choices against the property each shape is there for), and the rolls of T.ROLLS put compared voxels where the device tests need them."""
import numpy as np
import pytest

from tests import local_sharpening_ref as R
from tests import volume_tiles as T


def test_shapes_reach_their_tiles():
    T.check_reach()


def test_compared_voxels_counts_slots_and_tail():
    """ldb_compared on a hand-made inside set: (21, 19, 160) has rpb = 6 and 960 outputs per workgroup, 399 = 66 * 6 + 3 rows"""
    inside = np.zeros(T.X160, bool)
    inside[0, 0, 0] = True               # row 0, q = 0: slot 0
    inside[0, 1, 100] = True             # row 1, q = 260: slot 1
    inside[0, 5, 159] = True             # row 5, q = 959: slot 3
    inside[20, 18, 7] = True             # row 398 = 66 * 6 + 2, q = 327: slot 1, in the tail workgroup
    assert T.ldb_compared(T.X160, inside) == ([1, 2, 0, 1], 1)
    assert T.ldb_compared((24, 20, 18), np.ones((24, 20, 18), bool)) == ([24 * 20 * 18], None)


@pytest.mark.parametrize("shape", list(T.ROLLS))
def test_rolls_put_the_inside_set_into_the_tail_and_every_slot(shape):
    _, rm = R.synth(shape, 7)
    per_slot, tail = T.ldb_compared(shape, rm >= 2.0)
    assert tail == 0, "as synthesised the tail rows hold no compared voxel: that is what the roll is for"
    per_slot, tail = T.ldb_compared(shape, np.roll(rm, T.ROLLS[shape], axis=(0, 1, 2)) >= 2.0)
    assert tail > 0 and all(c > 0 for c in per_slot) and len(per_slot) == T.slots(shape)
