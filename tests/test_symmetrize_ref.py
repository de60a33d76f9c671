"""CPU checks that pin the numpy restatement of xmipp_transform_symmetrize (tests/symmetrize_ref.py) to what the project already trusts:
the oracle's 2-D applyGeometry, rotate and prefilter, the index-permutation identity of c4, the matrix counts of the groups, the helix on
a z-constant volume, and the bound of the helical interpolation's recursion. The device tolerance of tests/test_gpu_symmetrize.py is
derived here, from the restatement alone: see test_device_bound_is_derived_from_the_two_coordinate_forms."""
import math

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import symmetrize_ref as R

SHAPES2D = [(20, 20), (21, 23)]


def _img(shape, seed=1):
    return R.phantom(shape, seed)


@pytest.mark.parametrize("shape", SHAPES2D)
@pytest.mark.parametrize("degree", (1, 3))
@pytest.mark.parametrize("wrap", (True, False))
def test_apply_geometry2d_and_rotate_equal_the_oracle(shape, degree, wrap):
    """the incremental form is the oracle's own loop: equal to rounding of the library calls (1e-13 of max|I|; observed 0 to 4e-16).
    Without wrap the oracle writes 0 outside, which is the restatement's outside = 0"""
    img = _img(shape)
    tol = 1e-13 * np.abs(img).max()
    for ang in (10.0, 72.0, 137.5):
        got = R.rotate2d(img, ang, degree, wrap, 0.0, direct=False)
        want = po.rotate2d(img, ang, degree, wrap)
        assert np.abs(got - want).max() <= tol, (ang, np.abs(got - want).max())
    A = np.array([[0.9, 0.3, 0.0], [-0.2, 1.1, 0.0], [0.0, 0.0, 1.0]])
    got = R.apply_geometry(img, A, degree, wrap, 0.0, direct=False)
    want = po.apply_geometry2d(img, A, degree, False, wrap)
    assert np.abs(got - want).max() <= tol


@pytest.mark.parametrize("n", (20, 21, 70))
def test_prefilter_equals_the_oracle(n):
    img = _img((n, n))
    assert np.abs(R.prefilter(img) - po.prefilter2d(img)).max() <= 1e-13 * np.abs(img).max()


@pytest.mark.parametrize("degree", (1, 3))
@pytest.mark.parametrize("wrap", (True, False))
def test_a_z_constant_volume_turned_about_z_is_the_2d_result_in_every_slice(degree, wrap):
    img = _img((20, 22))
    vol = np.repeat(img[None], 19, axis=0)
    A = R.rotation2d_matrix(33.0)                       # about Z: the 2-D matrix with z left alone
    got = R.apply_geometry(vol, A, degree, wrap, 0.5, direct=False)
    want = R.apply_geometry(img, A, degree, wrap, 0.5, direct=False)
    # the z prefilter of a constant line returns the constant to rounding, and the four z weights sum to 1 to rounding
    assert np.abs(got - want[None]).max() <= 1e-13 * np.abs(img).max()


@pytest.mark.parametrize("shape,wrap", [((21, 21, 21), True), ((21, 21, 21), False), ((20, 20, 20), True)])
@pytest.mark.parametrize("degree", (1, 3))
def test_c4_is_the_mean_of_the_index_permuted_copies(shape, wrap, degree):
    v = R.phantom(shape, 2)
    got = R.symmetrize_volume(v, R.group_matrices("c4"), degree, wrap)
    want = c4_by_permutation(v)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(v).max()


def c4_by_permutation(v):
    """(V + its three quarter turns about Z) / 4 with no interpolation: the source of the logical point (x, y) is (-y, x), (-x, -y) and
    (y, -x). On an even box -min = max + 1 is outside and the wrap brings it to min: indices modulo n"""
    n = v.shape[1]
    assert v.shape[2] == n
    c = n // 2
    y, x = np.meshgrid(np.arange(n) - c, np.arange(n) - c, indexing="ij")
    out = v.copy()
    for sx, sy in ((-y, x), (-x, -y), (y, -x)):
        out = out + v[:, (sy + c) % n, (sx + c) % n]
    return out / 4.0


@pytest.mark.parametrize("sym,count", [("c5", 4), ("d3", 5), ("t", 11), ("o", 23), ("i1", 59)])
def test_matrix_counts(sym, count):
    M = R.group_matrices(sym)
    assert len(M) == count
    for m in M:
        assert np.abs(m @ m.T - np.eye(3)).max() < 1e-12 and not R.is_identity(m)


def test_no_group_lists_the_powers_of_each_generator_line():
    assert len(R.group_matrices("c5", no_group=True)) == 4
    assert len(R.group_matrices("d3", no_group=True)) == 2 + 1
    assert len(R.group_matrices("o", no_group=True)) == 2 + 3
    assert len(R.group_matrices("i2", no_group=True)) == 1 + 4 + 2


def test_helix_leaves_a_z_constant_volume_unchanged():
    """rotHelical = 0, Cn = 1: every term samples the same (x, y) at some kp inside the box, so the weighted mean is the value itself,
    wherever x and y stay in range: the trilinear corner x + 1 or y + 1 is never asked for at integer x, y"""
    img = _img((20, 20))
    vol = np.repeat(img[None], 24, axis=0)
    out = R.symmetry_helical(vol, 5.0, 0.0, 0.0, False, 0.95, 1)
    # cos(atan2(i, j)) rho returns j to rounding, not exactly: the corner beside an edge voxel may be outside, so the edge is left out
    inner = (slice(None), slice(1, -1), slice(1, -1))
    assert np.abs(out[inner] - vol[inner]).max() <= 1e-12 * np.abs(vol).max()


@pytest.mark.parametrize("Z", (20, 21))
def test_recursion_bound_formula(Z):
    v = R.phantom((Z, 12, 12), 3)
    seen = set()
    for zh in (1.25, 2.0, 3.7, 6.5, float(Z)):
        for hf in (0.5, 0.8, 0.95, 1.0):
            for dihedral in (False, True):
                stats = {}
                R.symmetry_helical(v, zh, 0.4, 0.1, dihedral, hf, 2, stats)
                bound = R.helical_depth(Z, zh, hf, dihedral)
                assert 0 <= bound and stats["depth"] <= bound, (zh, hf, dihedral, stats, bound)
                if dihedral and hf == 1.0 and Z % 2 == 0:
                    assert stats["depth"] == 1 == bound
                seen.add(stats["depth"])
    assert seen == ({0, 1} if Z % 2 == 0 else {0})
    for zh, hf in ((1.0, 0.95), (0.5, 0.95), (Z + 0.5, 0.95), (3.0, 1.2), (3.0, 0.0)):
        assert R.helical_depth(Z, zh, hf, True) == -1


def test_the_reference_does_not_terminate_below_one_voxel():
    v = R.phantom((20, 12, 12), 3)
    with pytest.raises(RecursionError):
        R.symmetry_helical(v, 0.75, 0.4, 0.0, True, 1.0, 1)


def test_device_bound_is_derived_from_the_two_coordinate_forms():
    """The tolerance of the device tests. For every parity case the restatement runs with the reference's incremental coordinates and with
    the direct ones the device uses; the largest difference relative to max|V_in| times 16, rounded up to a power of ten, is R.BOUND.
    Measured here: largest relative difference 4.9e-15, so 16 x gives 7.8e-14 and the bound is 1e-13.
    Precondition of every case, on both forms: no tested coordinate within 1e-9 of a threshold min - 1e-6 or max + 1e-6 (0 found).
    Under WRAP the voxels with a coordinate on a wrap edge min - 0.5 + k dim are not compared (R.wrap_edge_mask says why): the case stays,
    those voxels are counted."""
    worst, masked = 0.0, 0
    for shape, sym, degree, wrap in R.parity_cases():
        v = R.phantom(shape, 7)
        res, coords = [], []
        for direct in (False, True):
            res.append(R.symmetrize_volume(v, R.group_matrices(sym), degree, wrap, False, direct, coords))
        assert min(R.threshold_margin(shape, t) for t in coords) >= 1e-9, (shape, sym)
        keep = ~R.wrap_edge_mask(shape, coords) if wrap else np.ones(shape, dtype=bool)
        assert keep.mean() > 0.97
        masked = max(masked, int((~keep).sum()))
        worst = max(worst, np.abs(res[0] - res[1])[keep].max() / np.abs(v).max())
    print(f"largest relative difference of the two coordinate forms: {worst:.3e}; most voxels on a wrap edge in one case: {masked}")
    assert worst > 0
    assert R.BOUND == 10.0 ** math.ceil(math.log10(16 * worst))
