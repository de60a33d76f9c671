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
    Measured here: largest relative difference 4.9e-15, so 16 x gives 7.8e-14 and the bound is 1e-13; t and i1 at R.MID, which
    tests/test_gpu_symmetrize_laps.py compares, are among the cases and do not move it (144 voxels, 0.22 %, on a wrap edge for i1).
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


# ---------------------------------------------------------------- the cases of tests/test_gpu_symmetrize_laps.py
def _inverses(R_list):
    """the inverses the device forms for a list given to set_matrices, identity entries left out"""
    return [R.inv3x3(np.asarray(m).T) for m in R_list if not R.is_identity(np.asarray(m).T)]


@pytest.mark.parametrize("sym,want", [("t", {"staged": 973, "border": 2591, "over": 0, "largest": 2925, "partial": 62}),
                                      ("i1", {"staged": 5044, "border": 14072, "over": 0, "largest": 3360, "partial": 298})])
def test_point_groups_at_mid_stage_most_interior_bricks(sym, want):
    """what the MID cases are there for: oblique axes, whole source boxes in LDS, staged pairs on bricks the volume cuts. On the boxes of
    tests/test_gpu_symmetrize.py at most 141 pairs are staged"""
    got = R.staging_census(R.MID, _inverses(R.group_matrices(sym)))
    print(f"{sym} at {R.MID}: {got}")
    assert got == want
    small = max(R.staging_census(s, _inverses(R.group_matrices(g)))["staged"] for s in R.SMALL for g in R.GROUPS)
    assert small <= 141 < got["staged"]


GENERAL_CENSUS = {
    "0.5 A0": {"staged": 0, "border": 322, "over": 2, "largest": 0, "partial": 0},
    "0.62 A0": {"staged": 0, "border": 316, "over": 8, "largest": 0, "partial": 0},
    "0.8 A0": {"staged": 28, "border": 296, "over": 0, "largest": 4896, "partial": 0},
    "1.7 A0": {"staged": 298, "border": 26, "over": 0, "largest": 1331, "partial": 85},
    "diag(0.45, 1, 2) A0": {"staged": 4, "border": 296, "over": 24, "largest": 5814, "partial": 0},
    "diag(-1, 1, 1) A0": {"staged": 77, "border": 247, "over": 0, "largest": 3360, "partial": 5},
    "shear": {"staged": 128, "border": 196, "over": 0, "largest": 3136, "partial": 26},
}


def test_general_matrices_reach_the_branches_they_are_there_for():
    """every matrix that is no rotation: the census class it was chosen for, an inverse the entry points accept (entries up to 1e3), no
    source coordinate within 1e-9 of a threshold in either coordinate form (measured: 6.0e-6 at the least), and no voxel on a wrap edge,
    so that the two forms never part"""
    mats = R.general_matrices()
    assert sorted(mats) == sorted(GENERAL_CENSUS)
    for name, A in mats.items():
        Ainv = R.inv3x3(A)
        c = R.staging_census(R.MID, [Ainv])
        assert c == GENERAL_CENSUS[name], (name, c)
        assert c["staged"] + c["border"] + c["over"] == 324
        assert np.abs(Ainv).max() <= 1e3 and not R.is_identity(A)
        margins = []
        for wrap in (True, False):
            coords = [R.source_coords(R.MID, Ainv, wrap, direct)[0] for direct in (False, True)]
            margins.append(min(R.threshold_margin(R.MID, t) for t in coords))
            assert margins[-1] >= 1e-9, (name, wrap)
            assert R.threshold_margin_both_forms(R.MID, [A], wrap) == margins[-1]
            if wrap:
                assert not R.wrap_edge_mask(R.MID, coords).any(), name
        print(f"{name}: {c}, margin {min(margins):.2e}")
    for name in ("0.5 A0", "0.62 A0"):
        assert GENERAL_CENSUS[name]["over"] >= 1 and GENERAL_CENSUS[name]["staged"] == 0
    c = GENERAL_CENSUS["diag(0.45, 1, 2) A0"]
    assert c["staged"] >= 1 and c["border"] >= 1 and c["over"] >= 1 and R.SY_BOX - 18 == c["largest"]      # all three in one launch
    assert GENERAL_CENSUS["1.7 A0"]["staged"] >= 0.9 * 324
    assert GENERAL_CENSUS["0.8 A0"]["staged"] >= 1 and GENERAL_CENSUS["0.8 A0"]["largest"] > 3360          # larger than any rotation's box
    assert np.linalg.det(mats["diag(-1, 1, 1) A0"]) < -0.99 and GENERAL_CENSUS["diag(-1, 1, 1) A0"]["staged"] >= 1
    assert GENERAL_CENSUS["shear"]["staged"] >= 1 and GENERAL_CENSUS["shear"]["border"] >= 1
    # the list: the identity entry is the second of four, and the brick kernel stages beside it
    L = R.matrix_list()
    assert [R.is_identity(m.T) for m in L] == [False, True, False, False] and not np.array_equal(L[1], np.eye(3))
    c = R.staging_census(R.MID, _inverses(L))
    print(f"the list: {c}")
    assert c == {"staged": 211, "border": 761, "over": 0, "largest": 4896, "partial": 7}
    for wrap in (True, False):
        assert R.threshold_margin_both_forms(R.MID, [m.T for m in L], wrap) >= 1e-9


def test_general_bound_is_derived_from_the_two_coordinate_forms():
    """R.BOUND_GENERAL, by the rule of R.BOUND: over every single-matrix case (outside value 0.375), the list, and the rotation A0 on
    the prefilter's tile shape (3, 26, 131) (splines, wrap), the largest difference of the restatement's incremental and direct coordinate
    forms relative to max|V_in|, times 16, rounded up to a power of ten. The incremental form adds A00 along a row: an inverse that
    stretches, or a row of 131 under wrap, makes it drift further than the rotations on rows of up to 70 that R.BOUND is derived on.
    Measured here: largest relative difference 1.1e-14 (A0 at (3, 26, 131)) and 6.9e-15 at MID (0.62 A0, splines, no wrap); 16 x gives
    1.8e-13 and the bound is 1e-12. Every case is clear of the thresholds by 1e-9 in both forms
    (test_general_matrices_reach_the_branches_they_are_there_for, and here for the tile shape).
    Wrap-edge voxels would be masked here, and only here; there are none."""
    worst, where, masked = 0.0, None, 0
    cases = [(n, d, w) for n, d, w in R.general_cases()] + [("list", d, w) for d in (1, 3) for w in (True, False)] + [("tile", 3, True)]
    for name, degree, wrap in cases:
        shape = R.TILE_APPLY if name == "tile" else R.MID
        v = R.phantom(shape, 7)
        res, coords = [], []
        for direct in (False, True):
            if name == "list":
                res.append(R.symmetrize_volume(v, R.matrix_list(), degree, wrap, False, direct, coords))
            else:
                res.append(R.apply_geometry(v, R.A0 if name == "tile" else R.general_matrices()[name], degree, wrap, 0.375, direct, None, coords))
        if name == "tile":
            assert min(R.threshold_margin(shape, t) for t in coords) >= 1e-9
        keep = ~R.wrap_edge_mask(shape, coords) if wrap else np.ones(shape, dtype=bool)
        masked += int((~keep).sum())
        diff = np.abs(res[0] - res[1])[keep].max() / np.abs(v).max()
        if diff > worst:
            worst, where = diff, (name, degree, wrap)
    print(f"general matrices: largest relative difference of the two coordinate forms {worst:.3e} at {where}; voxels masked {masked}")
    assert masked == 0 and worst > 0
    assert R.BOUND_GENERAL == 10.0 ** math.ceil(math.log10(16 * worst))


def test_prefilter_tiles():
    """the x prefilter's tile: 64 rows up to X = 95, fewer from 96 on, 5 at 1024; the shapes run one short tile, two tiles with the second
    partial, and more than 32 rows in a tile (threads past the first half wave filter a row)"""
    assert all(R.prefilter_tile(X) == 64 for X in range(2, 96)) and R.prefilter_tile(96) == 63
    assert max(s[2] for s in R.SMALL + [R.BIG, R.MID]) < 96
    for shape, tr in R.TILE_SHAPES.items():
        assert R.prefilter_tile(shape[2]) == tr
    rows = {s: s[0] * s[1] for s in R.TILE_SHAPES}
    assert rows[(5, 7, 95)] == rows[(5, 7, 96)] == 35 > 32
    assert rows[(3, 26, 131)] == 78 == 46 + 32
    assert rows[(2, 3, 1024)] == 6 == 5 + 1
    n, Y, X = R.STACK_BIG
    assert R.prefilter_tile(X) == 23 and -(-n * Y // 23) == 185 and n * Y - 184 * 23 == 18


def test_stack_and_helix_sizes_pass_the_caps_of_256_compute_units():
    """the grids are capped at 16 workgroups of 256 threads per CU; an MI355X has 256 CUs. The device tests assert the same on the
    machine they run on"""
    cap = 256 * 16 * 256
    n, Y, X = R.STACK_BIG
    assert n * Y * X == 1113500 > cap
    n, Y, X = R.STACK_MANY
    assert n > 65535 and n * Y * X > cap and n * Y * X <= 2 ** 31
    shape, zh, rot, phase, cn, hf = R.HELIX_LAP
    assert shape[0] * shape[1] * shape[2] == 1050600 > cap
    assert R.helical_depth(shape[0], zh, hf, False) == 0


def test_image_bound_is_derived_in_higher_precision():
    """R.BOUND_IMAGES. At 250 x 262 the incremental form is no yardstick: it adds A00 262 times along a row and is 1.6e-14 from the direct
    form already at 97 x 96. The direct form (what the device computes) is instead held against R.symmetrize_image_exact: the same float64
    coordinates, truncations and tap indices, the weights, coefficients, outside mean and sums in np.longdouble. 16 times the largest
    distance relative to max|I|, rounded up to a power of ten, or R.BOUND where that is smaller. Over three images of the large stack in
    every mode and the seven 4 x 6 base images (splines, no wrap, the mode they run in).
    Measured here: 3.0e-16 at the most (a 4 x 6 image), so 16 x rounds up to 1e-14, below R.BOUND = 1e-13, which is the bound."""
    assert np.finfo(np.longdouble).nmant >= 63
    worst, where = 0.0, None
    big, base = R.big_stack()[:3], R.base_images()
    cases = [(img, d, w, "250 x 262") for img in big for d in (1, 3) for w in (True, False)] + [(img, 3, False, "4 x 6") for img in base]
    for img, degree, wrap, what in cases:
        want = R.symmetrize_image_exact(img, R.STACK_ORDER, degree, wrap)
        got = R.symmetrize_image(img, R.STACK_ORDER, degree, wrap, False, True)
        diff = float(np.abs(got - want).max() / np.abs(img).max())
        if diff > worst:
            worst, where = diff, (what, degree, wrap)
    derived = 10.0 ** math.ceil(math.log10(16 * worst))
    print(f"images: largest relative distance of the direct form to the higher-precision evaluation {worst:.3e} at {where}; "
          f"16 x rounds up to {derived:.0e}, R.BOUND is {R.BOUND:.0e}")
    assert worst > 0
    assert R.BOUND_IMAGES == max(derived, R.BOUND)


def test_stack_cases_are_clear_of_thresholds_and_wrap_edges():
    """order 5 on 250 x 262 and on 4 x 6: no source coordinate within 1e-9 of a threshold in either coordinate form, none on a wrap
    edge in the direct form the device is compared on; the base images are positive and all different"""
    As = [R.rotation2d_matrix(360.0 / R.STACK_ORDER * i) for i in range(1, R.STACK_ORDER)]
    for shape, wraps in ((R.STACK_BIG[1:], (True, False)), (R.STACK_MANY[1:], (False,))):
        for wrap in wraps:
            m = R.threshold_margin_both_forms(shape, As, wrap)
            print(f"stack {shape} wrap {wrap}: margin {m:.2e}")
            assert m >= 1e-9
            if wrap:
                coords = [R.source_coords(shape, R.inv3x3(A), True, True)[0] for A in As]
                assert not R.wrap_edge_mask(shape, coords).any()
    base = R.base_images()
    assert base.min() > 0 and len({b.tobytes() for b in base}) == R.STACK_BASE
    out = [R.source_coords(R.STACK_MANY[1:], R.inv3x3(A), False, True)[2] for A in As]
    assert any(o.any() for o in out) and not all(o.all() for o in out)          # the outside mean is used, and so are the taps
