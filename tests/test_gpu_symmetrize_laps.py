"""GPU tests of xmipp_transform_symmetrize (xh_sym.hip, Symmetrize in api.py) past the first lap of its loops and in the branches that
tests/test_gpu_symmetrize.py leaves unvisited, against the numpy fp64 restatement (tests/symmetrize_ref.py, direct coordinate form).
tests/test_symmetrize_ref.py asserts on the CPU, with R.staging_census and the restatement alone, that every case reaches the branch it
is there for, stays 1e-9 clear of the thresholds in both coordinate forms and has no voxel on a wrap edge (but for the 0.22 % of i1 under
wrap, which are compared like every other voxel: the device falls on the direct form's side). 0 voxels are left out.

  bricks    k_sy_pass_staged at MID = 36 x 44 x 41 (324 bricks, partial ones in Y and X): t stages 973 and i1 5 044 (brick, matrix) pairs
            with boxes of up to 3 360 doubles, 62 and 298 of them on partial bricks; 2 591 and 14 072 pairs gather at the border.
  matrices  scalings, an anisotropic scaling, a mirror and a shear of the generic rotation A0: boxes above SY_BOX = 5 832 (0.5 A0 and
            0.62 A0, no pair staged), the largest staged box 5 814 beside refusals of both kinds in one launch (diag(0.45, 1, 2) A0), 298 of
            324 bricks staged (1.7 A0), and a list through set_matrices with an identity entry between rotations and 0.8 A0.
  tiles     k_sy_prefilter_x with 35 rows in a tile of 64 (X = 95) and of 63 (X = 96), 78 rows in tiles of 46 (X = 131) and 6 rows in tiles
            of 5 (X = 1 024); a stack of 4 250 rows in 185 tiles of 23, the last of 18.
  laps      k_sy_images and k_sy_helical past 16 workgroups per CU, k_sy_outside_images past 65 535 images.
  refusals  every refusal of the handle, with the handle's results unchanged behind it.

Bounds, all relative to max|V_in| and none taken from the device (tests/test_symmetrize_ref.py derives and asserts each):
  R.BOUND = 1e-13          point groups (the MID cases are part of its derivation: the two coordinate forms are 4.9e-15 apart at the most),
                           the coefficients, the helix.
  R.BOUND_GENERAL = 1e-12  matrices that are no rotation and the rotation on rows of 131: the two forms are 1.1e-14 apart at (3, 26, 131)
                           and 6.9e-15 at MID (0.62 A0, splines, no wrap); 16 x rounds up to 1e-12.
  R.BOUND_IMAGES = 1e-13   stacks: the direct form is 3.0e-16 from its evaluation in np.longdouble, 16 x rounds up to 1e-14, below
                           R.BOUND, which is used.
Measured on one MI355X, largest distance to the restatement: see the docstring of each test."""
import math

import numpy as np
import pytest

from tests import symmetrize_ref as R
from tests.test_gpu_symmetrize import MODES, dev, gpu, handle, margin, ref_sum, vol  # noqa: F401

pytestmark = pytest.mark.gpu


def near(got, want, scale, bound, what):
    d = float(np.abs(got - want).max())
    print(f"{what}: largest difference {d / scale:.3e} of max|V| (bound {bound:.0e})")
    assert np.isfinite(got).all() and d <= bound * scale, what


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def cus(gpu):
    return gpu[2].cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------- bricks
@pytest.mark.parametrize("sym", R.MID_GROUPS)
@pytest.mark.parametrize("degree,wrap", MODES)
def test_point_group_with_most_bricks_interior(gpu, sym, degree, wrap):
    """t and i1 at MID, averaged; i1 with splines and no wrap also summed (compared after division by n + 1). Every voxel within R.BOUND
    of the direct form. Measured: 0 with linear interpolation (the bits of the restatement), t 1.6e-16 and i1 1.3e-16 with splines"""
    shape = R.MID
    s, mats = ref_sum(shape, sym, degree, wrap)
    h = handle(gpu, shape)
    h.set_matrices(mats)
    v = dev(gpu, vol(shape))
    scale = np.abs(vol(shape)).max()
    n1 = len(mats) + 1
    got = h.symmetrize(v, degree, wrap, False).cpu().numpy()
    near(got, s * (1.0 / float(np.float32(len(mats)) + np.float32(1.0))), scale, R.BOUND, f"{sym} {shape} degree {degree} wrap {wrap}")
    if sym == "i1" and degree == 3 and not wrap:
        got = h.symmetrize(v, degree, wrap, True).cpu().numpy()
        near(got / n1, s / n1, scale, R.BOUND, f"{sym} {shape} degree {degree} wrap {wrap} --sum")


# ---------------------------------------------------------------- matrices
@pytest.mark.parametrize("name", list(R.general_matrices()))
@pytest.mark.parametrize("degree,wrap", MODES)
def test_apply_geometry3d_of_a_general_matrix(gpu, name, degree, wrap):
    """one matrix that is no rotation at MID, outside value 0.375: every voxel within R.BOUND_GENERAL of the direct form.
    Measured: 0 with linear interpolation, 6.5e-16 at the most with splines (the shear)"""
    shape, A = R.MID, R.general_matrices()[name]
    v = vol(shape)
    assert margin(shape, (A.tobytes(),), wrap) >= 1e-9
    want = R.apply_geometry(v, A, degree, wrap, 0.375, True)
    got = handle(gpu, shape).apply_geometry3d(dev(gpu, v), A, degree, wrap, 0.375).cpu().numpy()
    if not wrap:
        assert 0 < (want == 0.375).sum() < want.size          # both the outside value and the taps are compared
    near(got, want, np.abs(v).max(), R.BOUND_GENERAL, f"applyGeometry {name} degree {degree} wrap {wrap}")


@pytest.mark.parametrize("degree,wrap", MODES)
def test_a_list_with_an_identity_entry_and_a_scaling(gpu, degree, wrap):
    """[g1, I + 5e-7, 0.8 A0, g2] through set_matrices, g1 and g2 of t: the identity shortcut in the middle of a list in both pass
    kernels, a matrix that is no rotation beside it. Averaged and summed, every voxel within R.BOUND_GENERAL of R.symmetrize_volume.
    Measured: 0 with linear interpolation, 2.2e-16 at the most with splines"""
    shape, L = R.MID, R.matrix_list()
    v = vol(shape)
    assert margin(shape, tuple(m.T.tobytes() for m in L), wrap) >= 1e-9
    s = R.symmetrize_volume(v, L, degree, wrap, True, True)
    h = handle(gpu, shape)
    h.set_matrices(L)
    got = h.symmetrize(dev(gpu, v), degree, wrap, False).cpu().numpy()
    near(got, s * (1.0 / float(np.float32(4.0) + np.float32(1.0))), np.abs(v).max(), R.BOUND_GENERAL, f"the list, degree {degree} wrap {wrap}")
    got = h.symmetrize(dev(gpu, v), degree, wrap, True).cpu().numpy()
    near(got / 5, s / 5, np.abs(v).max(), R.BOUND_GENERAL, f"the list, degree {degree} wrap {wrap} --sum")


# ---------------------------------------------------------------- tiles
@pytest.mark.parametrize("shape", list(R.TILE_SHAPES))
def test_coefficients_past_the_full_tile(gpu, shape):
    """the x prefilter where a workgroup holds fewer than 64 rows, or fewer rows than its tile: within R.BOUND of R.prefilter.
    Measured: 1.4e-15 at the most ((5, 7, 95))"""
    assert R.prefilter_tile(shape[2]) == R.TILE_SHAPES[shape]
    v = vol(shape)
    got = handle(gpu, shape).coefficients(dev(gpu, v)).cpu().numpy()
    near(got, R.prefilter(v), np.abs(v).max(), R.BOUND, f"coefficients {shape}, tile {R.TILE_SHAPES[shape]}")


def test_apply_geometry3d_reads_the_coefficients_of_a_partial_tile(gpu):
    """(3, 26, 131), the rotation A0, splines, wrap: within R.BOUND_GENERAL of the direct form (rows of 131 are part of that bound's
    derivation). Measured: 5.7e-16"""
    shape = R.TILE_APPLY
    v = vol(shape)
    assert margin(shape, (R.A0.tobytes(),), True) >= 1e-9
    want = R.apply_geometry(v, R.A0, 3, True, 0.375, True)
    got = handle(gpu, shape).apply_geometry3d(dev(gpu, v), R.A0, 3, True, 0.375).cpu().numpy()
    near(got, want, np.abs(v).max(), R.BOUND_GENERAL, f"applyGeometry {shape}")


# ---------------------------------------------------------------- stacks past the caps
_STACK = {}


def big_stack():
    if "imgs" not in _STACK:
        _STACK["imgs"] = R.big_stack()
    return _STACK["imgs"]


@pytest.mark.parametrize("degree,wrap", MODES)
def test_image_stack_past_the_grid_cap(gpu, degree, wrap):
    """17 images of 250 x 262, order 5: 1 113 500 pixels, more than the 256 . 16 . CUs threads k_sy_images is launched with; the x
    prefilter in 185 tiles of 23 rows, the last of 18. Every pixel of every image within R.BOUND_IMAGES of R.symmetrize_image, direct
    form. Measured: 0 with linear interpolation, 2.4e-16 with splines"""
    imgs = big_stack()
    n, Y, X = imgs.shape
    assert imgs.shape == R.STACK_BIG and imgs.size > 256 * 16 * cus(gpu), f"{imgs.size} pixels do not exceed the cap on {cus(gpu)} CUs"
    As = tuple(R.rotation2d_matrix(360.0 / R.STACK_ORDER * i).tobytes() for i in range(1, R.STACK_ORDER))
    assert margin((Y, X), As, wrap) >= 1e-9
    got = handle(gpu, (1, Y, X)).symmetrize_images(dev(gpu, imgs), R.STACK_ORDER, degree, wrap, False).cpu().numpy()
    worst = 0.0
    for i in range(n):
        want = R.symmetrize_image(imgs[i], R.STACK_ORDER, degree, wrap, False, True)
        d = float(np.abs(got[i] - want).max() / np.abs(imgs[i]).max())
        worst = max(worst, d)
        assert np.isfinite(got[i]).all() and d <= R.BOUND_IMAGES, (i, d)
    print(f"stack {imgs.shape} order {R.STACK_ORDER} degree {degree} wrap {wrap}: largest difference {worst:.3e} of max|I| (bound {R.BOUND_IMAGES:.0e})")


def test_more_images_than_workgroups_of_the_outside_mean(gpu):
    """65 600 images of 4 x 6, order 5, splines, no wrap: k_sy_outside_images takes a second step for images 65 535 and later, and
    k_sy_images laps. Image i is base image i % 7, so output i must have the bytes of output i % 7 (every image compared, at no cost);
    the first seven are held to the restatement at R.BOUND_IMAGES. With order 1 the output has the input's bytes.
    Measured: 4.7e-16 at the most over the seven base images"""
    n, Y, X = R.STACK_MANY
    base = R.base_images()
    assert n > 65535 and n * Y * X > 256 * 16 * cus(gpu)
    idx = np.arange(n) % R.STACK_BASE
    imgs = np.ascontiguousarray(base[idx])
    h = handle(gpu, (1, Y, X))
    got = h.symmetrize_images(dev(gpu, imgs), R.STACK_ORDER, 3, False, False).cpu().numpy()
    for i in range(R.STACK_BASE):
        want = R.symmetrize_image(base[i], R.STACK_ORDER, 3, False, False, True)
        near(got[i], want, np.abs(base[i]).max(), R.BOUND_IMAGES, f"base image {i} of {base[i].shape}")
    assert np.array_equal(got.view(np.uint64), got[:R.STACK_BASE].view(np.uint64)[idx])
    assert len({got[i].tobytes() for i in range(R.STACK_BASE)}) == R.STACK_BASE
    for degree in (1, 3):
        copy = h.symmetrize_images(dev(gpu, imgs), 1, degree, False, False).cpu().numpy()
        assert same_bytes(copy, imgs)


# ---------------------------------------------------------------- the helix past the cap
def test_helix_past_the_grid_cap(gpu):
    """25 x 206 x 204, zHelical 4.3 voxels, -41.5 degrees, phase 0.2, C2, heightFraction 0.95: 1 050 600 voxels, more than the
    256 . 16 . CUs threads k_sy_helical is launched with. Every voxel within R.BOUND of the restatement, and two runs give the same bytes.
    Not dihedral: that branch's second pass is the brick kernel, which has no lap, and its restatement costs 15 s at this size; the
    dihedral helix is compared in tests/test_gpu_symmetrize.py. Measured: 2.2e-15"""
    shape, zh, rot, phase, cn, hf = R.HELIX_LAP
    assert shape[0] * shape[1] * shape[2] > 256 * 16 * cus(gpu), f"{shape} does not exceed the cap on {cus(gpu)} CUs"
    v = vol(shape)
    stats = {}
    want = R.symmetrize_helical(v, zh, math.radians(rot), phase, False, hf, cn, 3, True, stats)
    assert np.isfinite(want).all() and stats["depth"] == 0 == gpu[0].sym_helical_depth(shape[0], zh, hf, False)
    h = handle(gpu, shape)
    d = dev(gpu, v)
    got = h.helical(d, zh, math.radians(rot), phase, cn, False, hf, 3).cpu().numpy()
    near(got, want, np.abs(v).max(), R.BOUND, f"helix {shape}")
    assert same_bytes(h.helical(d, zh, math.radians(rot), phase, cn, False, hf, 3).cpu().numpy(), got)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_as_it_was(gpu):
    """every refusal of the handle is an XhError with its reason, the list set before a refused set_matrices stays in force, and the
    handle gives the bytes it gave before"""
    xa, ctx, torch = gpu
    shape = R.SMALL[2]
    v = dev(gpu, vol(shape))
    h = xa.Symmetrize(ctx, shape)
    mats = R.group_matrices("d3")
    h.set_matrices(mats)
    before = h.symmetrize(v, 3, False, False).cpu().numpy()
    assert not same_bytes(before, vol(shape))

    def unchanged():
        assert h.n_matrices == len(mats) and same_bytes(h.symmetrize(v, 3, False, False).cpu().numpy(), before)

    bad = np.array(mats[:2])
    bad[1, 1, 2] = np.nan
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 5.0]])
    for R_, why in ((np.tile(np.eye(3) * 2.0, (1025, 1, 1)), "1025 matrices"), (bad, "not finite"), ([mats[0], singular], "singular or scales"),
                    ([mats[0], 1e-4 * np.eye(3)], "singular or scales by more than 1000")):
        with pytest.raises(xa.XhError, match=why):
            h.set_matrices(R_)
        unchanged()
    with pytest.raises(xa.XhError, match="spline order 2"):
        h.symmetrize(v, 2, False, False)
    with pytest.raises(xa.XhError, match="spline order 2"):
        h.apply_geometry3d(v, R.A0, 2, False, 0.0)
    with pytest.raises(xa.XhError, match="made for volumes"):
        h.symmetrize_images(v, 5, 3, False, False)
    for cn in (0, 100):
        with pytest.raises(xa.XhError, match=f"Cn = {cn} "):
            h.helical(v, 5.0, 0.5, 0.0, cn, False, 0.95, 3)
    for rot, phase in ((float("nan"), 0.0), (0.5, float("inf"))):
        with pytest.raises(xa.XhError, match="rotation is not finite"):
            h.helical(v, 5.0, rot, phase, 1, False, 0.95, 3)
    unchanged()
    # a handle for images
    D = 20
    imgs = dev(gpu, np.stack([R.phantom((D, D), 20 + i) for i in range(3)]))
    hi = xa.Symmetrize(ctx, (1, D, D))
    first = hi.symmetrize_images(imgs, 5, 3, False, False).cpu().numpy()
    one = imgs[:1].contiguous()
    for call in (lambda: hi.symmetrize(one, 3, False, False), lambda: hi.coefficients(one), lambda: hi.outside_mean(one),
                 lambda: hi.apply_geometry3d(one, R.A0, 3, False, 0.0), lambda: hi.helical(one, 5.0, 0.5)):
        with pytest.raises(xa.XhError, match="made for images"):
            call()
    for order in (0, 1025):
        with pytest.raises(xa.XhError, match=f"order {order} "):
            hi.symmetrize_images(imgs, order, 3, False, False)
    with pytest.raises(xa.XhError, match="spline order 2"):
        hi.symmetrize_images(imgs, 5, 2, False, False)
    assert same_bytes(hi.symmetrize_images(imgs, 5, 3, False, False).cpu().numpy(), first)
    # no handle at all
    with pytest.raises(xa.XhError, match="above 1024 are not supported"):
        xa.Symmetrize(ctx, (8, 8, 1025))
    with pytest.raises(xa.XhError, match="bad size 8 x 1 x 8"):
        xa.Symmetrize(ctx, (8, 1, 8))


@pytest.mark.parametrize("degree,wrap", MODES)
def test_an_empty_list_returns_the_input(gpu, degree, wrap):
    xa, ctx, _ = gpu
    shape = R.SMALL[2]
    h = xa.Symmetrize(ctx, shape)
    h.set_matrices(R.group_matrices("c5"))
    h.set_matrices([])
    assert h.n_matrices == 0
    for sum_ in (False, True):
        assert same_bytes(h.symmetrize(dev(gpu, vol(shape)), degree, wrap, sum_).cpu().numpy(), vol(shape))
