"""GPU parity of xmipp_transform_symmetrize (xh_sym_*, Symmetrize in api.py) against the numpy fp64 restatement
(tests/symmetrize_ref.py, direct coordinate form): the spline coefficients, a single applyGeometry, the point-group pass, --no_group, the
outside mean, the c4 permutation identity, image stacks, the helix, run-to-run identity and the program end to end.

Boxes, Z x Y x X: 20^3, 21^3, 18 x 20 x 23 (every side different: a brick grid with remainders on every axis) and 66 x 70 x 68 with c5
(past 64 a side: the prefilter's truncated start, more than one lap of the grid-stride loops, bricks inside and on the border).

Bound: R.BOUND = 1e-13 of max|V_in|. It is not taken from the device: tests/test_symmetrize_ref.py derives it as 16 times the largest
relative difference (4.9e-15) between the restatement's incremental and direct coordinate forms over every point-group case here, rounded
up to a power of ten. Every case first asserts, on the restatement alone, that no source coordinate of any matrix, in either coordinate
form, lies within 1e-9 of a threshold min - 1e-6 or max + 1e-6 (0 found, no case left out). Every voxel of every case is compared. That
includes the voxels whose coordinate sits exactly on a wrap edge max + 0.5 (the icosahedral group on even boxes), where the restatement's
two forms part (R.wrap_edge_mask, used in the CPU derivation only): the device forms its coordinates, the inverse and realWRAP with the
operations of the direct form, so it must fall on the direct form's side, and the `>` against `>=` at max + 0.5, the (int) truncation at
min - 0.5 and m2 >= dim -> 0 are what these voxels check. A run with --sum is compared after division by n + 1 (by the order for
stacks), which is the averaged output the bound was derived on. The stacks have no second launch chunk: one grid-stride launch.
Outside mean: 1e-13 relative (positive data). Files: the output is float32, so half an ulp of it (6e-8 of the largest value) is added."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import symmetrize_ref as R
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_transform_symmetrize")
SHAPES = R.SMALL + [R.BIG]
MODES = [(d, w) for d in (1, 3) for w in (True, False)]
# a rotation with no special entries: Euler-like product about three axes
_A = R._mul(R._rot_axis(0.7, 0.2, -0.5, 1.0), R._rot_axis(-1.9, 1.0, 0.3, 0.1))


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_VOL, _SUM, _HANDLES = {}, {}, {}


def vol(shape):
    if shape not in _VOL:
        _VOL[shape] = R.phantom(shape, 7)
    return _VOL[shape]


def handle(gpu, shape):
    xa, ctx, _ = gpu
    if shape not in _HANDLES:
        _HANDLES[shape] = xa.Symmetrize(ctx, shape)
    return _HANDLES[shape]


def dev(gpu, a):
    return gpu[2].from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def ref_sum(shape, sym, degree, wrap, no_group=False):
    """(the unscaled sum, the matrices) of a point-group case, computed once"""
    key = (shape, sym, degree, wrap, no_group)
    if key not in _SUM:
        mats = R.group_matrices(sym, no_group)
        assert margin(shape, tuple(m.T.tobytes() for m in mats), wrap) >= 1e-9, key
        _SUM[key] = (R.symmetrize_volume(vol(shape), mats, degree, wrap, True, True), mats)
    return _SUM[key]


_MARGIN = {}


def margin(shape, As, wrap):
    """the smallest distance of a source coordinate to a threshold, over the matrices (their bytes) and both coordinate forms"""
    key = (shape, As, wrap)
    if key not in _MARGIN:
        _MARGIN[key] = R.threshold_margin_both_forms(shape, [np.frombuffer(a).reshape(3, 3) for a in As], wrap)
    return _MARGIN[key]


def close(got, want, scale, what=""):
    d = np.abs(got - want)
    print(f"{what}: largest difference {d.max() / scale:.3e} of max|V| (bound {R.BOUND:.0e})")
    assert d.max() <= R.BOUND * scale, what


@pytest.mark.parametrize("shape", SHAPES)
def test_coefficients(gpu, shape):
    v = vol(shape)
    got = handle(gpu, shape).coefficients(dev(gpu, v)).cpu().numpy()
    close(got, R.prefilter(v), np.abs(v).max(), f"coefficients {shape}")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("degree,wrap", MODES)
def test_apply_geometry3d(gpu, shape, degree, wrap):
    v = vol(shape)
    assert margin(shape, (_A.tobytes(),), wrap) >= 1e-9
    want = R.apply_geometry(v, _A, degree, wrap, 0.375, True)
    got = handle(gpu, shape).apply_geometry3d(dev(gpu, v), _A, degree, wrap, 0.375).cpu().numpy()
    close(got, want, np.abs(v).max(), f"applyGeometry {shape} degree {degree} wrap {wrap}")


def test_apply_geometry3d_identity_copies(gpu):
    v = vol(R.SMALL[2])
    got = handle(gpu, R.SMALL[2]).apply_geometry3d(dev(gpu, v), np.eye(3) + 1e-7, 3, False, 9.0).cpu().numpy()
    assert np.array_equal(got, v)


@pytest.mark.parametrize("shape,sym", [(s, g) for s in R.SMALL for g in R.GROUPS] + [(R.BIG, "c5")])
@pytest.mark.parametrize("degree,wrap", MODES)
def test_point_group(gpu, shape, sym, degree, wrap):
    s, mats = ref_sum(shape, sym, degree, wrap)
    h = handle(gpu, shape)
    h.set_matrices(mats)
    v = dev(gpu, vol(shape))
    scale = np.abs(vol(shape)).max()
    for sum_ in ((True, False) if shape != R.BIG else (False,)):
        got = h.symmetrize(v, degree, wrap, sum_).cpu().numpy()
        want = s if sum_ else s * (1.0 / float(np.float32(len(mats)) + np.float32(1.0)))
        if sum_:
            got, want = got / (len(mats) + 1), want / (len(mats) + 1)
        close(got, want, scale, f"{sym} {shape} degree {degree} wrap {wrap} sum {sum_}")


@pytest.mark.parametrize("degree,wrap", MODES)
def test_no_group(gpu, degree, wrap):
    shape = R.SMALL[1]
    s, mats = ref_sum(shape, "d3", degree, wrap, True)
    assert len(mats) == 3
    h = handle(gpu, shape)
    h.set_matrices(mats)
    got = h.symmetrize(dev(gpu, vol(shape)), degree, wrap, False).cpu().numpy()
    close(got, s * (1.0 / float(np.float32(4.0))), np.abs(vol(shape)).max(), f"--no_group d3 degree {degree} wrap {wrap}")


@pytest.mark.parametrize("shape", SHAPES)
def test_outside_mean(gpu, shape):
    v = vol(shape)
    assert v.min() > 0                                   # nothing cancels: a relative bound means something
    got, want = handle(gpu, shape).outside_mean(dev(gpu, v)), R.outside_mean(v)
    print(f"outside mean {shape}: {abs(got - want) / want:.3e} relative")
    assert abs(got - want) <= 1e-13 * want


@pytest.mark.parametrize("shape,wrap", [((21, 21, 21), True), ((21, 21, 21), False), ((20, 20, 20), True)])
@pytest.mark.parametrize("degree", (1, 3))
def test_c4_is_the_mean_of_the_index_permuted_copies(gpu, shape, wrap, degree):
    from tests.test_symmetrize_ref import c4_by_permutation
    v = vol(shape)
    h = handle(gpu, shape)
    h.set_matrices(R.group_matrices("c4"))
    got = h.symmetrize(dev(gpu, v), degree, wrap, False).cpu().numpy()
    assert np.abs(got - c4_by_permutation(v)).max() <= 1e-12 * np.abs(v).max()


@pytest.mark.parametrize("D", (20, 33))
@pytest.mark.parametrize("order", (2, 5, 6))
@pytest.mark.parametrize("degree,wrap", MODES)
def test_image_stack(gpu, D, order, degree, wrap):
    xa, ctx, _ = gpu
    imgs = np.stack([R.phantom((D, D), 20 + i) for i in range(3)])
    h = handle(gpu, (1, D, D))
    As = [R.rotation2d_matrix(360.0 / order * i) for i in range(1, order)]
    assert R.threshold_margin_both_forms((D, D), As, wrap) >= 1e-9
    for sum_ in (False, True):
        got = h.symmetrize_images(dev(gpu, imgs), order, degree, wrap, sum_).cpu().numpy()
        for i in range(3):
            want = R.symmetrize_image(imgs[i], order, degree, wrap, sum_, True)
            div = order if sum_ else 1
            close(got[i] / div, want / div, np.abs(imgs[i]).max(), f"stack D {D} order {order} degree {degree} wrap {wrap} sum {sum_} image {i}")


HELIX_SHAPES = [(24, 20, 20), (33, 33, 33)]
# (zHelical in voxels, rotHelical in degrees): 5 A at 1 A / px, and 7.31 A at 1.7 A / px = 4.3 voxels
PITCHES = [(5.0, 27.0), (7.31 / 1.7, -41.5)]


@pytest.mark.parametrize("shape", HELIX_SHAPES)
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("cn", (1, 3))
@pytest.mark.parametrize("dihedral", (False, True))
@pytest.mark.parametrize("hf", (0.95, 1.0))
def test_helix(gpu, shape, pitch, cn, dihedral, hf):
    xa = gpu[0]
    zh, rot = pitch[0], math.radians(pitch[1])
    v = vol(shape)
    stats = {}
    want = R.symmetrize_helical(v, zh, rot, 0.2, dihedral, hf, cn, 3, True, stats)
    assert np.isfinite(want).all()
    depth = xa.sym_helical_depth(shape[0], zh, hf, dihedral)
    assert depth == R.helical_depth(shape[0], zh, hf, dihedral) and stats["depth"] <= depth
    if dihedral and hf == 1.0 and shape[0] % 2 == 0:
        assert stats["depth"] == 1                        # the recursion's second level runs
    got = handle(gpu, shape).helical(dev(gpu, v), zh, rot, 0.2, cn, dihedral, hf, 3).cpu().numpy()
    close(got, want, np.abs(v).max(), f"helix {shape} zHelical {zh:.3f} Cn {cn} dihedral {dihedral} hf {hf}")


def test_helix_refusals(gpu):
    xa = gpu[0]
    h = handle(gpu, (24, 20, 20))
    v = dev(gpu, vol((24, 20, 20)))
    for zh, hf in ((1.0, 0.95), (0.4, 0.95), (24.5, 0.95), (5.0, 1.1)):
        with pytest.raises(xa.XhError, match="recursion"):
            h.helical(v, zh, 0.3, 0.0, 1, True, hf, 3)


def test_two_runs_give_the_same_bytes(gpu):
    shape = R.SMALL[2]
    h = handle(gpu, shape)
    h.set_matrices(R.group_matrices("o"))
    v = dev(gpu, vol(shape))
    a, b = h.symmetrize(v, 3, False, False).cpu().numpy(), h.symmetrize(v, 3, False, False).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    assert h.outside_mean(v) == h.outside_mean(v)
    hv = dev(gpu, vol((24, 20, 20)))
    hh = handle(gpu, (24, 20, 20))
    a, b = hh.helical(hv, 5.0, 0.5, 0.0, 3, True, 1.0, 3).cpu().numpy(), hh.helical(hv, 5.0, 0.5, 0.0, 3, True, 1.0, 3).cpu().numpy()
    assert a.tobytes() == b.tobytes()


def test_stage_times(gpu):
    shape = R.SMALL[0]
    h = handle(gpu, shape)
    h.set_matrices(R.group_matrices("c5"))
    h.set_timing(True)
    h.symmetrize(dev(gpu, vol(shape)), 3, False, False)
    ms = h.stage_ms()
    h.set_timing(False)
    assert list(ms) == ["coefficients", "outside_mean", "pass"] and all(t > 0 for t in ms.values())


# ---------------------------------------------------------------- the program on files
def run(*args):
    return subprocess.run([PROG] + [str(a) for a in args], capture_output=True, text=True)


def file_close(got, want, vmax):
    d = np.abs(got - want)
    assert d.max() <= 6e-8 * np.abs(want).max() + R.BOUND * vmax


def test_program_on_files(gpu, tmp_path):
    shape = (21, 21, 21)
    v, v2 = vol(shape), R.phantom(shape, 31)
    s, mats = ref_sum(shape, "c5", 3, False)
    want = s * (1.0 / float(np.float32(5.0)))
    # a volume with -o
    xmipp_io.write_volume(tmp_path / "a.vol", v)
    r = run("-i", tmp_path / "a.vol", "-o", tmp_path / "b.vol", "--sym", "c5", "--dont_wrap")
    assert r.returncode == 0, r.stderr
    file_close(xmipp_io.read_volume(tmp_path / "b.vol"), want, np.abs(v).max())
    assert np.array_equal(xmipp_io.read_volume(tmp_path / "a.vol"), v.astype(np.float32))
    # in place
    r = run("-i", tmp_path / "a.vol", "--sym", "c5", "--dont_wrap", "-v", 0)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    file_close(xmipp_io.read_volume(tmp_path / "a.vol"), want, np.abs(v).max())
    # a metadata of two volumes, in place, linear, summed
    xmipp_io.write_volume(tmp_path / "c.vol", v)
    xmipp_io.write_volume(tmp_path / "d.vol", v2)
    xmipp_io.write_xmd(tmp_path / "vols.xmd", [("noname", ["image"], [[str(tmp_path / "c.vol")], [str(tmp_path / "d.vol")]])])
    r = run("-i", tmp_path / "vols.xmd", "--sym", "d3", "--spline", 1, "--dont_wrap", "--sum")
    assert r.returncode == 0, r.stderr
    for name, src in (("c.vol", v), ("d.vol", v2)):
        w = R.symmetrize_volume(src, R.group_matrices("d3"), 1, False, True, True)
        file_close(xmipp_io.read_volume(tmp_path / name), w, np.abs(src).max() * 6)
    # --no_group through the program's own SymList: d3's two generator lines give 2 + 1 matrices
    s3, mats3 = ref_sum(shape, "d3", 3, False, True)
    xmipp_io.write_volume(tmp_path / "e.vol", v)
    r = run("-i", tmp_path / "e.vol", "--sym", "d3", "--no_group", "--dont_wrap")
    assert r.returncode == 0, r.stderr
    file_close(xmipp_io.read_volume(tmp_path / "e.vol"), s3 * (1.0 / float(np.float32(4.0))), np.abs(v).max())
    # a stack, to a new stack and in place
    imgs = np.stack([R.phantom((20, 20), 40 + i) for i in range(3)])
    xmipp_io.write_stack(tmp_path / "s.stk", imgs)
    wants = [R.symmetrize_image(imgs[i], 5, 3, False, False, True) for i in range(3)]
    r = run("-i", tmp_path / "s.stk", "-o", tmp_path / "t.stk", "--sym", 5, "--dont_wrap")
    assert r.returncode == 0, r.stderr
    out = xmipp_io.read_stack(tmp_path / "t.stk")
    for i in range(3):
        file_close(out[i], wants[i], np.abs(imgs[i]).max())
    assert len(xmipp_io.read_xmd(tmp_path / "t.xmd")[1]) == 3
    r = run("-i", tmp_path / "s.stk", "--sym", 5, "--dont_wrap")
    assert r.returncode == 0, r.stderr
    out = xmipp_io.read_stack(tmp_path / "s.stk")
    for i in range(3):
        file_close(out[i], wants[i], np.abs(imgs[i]).max())
    # the helix through the program: degrees and Angstroms on the command line
    hv = vol((24, 20, 20))
    xmipp_io.write_volume(tmp_path / "h.vol", hv)
    r = run("-i", tmp_path / "h.vol", "--sym", "helicalDihedral", "--sym2", "c3", "--helixParams", 7.31, -41.5, 11.0, "--sampling", 1.7, "--heightFraction", 1.0)
    assert r.returncode == 0, r.stderr
    w = R.symmetrize_helical(hv, 7.31 / 1.7, math.radians(-41.5), math.radians(11.0), True, 1.0, 3, 3, True)
    file_close(xmipp_io.read_volume(tmp_path / "h.vol"), w, np.abs(hv).max())
