"""CPU checks of the restatement of xmipp_reconstruct_wbp (tests/reconstruct_wbp_ref.py): against itself, against exact sums, against the
pieces the tree already pins, and the preconditions of every GPU case (tests/test_gpu_reconstruct_wbp.py). The bound of the GPU tests is
derived here, from the restatement alone."""
import math

import numpy as np
import pytest

from tests import reconstruct_wbp_ref as R
from tests import symmetrize_ref as S

CASES = R.cases()
BOUND = 1e-14          # what test_bound_is_derived_from_exact_sums derives; tests/test_gpu_reconstruct_wbp.py holds the device to it


def test_sinc_table_reading():
    """Tabsinc(0.0001, D): (int)(D / 0.0001) entries of sinc(n * 0.0001), sinc(0) = 1"""
    t = R.sinc_table(16)
    assert len(t) == int(16 / 0.0001) and t[0] == 1.0
    for n in (1, 5000, 10000, 25000, 159999):
        x = n * 0.0001
        assert abs(t[n] - math.sin(math.pi * x) / (math.pi * x)) <= 4e-16
    assert abs(t[10000]) < 1e-15 and t[5000] == pytest.approx(2 / math.pi, rel=1e-15)


def test_transform_reading():
    """the complete transform times 1 / D^2 with DC at the logical origin; the inverse reads columns 0 .. D / 2 and is real"""
    rng = np.random.default_rng(3)
    for D in (16, 17):
        P = rng.standard_normal((D, D))
        F = R.forward(P)
        assert F[D // 2, D // 2] == pytest.approx(P.mean(), rel=1e-13)
        i, j = 3, -2
        want = sum(P[y, x] * np.exp(-2j * math.pi * (i * y + j * x) / D) for y in range(D) for x in range(D)) / (D * D)
        assert abs(F[i + D // 2, j + D // 2] - want) < 1e-14
        assert np.abs(R.inverse(F) - P).max() < 1e-13
        # what lies right of column D / 2 of the uncentred array is never read
        G = np.roll(F, (-(D // 2), -(D // 2)), axis=(0, 1))
        G[:, D // 2 + 1:] = 7.0
        assert np.array_equal(R.inverse(np.roll(G, (D // 2, D // 2), axis=(0, 1))), R.inverse(F))
        for exact in (False, True):
            assert np.abs(R.inverse(R.forward(P, exact), exact) - P).max() < 1e-13


def test_shift_and_flip_reading():
    """:552-554 as read here: A = (shifts in column 2, a flip negates A00 and A01) applied as IS_INV, so out(x, y) = in(+-x + shiftX, y + shiftY):
    the content moves by MINUS the shifts, the opposite of readApplyGeo's IS_NOT_INV with the same matrix"""
    D = 16
    img = np.zeros((D, D))
    img[D // 2 + 2, D // 2 + 3] = 1.0                                   # logical (y, x) = (2, 3)
    out = R.prepare(img, 2.0, 1.0, False, 1.0)
    assert np.unravel_index(np.argmax(out), out.shape) == (D // 2 + 1, D // 2 + 1)       # x + 2 = 3, y + 1 = 2
    assert out.max() == pytest.approx(1.0, abs=1e-12)
    out = R.prepare(img, 2.0, 1.0, True, 1.0)
    assert np.unravel_index(np.argmax(out), out.shape) == (D // 2 + 1, D // 2 - 1)       # -x + 2 = 3
    assert np.array_equal(R.prepare(img, 0.0, 0.0, False, 3.0), 3.0 * img)                # the identity copies
    assert np.array_equal(R.prepare(img, 5e-7, 0.0, False, 1.0), img)                     # isIdentity's 1e-6
    # a shift of D wraps onto the image itself
    rng = np.random.default_rng(5)
    img = rng.standard_normal((D, D))
    assert np.abs(R.prepare(img, float(D), 0.0, False, 1.0) - img).max() < 1e-12


def test_prepare_is_the_pinned_apply_geometry():
    """IS_INV with A is IS_NOT_INV with inv(A): the 2-D applyGeometry that tests/test_symmetrize_ref.py pins to the oracle"""
    rng = np.random.default_rng(7)
    img = rng.standard_normal((17, 17))
    for sx, sy, flip in ((1.25, -2.5, False), (0.75, 3.125, True), (20.5, -19.25, False)):
        A = R.geometry_matrix(sx, sy, flip)
        Ainv = np.array([[A[0, 0], 0.0, -A[0, 0] * sx], [0.0, 1.0, -sy], [0.0, 0.0, 1.0]])          # exact for these entries
        assert np.array_equal(S.inv3x3(Ainv), A)
        want = S.apply_geometry(img, Ainv, 3, True, direct=False)
        assert np.array_equal(R.prepare(img, sx, sy, flip, 1.0), want)


def test_directions_of_each_image():
    angles = [(10.0, 20.0, 30.0), (200.0, 95.0, -40.0)]
    Rm = S.group_matrices("c3")
    g, tot = R.all_matrices(angles, None, Rm)
    assert g.shape == (6, 4) and tot == 6.0
    for n, (rot, tilt, psi) in enumerate(angles):
        E = np.array(R.euler_matrix(rot, -tilt, psi))
        assert np.array_equal(g[3 * n, :3], E[2])
        for i in range(2):
            assert np.allclose(g[3 * n + 1 + i, :3], (E @ Rm[i])[2], atol=1e-15)
            assert abs(np.linalg.norm(g[3 * n + 1 + i, :3]) - 1) < 1e-15
    g, tot = R.all_matrices(angles, [0.5, 3.0], Rm)
    assert tot == 10.5 and list(g[:, 3]) == [0.5] * 3 + [3.0] * 3


def test_weight_symmetry_is_exact():
    """weight(-i, -j) == weight(i, j) bit for bit, which the filter kernel relies on; the unpaired row and column of an even D differ"""
    for case in (CASES[0], CASES[1]):
        D = case["D"]
        F, _ = R.image_matrices(*case["angles"][0])
        w = R.weights_of(R.filter_terms(D, F, case["g"], case["diameter"])[0])
        lo = 1 if D % 2 == 0 else 0
        inner = w[lo:, lo:]
        assert np.array_equal(inner, inner[::-1, ::-1])
        if D % 2 == 0:
            assert not np.array_equal(w[0, 1:], w[0, :0:-1])


def test_backprojection_row_quirk_and_cuts():
    """l and scaley come from the row's first voxel (:406-412): on an image whose value is its row index, every voxel of a volume row
    gets the row-start yp, whatever its own yp would be. The sphere of radius 5 on 20 voxels holds 515 voxels"""
    case = CASES[2]
    D = case["D"]
    _, B = R.image_matrices(*case["angles"][0])
    img = np.repeat(np.arange(D, dtype=np.float64)[:, None], D, axis=1)
    terms, keep = R.backprojection_terms(img, B, 10)
    l = np.arange(D, dtype=np.float64) - D // 2
    k, i, j = np.meshgrid(l, l, l, indexing="ij")
    assert int(((k * k + i * i) + j * j <= 25.0).sum()) == 515 and keep.sum() <= 515 and keep.any()
    dim2 = float(D // 2)
    seen = 0
    for i in range(D):
        for j in range(D):
            ks = np.flatnonzero(keep[i, j])
            if len(ks) < 2:
                continue
            z, y = -i + dim2, j - dim2
            yp0 = (0 - dim2) * B[0, 1] + y * B[1, 1] + (z * B[2, 1] + dim2)
            assert np.abs(terms[i, j, ks] - yp0).max() < 1e-12
            assert abs(B[0, 1]) * (ks[-1] - ks[0]) > 1e-3                     # the voxels' own yp would differ by far more
            seen += 1
    assert seen > 20


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_preconditions(case):
    """conditions, not measurements: 0 cells and 0 voxels have to be left out of a comparison"""
    col = {}
    V, F, count, kept = R.reconstruct(case, collect=col)
    assert R.excluded(col, case["threshold"], case["D"]) == {"threshold": 0, "index": 0, "taps": 0, "radius": 0, "wrap": 0}
    # the device's coordinate form (direct for the image and the symmetry copies) decides every cut and branch alike
    Vd, Fd, countd, keptd = R.reconstruct(case, direct=True)
    assert countd == count and np.array_equal(keptd, kept)
    want = R.result(case)
    assert np.array_equal(want[0], V) and want[2] == count
    if "threshold" in case["name"]:
        assert count > 0


def test_bound_is_derived_from_exact_sums():
    """16 times the largest relative difference between the restatement and the same per-term values summed exactly, up to a power of ten"""
    worst = 0.0
    for case in CASES:
        V, F, count, _ = R.result(case)
        Ve, Fe, counte, _ = R.reconstruct(case, exact=True)
        assert counte == count
        dv, df = R.distance(V, Ve), R.distance(F, Fe)
        print(f"{case['name']}: volume {dv:.2e}, filtered images {df:.2e}")
        worst = max(worst, dv, df)
    derived = 10.0 ** math.ceil(math.log10(16 * worst))
    print(f"largest {worst:.2e}, bound {derived:g}")
    assert derived == BOUND


def test_direct_backprojection_would_miss_the_bound():
    """why the device carries xp along the row: x a00 + y a10 + xpz formed directly moves a volume by more than the bound"""
    case = CASES[4]
    _, F, _, _ = R.result(case)
    _, B = R.image_matrices(*case["angles"][0])
    a, _ = R.backprojection_terms(F[0], B, case["diameter"], False)
    b, _ = R.backprojection_terms(F[0], B, case["diameter"], True)
    assert R.distance(b, a) > BOUND
