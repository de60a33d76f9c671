"""Host-side checks of xmipp_subtract_projection (usage, refusals), of its fit, model choice and frequency map, and of the real-space
ray projector's surroundings: the ABI is declared and exported, and the numpy restatement that the GPU tests compare against (tests/subtract_projection_ref.py) is itself held to a scalar transliteration of projectVolume
(reference libraries/data/projection.cpp:337-589) and meets, alone, the condition the GPU tests put on their inputs."""
import math
import os

import numpy as np
import pytest

from tests import subtract_projection_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_is_declared_exported_and_bound():
    import xmipp3_amd as xa
    from xmipp3_amd import _lib
    names = ["xh_rsp_create", "xh_rsp_destroy", "xh_rsp_info", "xh_rsp_project", "xh_rsp_steps", "xh_sub_defaults", "xh_sub_freq_map", "xh_sub_fit",
             "xh_sub_choose", "xh_sub_create", "xh_sub_destroy", "xh_sub_info", "xh_sub_load", "xh_sub_run", "xh_sub_last"]
    header = open(os.path.join(ROOT, "include", "xmipp_hip.h")).read()
    L = xa.lib()
    for n in names:
        assert n in _lib.SIGNATURES and f" {n}(" in header
        assert getattr(L, n) is not None
    assert xa.RealSpaceProjector.MODES == {"value": 0, "support": 1}


def _scalar_project_volume(V, E, offset):
    """projectVolume line by line, one ray at a time, one running ray_sum per pixel"""
    D = V.shape[0]
    x_0 = y_0 = z_0 = -(D // 2)
    x_F = y_F = z_F = x_0 + D - 1
    step = 1.0 / 3.0
    direction = [float(E[2][0]), float(E[2][1]), float(E[2][2])]
    for c in range(3):
        if direction[c] == 0:
            direction[c] = 1e-6
    sign = [1 if c >= 0 else -1 for c in direction]
    half = [0.5 * s for s in sign]
    inv = [1.0 / c for c in direction]
    eulert = [[float(E[c][r]) for c in range(3)] for r in range(3)]
    P = np.zeros((D, D))

    def rnd(x):
        return int(x + 0.5) if x > 0 else int(x - 0.5)

    def clip(x, a, b):
        return a if x < a else (b if x > b else x)

    for i in range(y_0, y_F + 1):
        for j in range(x_0, x_F + 1):
            ray_sum = 0.0
            for ray in range(4):
                r_p = [[j - step, i - step, 0.0], [j - step, i + step, 0.0], [j + step, i - step, 0.0], [j + step, i + step, 0.0]][ray]
                if offset is not None:
                    r_p[0] -= offset[0]
                    r_p[1] -= offset[1]
                p1 = [eulert[c][0] * r_p[0] + eulert[c][1] * r_p[1] + eulert[c][2] * r_p[2] for c in range(3)]
                p1s = [p1[c] - half[c] for c in range(3)]
                lo = [x_0, y_0, z_0]
                hi = [x_F, y_F, z_F]
                alpha_min = alpha_max = None
                for c in range(3):
                    a = (lo[c] - 0.5 - p1[c]) * inv[c]
                    b = (hi[c] + 0.5 - p1[c]) * inv[c]
                    aux_min, aux_max = (a, b) if a < b else (b, a)
                    alpha_min = aux_min if c == 0 else max(aux_min, alpha_min)
                    alpha_max = aux_max if c == 0 else min(aux_max, alpha_max)
                if alpha_max - alpha_min < 1e-6:
                    continue
                v = [p1[c] + direction[c] * alpha_min for c in range(3)]
                idx = [clip(rnd(v[c]), lo[c], hi[c]) for c in range(3)]
                alpha = alpha_min
                while True:
                    al = [(float(idx[c]) - p1s[c]) * inv[c] for c in range(3)]
                    diff = [math.fabs(alpha - al[c]) for c in range(3)]
                    src, diff_alpha = 0, diff[0]
                    if diff[1] < diff_alpha:
                        src, diff_alpha = 1, diff[1]
                    if diff[2] < diff_alpha:
                        src, diff_alpha = 2, diff[2]
                    ray_sum += diff_alpha * V[idx[2] - z_0, idx[1] - y_0, idx[0] - x_0]       # an index outside would raise
                    alpha = al[src]
                    idx[src] += sign[src]
                    if not (alpha_max - alpha) > 1e-6:
                        break
            P[i - y_0, j - x_0] = ray_sum * 0.25
    return P


@pytest.mark.parametrize("D", [8, 9])
def test_restatement_is_the_scalar_walk(oracle, D):
    rng = np.random.default_rng(D)
    V = rng.standard_normal((D, D, D))
    for ang in ref.EXACT_ANGLES[:3] + ref.generic_angles(2):
        for off in (None, ref.OFFSET):
            E = oracle.euler_matrix(*ang)
            plane, _, _ = ref.project_volume(V, E, off)
            assert np.array_equal(plane, _scalar_project_volume(V, E, off)), (ang, off)


def test_axis_aligned_projection_is_the_column_sum(oracle):
    # rot = tilt = psi = 0: direction (1e-6, 1e-6, 1), every ray stays in its pixel's column of voxels
    D = 9
    V = np.random.default_rng(3).standard_normal((D, D, D))
    plane, _, _ = ref.project_volume(V, oracle.euler_matrix(0, 0, 0), None)
    assert np.abs(plane - V.sum(axis=0)).max() < 1e-4


@pytest.mark.parametrize("D,n_generic", [(16, 4), (17, 4), (33, 1)])
def test_inputs_of_the_gpu_tests_have_few_marginal_pixels(oracle, D, n_generic):
    rng = np.random.default_rng(100 + D)
    blob = ref.blob_mask(D)
    rng.standard_normal((D, D, D))                             # the GPU tests draw their random volume first
    for vol in (blob, rng.random((D, D, D)) * blob):
        for ang in ref.EXACT_ANGLES + ref.generic_angles(n_generic):
            for off in (None, ref.OFFSET):
                plane, support, marginal = ref.project_volume(vol, oracle.euler_matrix(*ang), off)
                assert marginal.mean() <= 0.02, (ang, off, marginal.sum())
                assert support.any() and not support.all()
                assert np.array_equal(support[~marginal], plane[~marginal] > 0)


# ------------------------------------------------------------------ xmipp_subtract_projection: the program, the fit, the frequency map
import subprocess  # noqa: E402

from tests import xmipp_io  # noqa: E402

PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_subtract_projection")


@pytest.fixture(scope="module")
def xa():
    import xmipp3_amd
    xmipp3_amd.lib()
    return xmipp3_amd


def _run(args):
    return subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_usage_lists_every_reference_flag_with_its_default(xa):
    assert os.path.exists(PROG)
    r = _run(["--help"])
    assert r.returncode == 0 and "subtraction between particles and a reference" in r.stderr
    for line in ("-i <arg>", "-o <arg>", "--ref <arg>", "[--mask_roi <=>]", "[--cirmaskrad <=-1.0>]", "[--mask <=>]", "[--sampling <=1>]",
                 "[--max_resolution <=-1>]", "[--padding <=2>]", "[--sigma <=1>]", "[--nonNegative]", "[--boost]", "[--save <=>]", "[--subtract]",
                 "[--realSpaceProjection]", "[--ignoreCTF]", "[--noise_est]", "[--dev <=0>]"):
        assert line in r.stderr, line
    assert [l for l in r.stderr.splitlines() if "--save" in l and "ignored" in l]


def _files(tmp, D=8, vol_shape=None, img_shape=None, ctf_model=False):
    vol_shape = vol_shape or (D, D, D)
    img_shape = img_shape or (2, D, D)
    xmipp_io.write_volume(str(tmp / "ref.vol"), np.ones(vol_shape, np.float32))
    xmipp_io.write_stack(str(tmp / "in.stk"), np.ones(img_shape, np.float32))
    labels = ["image", "angleRot", "angleTilt", "anglePsi"] + (["ctfModel"] if ctf_model else [])
    rows = [[f"{i + 1}@{tmp / 'in.stk'}", 10.0, 20.0, 30.0] + (["some.ctfparam"] if ctf_model else []) for i in range(img_shape[0])]
    xmipp_io.write_xmd(str(tmp / "in.xmd"), [("noname", labels, rows)])
    return ["-i", str(tmp / "in.xmd"), "-o", str(tmp / "out.stk"), "--ref", str(tmp / "ref.vol")]


@pytest.mark.parametrize("case,msg", [
    ("noise_est", "--noise_est is not available"),
    ("oroot", "--oroot / --oext are not available"),
    ("oext", "--oroot / --oext are not available"),
    ("devices", "several devices are not supported"),
    ("ctf_model", "ctfModel files are not read"),
    ("non_square", "must be square"),
    ("non_cubic", "must be a cube"),
    ("other_size", "must have the size of the reference volume"),
])
def test_refusals(xa, tmp_path, case, msg):
    base = _files(tmp_path, vol_shape=(8, 8, 6) if case == "non_cubic" else None,
                  img_shape={"non_square": (2, 8, 6), "other_size": (2, 6, 6)}.get(case), ctf_model=case == "ctf_model")
    extra = {"noise_est": ["--noise_est"], "oroot": ["--oroot", "x"], "oext": ["--oext", "mrc"], "devices": ["--dev", "0", "1"]}.get(case, [])
    r = _run(base + extra)
    assert r.returncode == 61 and "XMIPP_ERROR 61" in r.stderr and msg in r.stderr, r.stderr       # ERR_NOT_IMPLEMENTED
    assert not (tmp_path / "out.xmd").exists()


def test_missing_reference_is_an_error(xa):
    r = _run(["-i", "a.xmd", "-o", "o.stk"])
    assert r.returncode != 0 and "--ref is mandatory" in r.stderr


@pytest.mark.parametrize("D", [16, 17])
@pytest.mark.parametrize("maxres", [-1.0, 2.0])
def test_frequency_map_and_cut(xa, D, maxres):
    sampling = 1.0 if maxres == -1.0 else 1.7
    mr = maxres if maxres == -1.0 else 2 * sampling
    wi, maxwi = xa.sub_freq_map(D, sampling, mr)
    ewi, emaxwi = ref.freq_map(D, sampling, mr)
    assert np.array_equal(wi, ewi) and maxwi == emaxwi
    # by hand: sampling / maxResol over sqrt(2), times D, rounded
    assert maxwi == int(math.floor(D * ((1.0 if maxres == -1.0 else 0.5) / math.sqrt(2.0)) + 0.5))
    assert wi[0, 0] == 0 and wi[1, 0] == 1 and wi[D - 1, 0] == 1 and wi[0, D // 2] == D // 2 and wi[1, 1] == 1 and wi[2, 2] == 3


def _fit_by_hand(S, maxwi, a11):
    w = np.arange(maxwi + 1.0)
    use = (w > 0) & (w < maxwi)
    num, den = S[use, 0].sum(), S[use, 1].sum()
    a01, b11 = (w * S[:, 2])[use].sum(), (w * S[:, 3])[use].sum()
    A = np.array([[den, a01], [a01, a11]])
    return num / den, np.linalg.lstsq(A, np.array([num, b11]), rcond=None)[0]


def test_fit_on_hand_made_sums(xa):
    rng = np.random.default_rng(5)
    maxwi = 6
    S = rng.uniform(0.5, 2.0, (maxwi + 1, 4))
    S[0] = 1e9                                     # wi = 0 and wi = maxwiIdx stay out of the fit
    S[maxwi] = -1e9
    a11 = 40.0
    beta00, beta01, beta1 = xa.sub_fit(S, maxwi, a11)
    e00, (e01, e1) = _fit_by_hand(S, maxwi, a11)
    assert abs(beta00 - e00) <= 1e-14 * abs(e00)
    assert abs(beta01 - e01) <= 1e-10 * abs(e01) and abs(beta1 - e1) <= 1e-10 * abs(e1)
    # an exact case: PiMFourier = 2 in one cell per wi (re = 2, im = 0), IiMFourier = 3 PiMFourier: beta00 = 3, and T(w) = 3 + 0 w solves the system
    S = np.zeros((maxwi + 1, 4))
    for w in range(1, maxwi):
        S[w] = [12.0, 4.0, 2.0, 6.0]
    a11 = float(sum(2 * w for w in range(1, maxwi)))
    beta00, beta01, beta1 = xa.sub_fit(S, maxwi, a11)
    e00, (e01, e1) = _fit_by_hand(S, maxwi, a11)
    assert beta00 == 3.0 and abs(beta01 - e01) <= 1e-12 and abs(beta1 - e1) <= 1e-12
    with pytest.raises(xa.XhError):
        xa.sub_fit(np.zeros((3, 4)), maxwi, 1.0)


def test_model_choice_on_hand_made_sums(xa):
    cells = 100.0
    N = 2 * cells
    sumY, sumY2 = 10.0, 60.0
    varY = sumY2 / N - (sumY / N) ** 2
    # order 1 fits much better: it wins, with its adjusted R2
    R2adj, model, R20adj = xa.sub_choose(sumY, sumY2, 20.0, 5.0, cells)
    e20 = 1 - (20.0 / N) / varY
    e21 = 1 - (1 - (1 - (5.0 / N) / varY)) * (N - 1) / (N - 2)
    assert model == 1 and abs(R2adj - e21) <= 1e-14 and abs(R20adj - e20) <= 1e-14
    # order 1 fits a little better, but not after the adjustment for its second parameter: order 0
    R2adj, model, _ = xa.sub_choose(sumY, sumY2, 20.0, 19.95, cells)
    assert model == 0 and abs(R2adj - e20) <= 1e-14
    # R21adj == R20adj gives order 0: the comparison is strict. sumE1 = sumE0 (N - 2) / (N - 1) makes them equal; chosen so that every
    # step is exact in binary (N - 2 = 2, N - 1 = 3 would not be; here N = 3, cells = 1.5: (N - 1) / (N - 2) = 2)
    sumE0, cells = 0.5, 1.5
    R2adj, model, R20adj = xa.sub_choose(0.0, 3.0, sumE0, sumE0 / 2, cells)
    assert model == 0 and R2adj == R20adj == 1 - (sumE0 / 3.0) / 1.0
