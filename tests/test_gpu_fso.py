"""GPU parity of xmipp_resolution_fso (xh_fso_*, FSO in api.py) against the numpy restatement of the reference (tests/fso_ref.py): the
shell-sorted layout, the global sums, the cone sums, the threshold decisions, the 3DFSC and the program end to end.

Shapes: (24, 28, 30) with segments of 64 coefficients (many segments per shell, odd-length tails, a box that is not cubic), 32^3 with
segments of 256, 64^3 with the default segment, and volume_tiles.BIG, where the mask kernel's grid-stride loop takes a second lap (every
other kernel of xh_fso.hip has one thread, wave or workgroup per item and no such loop). Direction sets: level 3 (321: five full waves
and a tail of one lane), level 2 (81), level 2 with every other direction flipped to its antipode, a single direction, the three axes. The restatement of a case is computed once and shared.

Bounds. The in-cone counts are exact: the comparison is float arithmetic in a fixed order, the check on FMA contraction. The weights can
differ by expf's last bits, at most about 2.4e-7 relative each, and |num| <= sqrt(den1 den2) bounds the effect on an FSC at about 4 eps:
1e-6 absolute. The 3DFSC adds a float accumulation over about 14 terms: 2e-6. A (direction, shell) pair is marginal when the
restatement's FSC lies within 1e-5 of the threshold; decisions are compared where no marginal pair can change them. Values read from a
metadata file carry the 5e-7 of their six decimals."""
import os
import subprocess

import numpy as np
import pytest

from tests import fso_ref as R
from tests import volume_tiles as T
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_resolution_fso")
SMALL, CUBE, C64, BIG = (24, 28, 30), (32, 32, 32), (64, 64, 64), T.BIG
SEG = {SMALL: 64, CUBE: 256, C64: 0, BIG: 0}
THRS, ANGLE, SAMPLING = 0.143, 17.0, 1.0
MARGIN = 1e-5
PRINTED = 5e-7


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_IN, _LAY, _DIRS, _CONES = {}, {}, {}, {}


def inputs(shape):
    """the synthetic pair and its mask as a float file stores them"""
    if shape not in _IN:
        _IN[shape] = tuple(a.astype(np.float32).astype(np.float64) for a in R.synth(shape, 3))
    return _IN[shape]


def ref_layout(shape, masked=True):
    key = (shape, masked)
    if key not in _LAY:
        h1, h2, m = inputs(shape)
        _LAY[key] = R.layout(shape, *R.spectra(h1, h2, m if masked else None))
    return _LAY[key]


def directions(name):
    import xmipp3_amd as xa
    if name not in _DIRS:
        if name == "level3":
            d = R.unit_vectors(xa.fso_directions(3))
        elif name == "level2":
            d = R.unit_vectors(xa.fso_directions(2))
        elif name == "single":
            d = R.unit_vectors(xa.fso_directions(3))[137:138]
        elif name == "axes":
            d = np.eye(3, dtype=np.float32)
        elif name == "flipped":                 # level 2 with every other direction replaced by its antipode: the same cones
            d = R.unit_vectors(xa.fso_directions(2)) * np.where(np.arange(81) % 2, -1, 1).astype(np.float32)[:, None]
        else:                                   # what the program uses
            d = xa.fso_unit_vectors(xa.fso_directions(3))
        _DIRS[name] = np.ascontiguousarray(d, np.float32)
    return _DIRS[name]


def ref_cones(shape, name, masked=True):
    key = (shape, name, masked)
    if key not in _CONES:
        cosA, aux = R.cone(ANGLE)
        _CONES[key] = R.cone_sums(ref_layout(shape, masked), directions(name), cosA, aux)
    return _CONES[key]


def loaded(gpu, shape, masked=True, seg=None):
    xa, ctx, torch = gpu
    h1, h2, m = inputs(shape)
    f = xa.FSO(ctx, shape, seg=SEG[shape] if seg is None else seg)
    sums, cnt = f.load(torch.from_numpy(h1).cuda(), torch.from_numpy(h2).cuda(), torch.from_numpy(m).cuda() if masked else None)
    return f, sums, cnt


def read_mrc(path):
    h = np.fromfile(path, np.int32, 256)
    assert h[3] == 2
    return np.fromfile(path, np.float32, int(h[0]) * int(h[1]) * int(h[2]), offset=1024 + int(h[23])).reshape(int(h[2]), int(h[1]), int(h[0]))


# ---------------------------------------------------------------- layout and global sums
@pytest.mark.parametrize("shape,masked", [(SMALL, True), (CUBE, True), (CUBE, False), (C64, True), (BIG, True)])
def test_layout_and_global_sums(gpu, shape, masked):
    xa, ctx, torch = gpu
    exp = ref_layout(shape, masked)
    f, sums, cnt = loaded(gpu, shape, masked)
    info = f.info()
    n = exp["freqidx"].size
    assert info["ncomps"] == n and info["nshell"] == exp["L"] == shape[2] // 2 + 1
    assert np.array_equal(cnt, exp["shell_count"]) and cnt[0] == 1
    if shape == BIG:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert np.prod(shape) > 256 * 4 * cus, "the mask kernel's loop does not take a second lap on this device"
    if SEG[shape]:
        # several segments per shell and odd-length tails
        per_shell = -(-cnt // SEG[shape])
        assert info["seg"] == SEG[shape] and info["nseg"] == int(per_shell.sum()) - (1 if cnt[0] == 1 else 0) and (per_shell > 1).sum() > 5
        assert ((cnt % SEG[shape]) % 2 == 1).any()
    got = f.layout()
    assert np.array_equal(got["freqidx"], exp["freqidx"]) and np.array_equal(got["arr2indx"], exp["arr2indx"])
    # the DC coefficient is position 0; the reference gives it 0 inf = NaN
    assert got["arr2indx"][0] == 0 and all(np.isnan(got[k][0]) and np.isnan(exp[k][0]) for k in ("fx", "fy", "fz"))
    for k in ("fx", "fy", "fz", "real_z1z2", "absz1", "absz2"):
        lo = 1 if k[0] == "f" else 0
        ulps = np.abs(got[k][lo:].astype(np.float64) - exp[k][lo:].astype(np.float64)) / np.spacing(np.abs(exp[k][lo:])).astype(np.float64)
        print(f"layout {shape} masked {masked}: {k} differs in {int((ulps > 0).sum())} of {n} values, at most {ulps.max():.0f} ulp")
        assert ulps.max() <= 1, k
    # global sums, 1e-12 relative: den1 and den2 of themselves; num, which cancels in the shells of noise, of sqrt(den1 den2) >= |num|
    e = exp["sums"]
    scale = np.stack([np.sqrt(e[:, 1] * e[:, 2]), e[:, 1], e[:, 2]], 1)
    err = np.abs(sums - e) / scale
    print(f"global sums {shape}: largest error {err.max():.3e} (of num relative to itself: {(np.abs(sums - e)[:, 0] / np.abs(e[:, 0])).max():.3e})")
    assert err.max() <= 1e-12
    # two loads give the same bytes
    f2, sums2, _ = loaded(gpu, shape, masked)
    got2 = f2.layout()
    assert sums2.tobytes() == sums.tobytes() and all(got2[k].tobytes() == got[k].tobytes() for k in got)


def test_refusals(gpu):
    xa, ctx, torch = gpu
    with pytest.raises(xa.XhError, match="below 8"):
        xa.FSO(ctx, (6, 8, 8))
    with pytest.raises(xa.XhError, match="odd X"):
        xa.FSO(ctx, (16, 16, 15))
    with pytest.raises(xa.XhError, match="segment"):
        xa.FSO(ctx, CUBE, seg=4096)
    f = xa.FSO(ctx, SMALL)
    d = directions("axes")
    cosA, aux = R.cone(ANGLE)
    with pytest.raises(xa.XhError, match="nothing is loaded"):
        f.directional(d, cosA, aux)
    h1, h2, m = inputs(SMALL)
    with pytest.raises(xa.XhError, match="shape"):
        f.load(torch.from_numpy(h1).cuda(), torch.zeros((24, 28, 28), dtype=torch.float64, device="cuda"))
    f.load(torch.from_numpy(h1).cuda(), torch.from_numpy(h2).cuda())
    with pytest.raises(xa.XhError, match="cubic"):
        f.threedfsc(d, cosA, aux, np.zeros((3, f.L), np.float32))
    with pytest.raises(xa.XhError, match="directions"):
        f.directional(np.zeros((1025, 3), np.float32), cosA, aux)


# ---------------------------------------------------------------- cones
CONE_CASES = [(s, n) for s in (SMALL, CUBE) for n in ("level3", "level2", "single", "axes")] + [(SMALL, "flipped"), (C64, "level3"), (BIG, "level3")]


@pytest.mark.parametrize("shape,name", CONE_CASES)
def test_cone_sums(gpu, shape, name):
    dirs = directions(name)
    cosA, aux = R.cone(ANGLE)
    esums, ecnt = ref_cones(shape, name)
    f, _, _ = loaded(gpu, shape)
    sums, cnt = f.directional(dirs, cosA, aux)
    assert ecnt.min() > 0 and np.array_equal(cnt, ecnt)
    err = np.abs(R.dir_fsc(sums).astype(np.float64) - R.dir_fsc(esums).astype(np.float64))
    print(f"cones {shape} {name}: {len(dirs)} directions, {int(cnt.sum())} in-cone pairs, largest FSC error {err.max():.3e}")
    assert err.max() <= 1e-6
    assert not sums[:, 0, :].any()                    # the DC coefficient is in no cone
    if name == "flipped":
        assert np.array_equal(ecnt, ref_cones(shape, "level2")[1]) and (directions(name)[:, 2] < 0).sum() > 30
    # determinism: the same handle again, and a fresh one
    sums2, cnt2 = f.directional(dirs, cosA, aux)
    sums3, cnt3 = loaded(gpu, shape)[0].directional(dirs, cosA, aux)
    assert sums2.tobytes() == sums.tobytes() == sums3.tobytes() and cnt2.tobytes() == cnt.tobytes() == cnt3.tobytes()


def test_segment_size_moves_the_last_bits_only(gpu):
    dirs = directions("level2")
    cosA, aux = R.cone(ANGLE)
    out = {}
    for seg in (64, 100, 2048):
        f, _, _ = loaded(gpu, SMALL, seg=seg)
        out[seg] = f.directional(dirs, cosA, aux)
        assert f.info()["seg"] == seg
    for seg in (100, 2048):
        assert np.array_equal(out[seg][1], out[64][1])
        assert np.abs(out[seg][0] - out[64][0]).max() <= 1e-13 * np.abs(out[64][0]).max()


def test_timed_run_changes_no_byte(gpu):
    """set_timing(True) puts a wait after every stage: load and directional return the same bytes, the stages report times (SMALL is no
    cube: the 3DFSC's stays 0), and set_timing resets them"""
    xa, ctx, torch = gpu
    h1, h2, m = (torch.from_numpy(a).cuda() for a in inputs(SMALL))
    dirs = directions("level2")
    cosA, aux = R.cone(ANGLE)
    f = xa.FSO(ctx, SMALL, seg=SEG[SMALL])

    def run():
        return [a.tobytes() for a in f.load(h1, h2, m) + f.directional(dirs, cosA, aux)]

    out = run()
    assert set(f.stage_ms().values()) == {0.0}                  # an untimed run reports nothing
    f.set_timing(True)
    out_t = run()
    ms = f.stage_ms()
    print(f"stage ms: {ms}")
    assert out_t == out
    assert list(ms) == list(xa.FSO.STAGES) and len(ms) == 5
    assert all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
    assert all(ms[k] > 0.0 for k in ("transforms", "layout", "cones", "segment_reduce"))
    f.set_timing(False)
    assert set(f.stage_ms().values()) == {0.0}
    assert run() == out
    assert set(f.stage_ms().values()) == {0.0}
    f.close()


# ---------------------------------------------------------------- threshold decisions
def check_decisions(got, exp, ndir, what):
    """got, exp: (fsc, resolution, fso, bingham) of the device sums and of the restatement"""
    import xmipp3_amd as xa
    fsc, resol, fso, bingham = exp
    marginal = np.abs(fsc.astype(np.float64) - THRS) <= MARGIN
    marginal[:, :3] &= False                                  # shells 0 .. 2 decide nothing that is compared: i > 2 (:480), FSO set to 1
    print(f"{what}: {int(marginal.sum())} marginal pairs of {marginal.size}")
    assert marginal.sum() <= 0.01 * marginal.size
    clear_dir, per_shell = ~marginal.any(1), marginal.sum(0)
    assert np.array_equal(got[1][clear_dir], resol[clear_dir]) and clear_dir.sum() >= 0.9 * ndir
    assert (np.abs(got[2].astype(np.float64) - fso.astype(np.float64)) <= per_shell / ndir + 2.0 ** -24).all()
    tab_g = np.array([xa.fso_incomplete_gamma(b) for b in got[3]])
    tab_e = np.array([R.incomplete_gamma(b) for b in bingham])
    assert np.array_equal(tab_g[per_shell == 0], tab_e[per_shell == 0])
    assert (fso[5:] < 1).any() and (resol > 0).any()


@pytest.mark.parametrize("shape", [SMALL, CUBE, C64])
def test_threshold_decisions(gpu, shape):
    xa, ctx, torch = gpu
    dirs = directions("level3")
    cosA, aux = R.cone(ANGLE)
    f, _, _ = loaded(gpu, shape)
    sums, _ = f.directional(dirs, cosA, aux)
    got = xa.fso_decide(sums, dirs, shape[2], SAMPLING, THRS)
    exp = R.decide(ref_cones(shape, "level3")[0], dirs, shape[2], SAMPLING, THRS)
    check_decisions(got, exp, len(dirs), f"decisions {shape}")


# ---------------------------------------------------------------- 3DFSC
@pytest.mark.parametrize("shape,name", [(CUBE, "level3"), (CUBE, "axes"), (C64, "level3")])
def test_threedfsc(gpu, shape, name):
    xa, ctx, torch = gpu
    dirs = directions(name)
    cosA, aux = R.cone(ANGLE)
    lay = ref_layout(shape)
    fsc = R.dir_fsc(ref_cones(shape, name)[0])
    ehalf, efull = R.threedfsc(shape, lay, dirs, cosA, aux, fsc)
    f, _, _ = loaded(gpu, shape)
    half, full = f.threedfsc(dirs, cosA, aux, fsc)
    half, full = half.cpu().numpy(), full.cpu().numpy()
    err = max(np.abs(half - ehalf).max(), np.abs(full - efull).max())
    print(f"3DFSC {shape} {name}: largest error {err:.3e}; values {ehalf.min():.3f} .. {ehalf.max():.3f}")
    assert err <= 2e-6
    Y = shape[1]
    # the line fixes by index, and that they changed something: the rows i > Y / 2 of column 0 are not in the layout
    assert np.array_equal(half[:, Y // 2 + 1:, 0], half[:, Y // 2 + 1:, 1]) and np.array_equal(half[:, 0, 0], half[:, 0, 1])
    assert half[:, Y // 2 + 1:, 0].any() and half[0, 0, 0] == half[0, 0, 1]
    assert np.array_equal(full, R.complete_and_center(half, shape[2]))
    if name == "axes":
        assert (ehalf == 1).sum() > 100 and (ehalf == 0).sum() > 100      # NaN -> 1 where no cone reaches; 0 outside the layout
    half2, full2 = f.threedfsc(dirs, cosA, aux, fsc)
    assert half2.cpu().numpy().tobytes() == half.tobytes() and full2.cpu().numpy().tobytes() == full.tobytes()


# ---------------------------------------------------------------- the Python run and the program
def test_run_returns_what_its_stages_return(gpu):
    xa, ctx, torch = gpu
    h1, h2, m = (torch.from_numpy(a).cuda() for a in inputs(CUBE))
    f = xa.FSO(ctx, CUBE, seg=SEG[CUBE])
    out = f.run(h1, h2, m, sampling=SAMPLING, anglecone=ANGLE, threshold=THRS, threedfsc=True)
    dirs = directions("program")
    cosA, aux = xa.fso_cone(ANGLE)
    assert np.array_equal(out["dirs"], dirs) and len(dirs) == 321
    sums, cnt = f.directional(dirs, cosA, aux)
    fsc, resol, fso, bingham = xa.fso_decide(sums, dirs, CUBE[2], SAMPLING, THRS)
    assert np.array_equal(out["counts"], cnt) and np.array_equal(out["fsc"], fsc) and np.array_equal(out["fso"], fso) and np.array_equal(out["resolution"], resol)
    half, full = f.threedfsc(dirs, cosA, aux, fsc)
    assert torch.equal(out["threedfsc_half"], half) and torch.equal(out["threedfsc_full"], full)
    assert out["distribution"].shape == (360, 91) and out["anisotropy"].shape == (17,)


def _xmd_columns(path, labels):
    got, rows = xmipp_io.read_xmd(path)
    assert got == labels, (path, got)
    return np.array([[float(v) for v in r] for r in rows])


@pytest.mark.parametrize("masked,flag", [(True, True), (False, False)])
def test_program_end_to_end(gpu, tmp_path, masked, flag):
    xa, ctx, torch = gpu
    shape = CUBE
    h1, h2, m = inputs(shape)
    for name, v in (("h1", h1), ("h2", h2), ("m", m)):
        xmipp_io.write_volume(str(tmp_path / (name + ".vol")), v)
    out = tmp_path / "results"
    args = ["--half1", str(tmp_path / "h1.vol"), "--half2", str(tmp_path / "h2.vol"), "-o", str(out), "--sampling", str(SAMPLING), "--threads", "3"]
    args += (["--mask", str(tmp_path / "m.vol")] if masked else []) + (["--threedfsc_filter"] if flag else [])
    r = subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    expected = ["GlobalFSC.xmd", "Resolution_Distribution.xmd", "fso.xmd"]
    if flag:
        expected += ["3dFSC.mrc", "filteredHalfMap1.mrc", "filteredHalfMap2.mrc", "threeD_FSC.mrc"]
    assert sorted(os.listdir(out)) == sorted(expected)
    assert not (tmp_path / "threeD_FSC.mrc").exists()                 # the reference writes it to the working directory
    # the restatement with the directions the program uses
    dirs = directions("program")
    cosA, aux = R.cone(ANGLE)
    lay = ref_layout(shape, masked)
    esums, _ = ref_cones(shape, "program", masked)
    exp = R.decide(esums, dirs, shape[2], SAMPLING, THRS)
    L, ndir = lay["L"], len(dirs)
    freq = R.freq_axis(L, shape[2], SAMPLING)[1:]
    g = _xmd_columns(str(out / "GlobalFSC.xmd"), ["resolutionFreqFourier", "resolutionFRC", "resolutionFreqReal"])
    assert g.shape == (L - 1, 3) and np.abs(g[:, 0] - freq).max() <= PRINTED and np.abs(g[:, 2] - 1 / freq).max() <= PRINTED
    assert np.abs(g[:, 1] - R.global_fsc(lay["sums"])[1:]).max() <= 1e-12 + PRINTED
    assert "Resolution " in r.stdout
    a = _xmd_columns(str(out / "fso.xmd"), ["resolutionFreqFourier", "resolutionFSO", "resolutionFreqReal", "resolutionAnisotropy"])
    marginal = np.abs(exp[0].astype(np.float64) - THRS) <= MARGIN
    marginal[:, :3] &= False
    print(f"program masked {masked}: {int(marginal.sum())} marginal pairs of {marginal.size}")
    assert marginal.sum() <= 0.01 * marginal.size
    per_shell = marginal.sum(0)[1:]
    assert a.shape == (L - 1, 4) and np.abs(a[:, 0] - freq).max() <= PRINTED
    assert (np.abs(a[:, 1] - exp[2].astype(np.float64)[1:]) <= per_shell / ndir + PRINTED).all()
    tab = np.array([R.incomplete_gamma(b) for b in exp[3]])[1:]
    assert (np.abs(a[:, 3] - tab)[per_shell == 0] <= PRINTED).all()
    # the resolution distribution: grid points on no cone's edge, inside no cone of a direction with a marginal pair
    d = _xmd_columns(str(out / "Resolution_Distribution.xmd"), ["angleRot", "angleTilt", "resolutionFRC"])
    assert d.shape == (360 * 91, 3) and np.array_equal(d[:, 0], np.repeat(np.arange(360.0), 91)) and np.array_equal(d[:, 1], np.tile(np.arange(91.0), 360))
    rot, tilt = np.radians(d[:, 0]), np.radians(d[:, 1])
    p = np.stack([np.sin(tilt) * np.cos(rot), np.sin(tilt) * np.sin(rot), np.cos(tilt)], 1)
    c = np.abs(p @ dirs.astype(np.float64).T)
    ok = (np.abs(c - float(cosA)).min(1) > 1e-6) & ~(c[:, marginal.any(1)] >= float(cosA) - 1e-6).any(1)
    assert ok.mean() >= 0.9
    edist = R.resolution_distribution(dirs, exp[1], ANGLE).ravel()
    assert (np.abs(d[:, 2] - edist)[ok] <= 1e-5 * np.abs(edist)[ok] + PRINTED).all()
    if flag:
        fsc = exp[0]
        ehalf, efull = R.threedfsc(shape, lay, dirs, cosA, aux, fsc)
        # a marginal pair does not enter here: the FSC values themselves are the weights' partners, and they agree to 1e-6
        assert np.abs(read_mrc(str(out / "threeD_FSC.mrc")) - ehalf).max() <= 2e-6 + 1e-6 + 2.0 ** -24
        assert np.abs(read_mrc(str(out / "3dFSC.mrc")) - efull).max() <= 2e-6 + 1e-6 + 2.0 ** -24
        mm = m if masked else 1.0
        assert np.array_equal(read_mrc(str(out / "filteredHalfMap1.mrc")), (h1 * mm).astype(np.float32))
        assert np.array_equal(read_mrc(str(out / "filteredHalfMap2.mrc")), (h2 * mm).astype(np.float32))
