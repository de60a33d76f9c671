"""GPU parity of xmipp_volume_subtraction (xh_vsub_*, VolumeSubtraction in api.py) against the numpy fp64 restatement of the reference
(tests/volume_subtraction_ref.py): the hooks, the full adjustment, the energies, the subtraction, and the program end to end.

Shapes, Z x Y x X: 32^3, 27^3 (odd: Bluestein lines), 36 x 30 x 25 (non-cubic, empty radial bins: the NaN -> 0 of the quotient) and
82 x 80 x 81 (beyond 64 a side, no power-of-two side, more than one lap of the grid-stride loops' workgroups), the last with 2
iterations; one iteration at 130^3, where the loops over the half spectrum and over the octant's rows take a second lap. The
restatement of a case is computed once and shared.

Bounds. Volumes: 1e-10 of max|V1|, the bound the full runs of LocalDeblur carry. Its margin: an fp64 transform pair is good to some
1e-15 of the maximum, and the iteration does not amplify: the test perturbs the restatement's input by 1e-12 and asserts that the
output moves by less than 100 times that (observed: 0.14 .. 0.92), so the device may differ from the restatement by 1e-13 at the most.
Tables (radial mean, quotient): 1e-12 relative; spectrum magnitudes: 1e-12 of the largest.

Precondition of the plain amplitude mode: it is discontinuous at mod = 1e-10, so every case compared in it first asserts that the
restatement saw no coefficient with a modulus in [0.5e-10, 2e-10] at any amplitude step. At 82 x 80 x 81 the raised-cosine edge of
cutFreq can put coefficients there, so that box runs cutFreq in --radavg mode only."""
import os
import subprocess

import numpy as np
import pytest

from tests import volume_subtraction_ref as R
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_volume_subtraction")
SMALL = [(32, 32, 32), (27, 27, 27), (36, 30, 25)]
BIG = (82, 80, 81)
SHAPES = SMALL + [BIG]
CUT = 0.3
MODES = [(False, 0.0), (False, CUT), (True, 0.0), (True, CUT)]
# (shape, iterations, radavg, cutFreq)
FULL = [(s, 5, r, c) for s in SMALL for r, c in MODES] + [(BIG, 2, False, 0.0), (BIG, 2, True, 0.0), (BIG, 2, True, CUT)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_IN, _REF, _ADJ = {}, {}, {}


def inputs(shape):
    if shape not in _IN:
        _IN[shape] = R.synth(shape, 3)
    return _IN[shape]


def reference(shape, masked=True):
    key = (shape, masked)
    if key not in _REF:
        v1, _, mask = inputs(shape)
        _REF[key] = R.Reference(v1, mask if masked else np.ones(shape))
    return _REF[key]


def ref_adjust(shape, niter, radavg, cut, masked=True, which=1):
    """which: 1 adjusts the synthetic V, 2 a second volume (V rolled and rescaled), for the handle re-use test"""
    key = (shape, niter, radavg, cut, masked, which)
    if key not in _ADJ:
        _ADJ[key] = R.adjust(reference(shape, masked), target(shape, which), niter, 1.0, radavg, cut)
    return _ADJ[key]


def target(shape, which=1):
    v = inputs(shape)[1]
    return v if which == 1 else (0.5 * np.roll(v, (1, -2, 3), axis=(0, 1, 2)) + 0.01).astype(np.float32).astype(np.float64)


def bound(shape):
    return 1e-10 * np.abs(inputs(shape)[0]).max()


def handle(gpu, shape, radavg=False, masked=True):
    xa, ctx, torch = gpu
    v1, _, mask = inputs(shape)
    h = xa.VolumeSubtraction(ctx, shape)
    h.set_reference(torch.from_numpy(v1).cuda(), torch.from_numpy(mask).cuda() if masked else None, radavg)
    return h


def dev(gpu, a):
    return gpu[2].from_numpy(np.ascontiguousarray(a)).cuda()


def no_coefficient_near_the_threshold(ref):
    assert len(ref["near"]) > 0 and sum(ref["near"]) == 0, ref["near"]


# ---------------------------------------------------------------- hooks
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_side_info_and_magnitude(gpu, shape):
    ref = reference(shape)
    h = handle(gpu, shape)
    info = h.info()
    assert info["v1min"] == ref.v1min and info["v1max"] == ref.v1max and info["nbins"] == R.num_bins(shape)
    assert abs(info["std1"] - ref.std1) <= 1e-12 * ref.std1
    got = h.reference_magnitude().cpu().numpy()
    err = float(np.abs(got - ref.v1mag).max() / ref.v1mag.max())
    print(f"V1FourierMag {shape}: error {err:.3e} of the largest")
    assert err <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_radial_mean_and_quotient(gpu, shape):
    ref = reference(shape)
    h = handle(gpu, shape, radavg=True)
    exp = R.radial_average(ref.v1mag, shape)
    got = h.radial_mean(dev(gpu, ref.v1mag))
    empty = np.isnan(exp)
    assert np.array_equal(np.isnan(got), empty) and (empty.sum() > 0) == (shape == (36, 30, 25))
    err = float(np.abs(got[~empty] / exp[~empty] - 1).max())
    prepared = ref_adjust(shape, 0, True, 0.0)["prepared"]
    q_exp = R.rad_quotient(ref.v1mag, np.abs(R.ft(prepared)), shape)
    q = h.quotient(dev(gpu, prepared))
    assert (q[empty] == 0).all() and (q >= 0).all() and (q <= 1).all() and np.array_equal(q == 1, q_exp == 1)
    qerr = float(np.abs(q[~empty] / q_exp[~empty] - 1).max())
    print(f"radial mean {shape}: {empty.sum()} empty bins, error {err:.3e}, quotient {qerr:.3e} (relative), {int((q_exp == 1).sum())} bins clamped to 1")
    assert err <= 1e-12 and qerr <= 1e-12
    assert h.radial_mean(dev(gpu, ref.v1mag)).tobytes() == got.tobytes()


@pytest.mark.parametrize("radavg,cut", MODES)
@pytest.mark.parametrize("shape", SMALL)
def test_one_iteration(gpu, shape, radavg, cut):
    """runIteration on the restatement's state after two iterations, with the phases and the quotient of the prepared input"""
    ref = reference(shape)
    full = ref_adjust(shape, 5, radavg, cut)
    if not radavg:
        no_coefficient_near_the_threshold(full)
    v0, v = full["states"][0], full["states"][2]
    exp, _ = R.run_iteration(ref, v, R.extract_phase(R.ft(v0)), 1.0, radavg, cut, full["quotient"])
    got = handle(gpu, shape, radavg).iteration(dev(gpu, v0), dev(gpu, v), 1.0, radavg, cut).cpu().numpy()
    err = float(np.abs(got - exp).max())
    print(f"one iteration {shape} radavg {radavg} cutFreq {cut}: error {err:.3e}, bound {bound(shape):.3e}")
    assert err <= bound(shape)


@pytest.mark.parametrize("shape", SMALL)
def test_smoothed_mask(gpu, shape):
    mask = inputs(shape)[2]
    exp = R.smooth_mask(mask, 3)
    got = handle(gpu, shape).smooth_mask(dev(gpu, mask), 3).cpu().numpy()
    err = float(np.abs(got - exp).max())
    print(f"smoothed mask {shape}: error {err:.3e}")
    assert err <= 1e-12 and exp.max() - exp.min() > 0.1


@pytest.mark.parametrize("shape", [(27, 27, 27), (36, 30, 25)])
def test_subtraction_formula_is_exact(gpu, shape):
    """given equal inputs the formula has one rounding per operation on both sides"""
    v1, _, mask = inputs(shape)
    vadj = ref_adjust(shape, 5, False, 0.0)["adjusted"]
    msub = R.smooth_mask(mask, 3)
    h = handle(gpu, shape)
    out, v1f = (t.cpu().numpy() for t in h.subtract(dev(gpu, v1), dev(gpu, vadj), dev(gpu, msub), 0.0))
    exp, _ = R.subtraction(v1, vadj, msub, 0.0)
    assert np.array_equal(v1f, v1) and np.array_equal(out, exp)
    assert (vadj < v1).any() and (vadj > v1).any()                       # both branches of the min
    # with the low pass: V1F within the bound, and the formula exact on the device's own V1F
    out, v1f = (t.cpu().numpy() for t in h.subtract(dev(gpu, v1), dev(gpu, vadj), dev(gpu, msub), CUT))
    exp, exp_f = R.subtraction(v1, vadj, msub, CUT)
    assert np.abs(v1f - exp_f).max() <= bound(shape)
    assert np.array_equal(out, v1 * (1 - msub) + (v1f - np.minimum(vadj, v1f)) * msub)
    assert np.abs(out - exp).max() <= bound(shape)
    assert np.array_equal(h.lowpass(dev(gpu, v1), CUT).cpu().numpy(), v1f)


# ---------------------------------------------------------------- the full adjustment
@pytest.mark.parametrize("shape,niter,radavg,cut", FULL)
def test_full_adjust(gpu, shape, niter, radavg, cut):
    ref = reference(shape)
    exp = ref_adjust(shape, niter, radavg, cut)
    if not radavg:
        no_coefficient_near_the_threshold(exp)
    # the margin of the bound: what the iteration does to a perturbation of 1e-12
    p = 1e-12 * np.random.default_rng(1).standard_normal(shape)
    moved = R.adjust(ref, target(shape), niter, 1.0, radavg, cut, perturb=p)["adjusted"]
    factor = float(np.abs(moved - exp["adjusted"]).max() / np.abs(p).max())
    got = handle(gpu, shape, radavg).adjust(dev(gpu, target(shape)), niter, 1.0, radavg, cut).cpu().numpy()
    err = float(np.abs(got - exp["adjusted"]).max())
    print(f"adjust {shape} x{niter} radavg {radavg} cutFreq {cut}: error {err:.3e}, bound {bound(shape):.3e}, amplification {factor:.2f}")
    assert factor <= 100
    assert err <= bound(shape)
    if cut == 0:
        assert (got >= 0).all() and abs(R.stddev(got) - ref.std1) <= 1e-12 * ref.std1


def test_one_iteration_past_the_grid_caps(gpu):
    """130^3: the half spectrum (1 115 400 elements) and the octant's rows (65 x 65 = 4225) exceed what the spectrum kernels' and
    k_vs_radial_rows' grids cover in one lap (8 workgroups per CU; 4096 rows), so their loops take a second lap. One iteration in each
    amplitude mode, the low pass with --radavg"""
    xa, ctx, torch = gpu
    shape = (130, 130, 130)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert shape[0] * shape[1] * (shape[2] // 2 + 1) > 256 * 8 * cus and (shape[0] // 2) * (shape[1] // 2) > 4096
    ref = reference(shape)
    exp_q = ref_adjust(shape, 1, True, CUT)
    prepared = exp_q["prepared"]
    q = handle(gpu, shape, radavg=True).quotient(dev(gpu, prepared))
    qerr = float(np.abs(q / exp_q["quotient"] - 1).max())
    print(f"quotient {shape}: {qerr:.3e} (relative)")
    assert qerr <= 1e-12
    for radavg, cut in ((False, 0.0), (True, CUT)):
        exp = ref_adjust(shape, 1, radavg, cut)
        if not radavg:
            no_coefficient_near_the_threshold(exp)
        got = handle(gpu, shape, radavg).adjust(dev(gpu, target(shape)), 1, 1.0, radavg, cut).cpu().numpy()
        err = float(np.abs(got - exp["adjusted"]).max())
        print(f"adjust {shape} x1 radavg {radavg} cutFreq {cut}: error {err:.3e}, bound {bound(shape):.3e}")
        assert err <= bound(shape)


@pytest.mark.parametrize("shape,niter,radavg,cut", [((27, 27, 27), 5, False, CUT), ((36, 30, 25), 5, True, 0.0), (BIG, 2, True, CUT)])
def test_energies_and_the_same_bytes_with_them(gpu, shape, niter, radavg, cut):
    exp = ref_adjust(shape, niter, radavg, cut)
    h = handle(gpu, shape, radavg)
    dv = dev(gpu, target(shape))
    plain = h.adjust(dv, niter, 1.0, radavg, cut)
    out, en = h.adjust(dv, niter, 1.0, radavg, cut, energies=True)
    assert out.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    assert len(en) == niter
    worst = 0.0
    for g, e in zip(en, exp["energies"]):
        for k in R.ENERGIES:
            if k == "filter" and cut == 0:
                assert g[k] == 0 and e[k] == 0
                continue
            assert e[k] > 0
            worst = max(worst, abs(g[k] - e[k]) / e[k])
    print(f"energies {shape} radavg {radavg} cutFreq {cut}: worst relative error {worst:.3e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("shape,radavg,cut", [((27, 27, 27), False, CUT), (BIG, True, 0.0)])
def test_two_runs_give_the_same_bytes(gpu, shape, radavg, cut):
    dv = dev(gpu, target(shape))
    a = handle(gpu, shape, radavg).adjust(dv, 2, 1.0, radavg, cut).cpu().numpy()
    b = handle(gpu, shape, radavg).adjust(dv, 2, 1.0, radavg, cut).cpu().numpy()
    assert a.tobytes() == b.tobytes()


def test_timed_run_changes_no_byte(gpu):
    """set_timing(True) puts a wait after every stage: the adjusted volume keeps its bytes, the four stages report times (radavg and a
    cut-off frequency: all four run), and set_timing resets them"""
    xa = gpu[0]
    shape = (36, 30, 25)
    dv = dev(gpu, target(shape))
    h = handle(gpu, shape, radavg=True)
    out = h.adjust(dv, 3, 1.0, True, CUT).cpu().numpy()
    assert set(h.stage_ms().values()) == {0.0}                  # an untimed run reports nothing
    h.set_timing(True)
    out_t = h.adjust(dv, 3, 1.0, True, CUT).cpu().numpy()
    ms = h.stage_ms()
    print(f"stage ms: {ms}")
    assert out_t.tobytes() == out.tobytes()
    assert list(ms) == list(xa.VolumeSubtraction.STAGES) and len(ms) == 4
    assert all(v > 0.0 for v in ms.values())
    h.set_timing(False)
    assert set(h.stage_ms().values()) == {0.0}
    assert h.adjust(dv, 3, 1.0, True, CUT).cpu().numpy().tobytes() == out.tobytes()
    assert set(h.stage_ms().values()) == {0.0}
    h.close()


@pytest.mark.parametrize("radavg", [False, True])
def test_one_reference_serves_two_volumes(gpu, radavg):
    shape = (36, 30, 25)
    h = handle(gpu, shape, radavg)
    a = h.adjust(dev(gpu, target(shape, 1)), 3, 1.0, radavg, CUT).cpu().numpy()
    b = h.adjust(dev(gpu, target(shape, 2)), 3, 1.0, radavg, CUT).cpu().numpy()
    a2 = h.adjust(dev(gpu, target(shape, 1)), 3, 1.0, radavg, CUT).cpu().numpy()
    assert a.tobytes() == a2.tobytes()
    assert b.tobytes() == handle(gpu, shape, radavg).adjust(dev(gpu, target(shape, 2)), 3, 1.0, radavg, CUT).cpu().numpy().tobytes()
    assert a.tobytes() == handle(gpu, shape, radavg).adjust(dev(gpu, target(shape, 1)), 3, 1.0, radavg, CUT).cpu().numpy().tobytes()
    exp = ref_adjust(shape, 3, radavg, CUT, which=2)
    if not radavg:
        no_coefficient_near_the_threshold(exp)
    assert np.abs(b - exp["adjusted"]).max() <= bound(shape) and np.abs(a - b).max() > 1e-3


def test_zero_iterations_give_the_masked_clipped_input(gpu):
    shape = (27, 27, 27)
    _, v, mask = inputs(shape)
    got = handle(gpu, shape).adjust(dev(gpu, v), 0).cpu().numpy()
    assert np.array_equal(got, np.maximum(0.0, v * mask)) and (got == 0).any() and (got > 0).any()
    out, en = handle(gpu, shape).adjust(dev(gpu, v), 0, energies=True)
    assert en == [] and np.array_equal(out.cpu().numpy(), got)


def test_without_a_mask(gpu):
    shape = (27, 27, 27)
    exp = ref_adjust(shape, 2, False, 0.0, masked=False)
    no_coefficient_near_the_threshold(exp)
    got = handle(gpu, shape, masked=False).adjust(dev(gpu, target(shape)), 2).cpu().numpy()
    assert np.abs(got - exp["adjusted"]).max() <= bound(shape)
    assert np.abs(exp["adjusted"] - ref_adjust(shape, 2, False, 0.0)["adjusted"]).max() > 1e-3


def test_refusals(gpu):
    xa, ctx, torch = gpu
    shape = (27, 27, 27)
    v1, v, mask = inputs(shape)
    h = xa.VolumeSubtraction(ctx, shape)
    with pytest.raises(xa.XhError, match="no reference"):
        h.adjust(dev(gpu, v))
    with pytest.raises(xa.XhError, match="shape"):
        h.set_reference(dev(gpu, v1), torch.zeros((27, 27, 26), dtype=torch.float64, device="cuda"))
    with pytest.raises(xa.XhError, match="stddev"):
        h.set_reference(torch.zeros(shape, dtype=torch.float64, device="cuda"))
    h.set_reference(dev(gpu, v1), dev(gpu, mask))
    for kw, text in (({"lam": 1.5}, "lambda"), ({"lam": -0.5}, "lambda"), ({"cut_freq": 0.6}, "cutFreq"), ({"cut_freq": -0.1}, "cutFreq"), ({"niter": -1}, "iterations")):
        with pytest.raises(xa.XhError, match=text):
            h.adjust(dev(gpu, v), **kw)
    with pytest.raises(xa.XhError, match="stddev"):
        h.adjust(torch.zeros(shape, dtype=torch.float64, device="cuda"), 1)
    with pytest.raises(xa.XhError, match="radial mean"):
        h.adjust(dev(gpu, v), 1, radavg=True)
    with pytest.raises(xa.XhError, match="sigma"):
        h.smooth_mask(dev(gpu, mask), -1)
    over = (24, 28, 30)
    ho = xa.VolumeSubtraction(ctx, over)
    z = torch.ones(over, dtype=torch.float64, device="cuda")
    with pytest.raises(xa.XhError, match="largest bin"):
        ho.set_reference(z, None, True)


# ---------------------------------------------------------------- the program
def _program(args):
    r = subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r


def _files(tmp_path, shape):
    v1, v, mask = inputs(shape)
    names = {}
    for k, a in (("v1", v1), ("v", v), ("m1", mask), ("m2", np.ones(shape)), ("msub", np.roll(mask, 2, axis=2))):
        names[k] = str(tmp_path / (k + ".vol"))
        xmipp_io.write_volume(names[k], a.astype(np.float32))
    return names


def _close(path, exp, shape):
    """a float file against the restatement: the volume bound plus the float's own rounding (one unit: a value may round the other way)"""
    got = xmipp_io.read_volume(path).astype(np.float64)
    return bool((np.abs(got - exp) <= bound(shape) + 2.0 ** -23 * np.abs(exp)).all())


def test_program_adjusts(gpu, tmp_path):
    shape = (27, 27, 27)
    f = _files(tmp_path, shape)
    out = str(tmp_path / "out.vol")
    r = _program(["--i1", f["v1"], "--i2", f["v"], "--mask1", f["m1"], "--mask2", f["m2"], "-o", out, "--computeEnergy"])
    exp = ref_adjust(shape, 5, False, 0.0)
    no_coefficient_near_the_threshold(exp)
    assert _close(out, exp["adjusted"], shape)
    lines = [l for l in r.stdout.splitlines() if l.startswith("Energy iteration")]
    assert len(lines) == 5 and "filter" not in lines[0]
    assert abs(float(lines[4].split()[4]) - exp["energies"][4]["amplitude"]) <= 1e-5 * exp["energies"][4]["amplitude"]
    assert not (tmp_path / "volume1_filtered.mrc").exists()


def test_program_takes_a_single_mask_as_no_mask(gpu, tmp_path):
    shape = (27, 27, 27)
    f = _files(tmp_path, shape)
    outs = []
    for extra in ([], ["--mask1", f["m1"]], ["--mask2", f["m1"]]):
        out = str(tmp_path / f"out{len(outs)}.vol")
        _program(["--i1", f["v1"], "--i2", f["v"], "-o", out, "--iter", "2"] + extra)
        outs.append(xmipp_io.read_volume(out))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert _close(str(tmp_path / "out0.vol"), ref_adjust(shape, 2, False, 0.0, masked=False)["adjusted"], shape)


@pytest.mark.parametrize("own_mask", [False, True])
def test_program_subtracts(gpu, tmp_path, own_mask):
    """--sub with the smoothed mask (--sigma 3) or with --maskSub; --radavg and --cutFreq on the way"""
    shape = (36, 30, 25)
    f = _files(tmp_path, shape)
    v1, v, mask = inputs(shape)
    out, s1, s2 = (str(tmp_path / n) for n in ("out.vol", "v1f.vol", "v2a.vol"))
    args = ["--i1", f["v1"], "--i2", f["v"], "--mask1", f["m1"], "--mask2", f["m2"], "-o", out, "--sub", "--radavg", "--cutFreq", str(CUT), "--saveV1", s1, "--saveV2", s2]
    args += ["--maskSub", f["msub"]] if own_mask else ["--sigma", "3"]
    _program(args)
    adj = ref_adjust(shape, 5, True, CUT)["adjusted"]
    msub = np.roll(mask, 2, axis=2) if own_mask else R.smooth_mask(mask, 3)
    exp, v1f = R.subtraction(v1, adj, msub, CUT)
    assert _close(s2, adj, shape) and _close(s1, v1f, shape) and _close(out, exp, shape)
    assert np.abs(exp - v1).max() > 1e-2
