"""GPU parity of xmipp_resolution_monogenic_signal (xh_mono_*, MonoRes in api.py) against the numpy fp64 restatement of the reference
(tests/monores_ref.py): the monogenic amplitude of one frequency, the per-shell sums, the one-rank select, the statistics, the assign
step, and the program end to end. Volumes are seeded synthetic ones: blobs with a texture low-passed to two local resolutions, zero
beyond a sphere, plus Gaussian noise inside a larger sphere; half maps are the same signal with independent noise.

The stages whose kernels choose a tile from the size (amplitude, Gaussian filter, shell sums, statistics, select) also run at the shapes of
tests/volume_tiles.py, where they leave the tile of the small shapes; the end-to-end sweep stays at 32^3."""
import os
import subprocess

import numpy as np
import pytest

from tests import monores_ref as R
from tests import volume_tiles as T
from tests import xmipp_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "xmipp3_amd", "bin", "xmipp_resolution_monogenic_signal")
SMALL = [(24, 20, 18), (21, 21, 21)]
# where the stages that depend on the size leave the tile of SMALL (tests/volume_tiles.py, asserted by tests/test_volume_tiles.py):
# POW2_X the bit-reversed placement of k_mn_rows_amp; X160 and X300 its rpb = 2 (with a tail workgroup) and 1; Z130 the z line pass at
# 64 KiB of LDS. BIG takes every grid-stride loop into another lap; it has tests of its own, one frequency and one sigma
STAGE_SHAPES = SMALL + [T.POW2_X, T.X160, T.X300, T.Z130]
BIG = T.BIG


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


def noisy_map(shape, seed):
    return R.synth_map(shape, seed) + np.random.default_rng(seed + 50).standard_normal(shape) * 0.2


# ---------------------------------------------------------------- amplitude
_AMP_IN = {}


def _amp_input(shape):
    if shape not in _AMP_IN:
        v = noisy_map(shape, 5)
        _AMP_IN[shape] = (v, np.fft.rfftn(v) / float(v.size))
    return _AMP_IN[shape]


def _plane_error(got, exp):
    """the largest |got - exp| of a z plane over that plane's maximum of the restatement"""
    return max(float(np.abs(got[k] - exp[k]).max() / np.abs(exp[k]).max()) for k in range(exp.shape[0]))


@pytest.mark.parametrize("shape", STAGE_SHAPES)
@pytest.mark.parametrize("freq", [0.015, 0.25, 0.49])      # freqH clips to 0, the middle, freqL clips to 0.5
def test_amplitude_of_one_frequency(gpu, shape, freq):
    _check_amplitude(gpu, shape, freq)


def _check_amplitude(gpu, shape, freq):
    xa, ctx, torch = gpu
    v, F = _amp_input(shape)
    freqL, freqH = min(freq + 0.02, 0.5), max(freq - 0.02, 0.0)
    assert (freqH == 0.0) == (freq == 0.015) and (freqL == 0.5) == (freq == 0.49)
    exp = R.amplitude_lpf(F, shape, freq, freqH, freqL)
    m = xa.MonoRes(ctx, shape)
    got = m.amplitude(torch.from_numpy(v).cuda(), freq, freqH, freqL, True).cpu().numpy()
    err = _plane_error(got, exp)
    print(f"amplitude {shape} freq {freq}: plane error {err:.3e}")
    assert err <= 1e-10


@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_amplitude_unbanded(gpu, shape):
    _check_amplitude_unbanded(gpu, shape)


def _check_amplitude_unbanded(gpu, shape):
    xa, ctx, torch = gpu
    v, F = _amp_input(shape)
    exp = R.monogenic_amplitude_3d_fourier(F, shape)
    got = xa.MonoRes(ctx, shape).amplitude(torch.from_numpy(v).cuda(), 0, 0, 0, False).cpu().numpy()
    err = _plane_error(got, exp)
    print(f"unbanded amplitude {shape}: plane error {err:.3e}")
    assert err <= 1e-10


@pytest.mark.parametrize("shape", STAGE_SHAPES)
@pytest.mark.parametrize("sigma", [3.0, 4.0])
def test_gaussian_filter(gpu, shape, sigma):
    _check_gaussian_filter(gpu, shape, sigma)


def _check_gaussian_filter(gpu, shape, sigma):
    xa, ctx, torch = gpu
    v, _ = _amp_input(shape)
    exp = R.real_gaussian_filter(v, sigma)
    got = xa.MonoRes(ctx, shape).gaussian(torch.from_numpy(v).cuda(), sigma).cpu().numpy()
    print(f"gaussian {shape} sigma {sigma}: error {np.abs(got - exp).max() / np.abs(exp).max():.3e} of the maximum")
    assert np.abs(got - exp).max() <= 1e-10 * np.abs(exp).max()


@pytest.fixture(scope="module")
def big(gpu):
    """BIG has more half-spectrum elements than the grid cap has threads: k_mn_split, k_mn_lowpass and k_mn_gauss take a second lap over
    NF; the loops over the N voxels (k_mn_stats, k_mn_sel_pass with its run-length carried from lap to lap) a third"""
    xa, ctx, torch = gpu
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t = T.tiling(BIG)
    print(f"{BIG}: {t.NF} half-spectrum elements, {t.N} voxels on {cus} CUs, grid cap {256 * 4 * cus} threads")
    assert t.NF > 256 * 4 * cus, f"{t.NF} half-spectrum elements do not exceed the grid cap of {256 * 4 * cus} threads on {cus} CUs"
    return BIG


def test_amplitude_past_the_grid_cap(gpu, big):
    _check_amplitude(gpu, big, 0.25)


def test_amplitude_unbanded_past_the_grid_cap(gpu, big):
    _check_amplitude_unbanded(gpu, big)


def test_gaussian_filter_past_the_grid_cap(gpu, big):
    _check_gaussian_filter(gpu, big, 3.0)


# ---------------------------------------------------------------- per-shell sums
# T.SHELLS has 262 shells: a thread of k_mn_shell_planes takes two (r += 256) and k_mn_shell_final runs in several workgroups. With Rzero
# below X / 2 the cliff assertion applies, but the shells beyond Rzero sum zeros: T.SHELLS also runs with no voxel cut (Rzero beyond the
# box), so that the shells of a thread's second lap (r >= 256) carry sums that are compared
@pytest.mark.parametrize("shape,Rzero", [((21, 21, 21), 8), ((24, 24, 24), 10), ((24, 20, 18), 7), (T.BIG, 30), (T.SHELLS, 4), (T.SHELLS, 300)])
def test_shell_sums_and_cliff_radius(gpu, shape, Rzero):
    xa, ctx, torch = gpu
    v = noisy_map(shape, 9)
    v[R.r2_map(shape) >= Rzero * Rzero] = 0.0
    es, es2, en = R.shell_sums(v)
    ea, ea2, _ = R.shell_sums(np.abs(v))
    m = xa.MonoRes(ctx, shape)
    assert m.info()["nshell"] == T.tiling(shape).nshell
    s, s2, n = m.shell_sums(torch.from_numpy(v).cuda())
    k = es.size
    assert np.array_equal(n[:k], en) and not n[k:].any() and not s[k:].any()         # counts exact
    live = ea > 0
    if Rzero * Rzero > R.r2_map(shape).max():
        assert live.all() and k > 256 and en[256:].sum() > 50          # nothing was cut: every shell has terms, the second lap's included
    print(f"shell sums {shape} Rzero {Rzero}: {n.size} shells, {int(live.sum())} with terms, largest error of a shell's terms: sum "
          f"{np.max(np.abs(s[:k] - es)[live] / ea[live]):.3e}, sum of squares {np.max(np.abs(s2[:k] - es2)[live] / ea2[live]):.3e}")
    assert np.all(np.abs(s[:k] - es) <= 1e-10 * ea) and np.all(np.abs(s2[:k] - es2) <= 1e-10 * ea2)
    assert int(n.sum()) == v.size
    lim = xa.mono_cliff_radius(s, s2, n, 3, shape[2])
    assert lim == R.cliff_radius(es, es2, en, 3, shape[2])
    if shape[2] // 2 > Rzero:
        assert lim == Rzero - 1


# ---------------------------------------------------------------- select
def _select_arrays():
    rng = np.random.default_rng(11)
    n = 7 * 9 * 11                                          # 693: not a multiple of the workgroup size
    a = rng.standard_normal(n)
    a[::5] = 0.0                                            # zeros
    a[1::7] = a[1]                                          # ties
    a[2::9] = -a[2::9] * 1e-300                             # tiny values of both signs
    big = rng.standard_normal(21 * 21 * 21) * np.exp(rng.uniform(-30, 30, 21 * 21 * 21))
    return {"mixed": a, "constant": np.full(n, -2.5), "negative": -np.abs(rng.standard_normal(n)) - 1.0, "wide": big,
            "two": np.array([3.0, -1.0])}


@pytest.mark.parametrize("name", ["mixed", "constant", "negative", "wide", "two"])
def test_select_is_an_element_of_the_sorted_input(gpu, name):
    xa, ctx, torch = gpu
    a = _select_arrays()[name]
    m = xa.MonoRes(ctx, (21, 21, 21))
    d = torch.from_numpy(a).cuda()
    srt = np.sort(a)
    for rank in sorted({0, 1 % a.size, a.size // 3, int(a.size * 0.95), int(a.size * 0.5), a.size - 1}):
        got = m.select(d, rank)
        assert np.float64(got).tobytes() == srt[rank].tobytes(), (name, rank, got, srt[rank])
    with pytest.raises(xa.XhError):
        m.select(d, a.size)                                 # a rank beyond the set is refused


def test_select_counts_only_the_set(gpu):
    xa, ctx, torch = gpu
    a = _select_arrays()["mixed"]
    rng = np.random.default_rng(12)
    m = xa.MonoRes(ctx, (7, 9, 11))
    d = torch.from_numpy(a).cuda()
    mask = (rng.uniform(size=a.size) < 0.3).astype(np.int32)
    srt = np.sort(a[mask != 0])
    for rank in (0, srt.size // 2, int(srt.size * 0.95), srt.size - 1):
        assert m.select(d, rank, torch.from_numpy(mask).cuda()) == srt[rank]
    one = np.zeros(a.size, np.int32)                         # a set of one element
    one[400] = 1
    assert m.select(d, 0, torch.from_numpy(one).cuda()) == a[400]
    with pytest.raises(xa.XhError):
        m.select(d, 1, torch.from_numpy(one).cuda())
    with pytest.raises(xa.XhError):
        m.select(d, 0, torch.from_numpy(np.zeros(a.size, np.int32)).cuda())


@pytest.mark.parametrize("masked", [False, True])
def test_select_past_the_grid_cap(gpu, big, masked):
    """531 360 values drawn as "wide" is: a thread of k_mn_sel_pass takes a third lap over them and carries its run of equal digits
    (last, cnt) from one lap into the next. The mask drops about half. One rank lies inside a planted run of 4096 equal values"""
    xa, ctx, torch = gpu
    rng = np.random.default_rng(13)
    n = T.tiling(big).N
    a = rng.standard_normal(n) * np.exp(rng.uniform(-30, 30, n))
    planted = 0.37
    a[100000:104096] = planted
    mask = (rng.uniform(size=n) < 0.5).astype(np.int32) if masked else None
    srt = np.sort(a if mask is None else a[mask != 0])
    first, run = int(np.searchsorted(srt, planted, "left")), int((srt == planted).sum())
    assert run == 4096 if mask is None else 1500 < run < 2600
    assert 0.4 * n < srt.size < 0.6 * n if masked else srt.size == n
    inside = first + run // 2
    assert 0 < first and inside + 1 < srt.size and srt[inside] == planted
    m = xa.MonoRes(ctx, big)
    d = torch.from_numpy(a).cuda()
    dm = None if mask is None else torch.from_numpy(mask).cuda()
    for rank in (0, srt.size // 2, srt.size - 1, inside):
        got = m.select(d, rank, dm)
        assert np.float64(got).tobytes() == srt[rank].tobytes(), (rank, got, srt[rank])
    with pytest.raises(xa.XhError):
        m.select(d, srt.size, dm)


# ---------------------------------------------------------------- statistics
@pytest.mark.parametrize("shape", [(21, 21, 21), (24, 20, 18), T.BIG])
@pytest.mark.parametrize("halves", [False, True])
def test_statistics(gpu, shape, halves):
    xa, ctx, torch = gpu
    rng = np.random.default_rng(21)
    ampS = rng.standard_normal(shape) + 0.5                  # the low-passed amplitude can be negative
    ampN = rng.standard_normal(shape) * 0.3 + 0.1
    mask = rng.integers(-1, 3, size=shape).astype(np.int32)  # -1, 0, 1, 2
    exp = R.statistics(ampS, ampN if halves else ampS, mask, 0.95, halves)
    m = xa.MonoRes(ctx, shape)
    got = m.statistics(torch.from_numpy(ampS).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(ampN).cuda() if halves else None, 0.95)
    assert got["NS"] == exp["NS"] and got["NN"] == exp["NN"]
    sig, noi = mask >= 1, (mask >= 0) if halves else (mask == 0)
    vN = ampN if halves else ampS
    for key, terms in (("sumS", ampS[sig]), ("sumS2", ampS[sig] ** 2), ("sumN", vN[noi]), ("sumN2", vN[noi] ** 2)):
        print(f"statistics {shape} halves {halves} {key}: error {abs(got[key] - exp[key]) / np.abs(terms).sum():.3e} of the terms")
        assert abs(got[key] - exp[key]) <= 1e-10 * np.abs(terms).sum(), key
    assert got["thr95"] == exp["thr95"]
    for key in ("meanS", "meanN", "sdS2", "sdN2"):
        assert abs(got[key] - exp[key]) <= 1e-10 * max(1.0, abs(exp[key]))


def test_statistics_refuses_an_empty_noise_set(gpu):
    xa, ctx, torch = gpu
    shape = (8, 8, 8)
    m = xa.MonoRes(ctx, shape)
    a = torch.ones(shape, dtype=torch.float64, device="cuda")
    with pytest.raises(xa.XhError, match="noise set is empty"):
        m.statistics(a, torch.ones(shape, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------- assign
@pytest.mark.parametrize("halves", [False, True])
def test_assign_three_calls(gpu, halves):
    xa, ctx, torch = gpu
    rng = np.random.default_rng(31)
    n = 5000
    m = xa.MonoRes(ctx, (21, 21, 21))
    mask = rng.integers(-1, 3, size=n).astype(np.int32)
    res = np.zeros(n)
    dm, dr = torch.from_numpy(mask.copy()).cuda(), torch.from_numpy(res.copy()).cuda()
    resolutions = [10.0, 8.0, 6.4]
    dropped = 0
    for it, resolution in enumerate(resolutions):
        amp = rng.standard_normal(n)
        amp[::11] = 0.3                                       # voxels exactly at the threshold fail it (>)
        r2 = resolutions[0] if it < 2 else resolutions[it - 2]
        before = mask.copy()
        R.set_local_resolution(amp, mask, res, 0.3, resolution, r2, halves)
        dropped += int(((before == 2) & (mask == (0 if halves else -1))).sum())
        m.assign(torch.from_numpy(amp).cuda(), dm, dr, 0.3, resolution, r2, halves)
        assert np.array_equal(dm.cpu().numpy(), mask) and np.array_equal(dr.cpu().numpy(), res)
    assert dropped > 100 and len(np.unique(res)) >= 3


# ---------------------------------------------------------------- end to end
SHAPE = (32, 32, 32)
R_PROT, R_NOISE = 9, 14
CASES = {
    "single": dict(halves=False),
    "single_gaussian": dict(halves=False, gaussian=True),
    "halves": dict(halves=True),
    "halves_gaussian": dict(halves=True, gaussian=True),
    "single_maskexcl": dict(halves=False, excl=True),
    "halves_noiseonly": dict(halves=True, noiseOnlyInHalves=True),
}
_E2E = {}


def e2e_inputs(name, shape=SHAPE, r_prot=R_PROT, r_noise=R_NOISE):
    c = CASES[name]
    seed = 1
    sig = R.synth_map(shape, seed)
    sig[R.r2_map(shape) > r_prot * r_prot] = 0.0
    if c["halves"]:
        v1 = sig + R.noise_in_sphere(shape, seed + 100, 0.21, r_noise)
        v2 = sig + R.noise_in_sphere(shape, seed + 200, 0.21, r_noise)
    else:
        v1, v2 = sig + R.noise_in_sphere(shape, seed + 100, 0.15, r_noise), None
    mask = R.protein_mask(shape, r_prot)
    excl = None
    if c.get("excl"):
        excl = np.zeros(shape, np.int32)
        excl[10:16, 12:20, 14:22] = 1
    # what the program reads from files: float32 values
    v1 = v1.astype(np.float32).astype(np.float64)
    v2 = None if v2 is None else v2.astype(np.float32).astype(np.float64)
    kw = dict(sampling=1.0, maxRes=10.0, freq_step=0.25, significance=0.95, gaussian=bool(c.get("gaussian")), noiseOnlyInHalves=bool(c.get("noiseOnlyInHalves")))
    return v1, v2, mask, excl, kw


def e2e_reference(name):
    """the restatement's run, computed once per case and left unchanged"""
    if name not in _E2E:
        v1, v2, mask, excl, kw = e2e_inputs(name)
        _E2E[name] = R.run(v1, mask, vol2=v2, mask_excl=excl, **kw)
    return _E2E[name]


def marginal_voxels(ref, sampling=1.0, maxRes=10.0):
    """voxels some comparison of the restatement decided within 1e-9 relative of the compared value"""
    m = np.zeros(SHAPE, bool)
    if "refine_amplitude" in ref:
        a = ref["refine_amplitude"]
        m |= (ref["mask_side"] >= 1) & (np.abs(a - ref["refine_threshold"]) <= 1e-9 * a.max())
    for s in ref["steps"]:
        if s["assigned"]:
            m |= (s["mask_before"] >= 1) & (np.abs(s["ampS"] - s["threshold"]) <= 1e-9 * s["ampS"].max())
    inside = ref["refined_mask"] > 0
    sm, res = ref["post_smooth"], ref["res_raw"]
    m |= inside & ((np.abs(sm - res) <= 1e-9 * maxRes) | (np.abs(sm - 2 * sampling) <= 1e-9 * maxRes))
    return m


def device_run(gpu, name):
    xa, ctx, torch = gpu
    v1, v2, mask, excl, kw = e2e_inputs(name)
    m = xa.MonoRes(ctx, SHAPE)
    return m.run(torch.from_numpy(v1).cuda(), torch.from_numpy(mask).cuda(), vol2=None if v2 is None else torch.from_numpy(v2).cuda(),
                 mask_excl=None if excl is None else torch.from_numpy(excl).cuda(), sampling=kw["sampling"], max_res=kw["maxRes"], step=kw["freq_step"],
                 significance=kw["significance"], gaussian=kw["gaussian"], noise_only_in_halves=kw["noiseOnlyInHalves"])


@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end(gpu, name):
    ref = e2e_reference(name)
    steps = ref["steps"]
    # ---- what the restatement itself must hold for the comparison to mean something
    marg = marginal_voxels(ref)
    in_noise_sphere = int((R.r2_map(SHAPE) < ref["radiuslimit"] ** 2).sum())
    assert marg.sum() <= 0.005 * in_noise_sphere
    cz = ref["criticalZ"]
    for s in steps:
        assert abs(s["NS"] / ref["nvoxels"] - 0.025) > 1e-6 * 0.025
        if s["NS"] / ref["nvoxels"] >= 0.025 and s["NS"] > 0:
            assert abs(s["meanS"] - 0.001 * s["max_meanS"]) > 1e-6 * abs(s["meanS"])
        if s["assigned"]:
            assert abs(s["z"] - cz) > 1e-6 * cz
    assert len(steps) >= 6
    assert len(np.unique(ref["res_raw"][ref["res_raw"] != 0])) >= 3
    drop = 0 if CASES[name]["halves"] else -1
    assert sum(int(((s["mask_before"] == 2) & (s["mask_after"] == drop)).sum()) for s in steps if s["assigned"]) >= 1
    # ---- the device against it
    out = device_run(gpu, name)
    assert out["radius"] == ref["radius"] and out["radiuslimit"] == ref["radiuslimit"] and out["nvoxels"] == ref["nvoxels"]
    assert [s["resolution"] for s in out["steps"]] == ref["resolutions"]
    assert out["stop"] == ref["stop"]
    for g, e in zip(out["steps"], steps):
        assert g["NN"] == e["NN"] and g["assigned"] == e["assigned"]
        if not marg.any():
            assert g["NS"] == e["NS"]
            assert abs(g["threshold"] - e["threshold"]) <= 1e-9 * abs(e["threshold"])
            assert abs(g["meanS"] - e["meanS"]) <= 1e-9 * abs(e["meanS"]) and abs(g["z"] - e["z"]) <= 1e-7 * max(1.0, abs(e["z"]))
    ok = ~marg
    assert np.array_equal(out["refined_mask"].cpu().numpy()[ok], ref["refined_mask"][ok])
    for key in ("chimera", "resolution_map"):
        got, exp = out[key].cpu().numpy(), ref[key]
        err = np.abs(got - exp)[ok] / np.maximum(np.abs(exp)[ok], 1e-3 * np.abs(exp).max())
        print(f"{name} {key}: relative error {err.max():.3e}, marginal voxels {int(marg.sum())}")
        assert err.max() <= 1e-9
    if CASES[name]["halves"]:
        assert np.array_equal(out["mean"].cpu().numpy(), ref["mean"])
    else:
        assert out["mean"] is None


def test_two_runs_give_the_same_bytes(gpu):
    for name in ("single", "halves"):
        a, b = device_run(gpu, name), device_run(gpu, name)
        for key in ("refined_mask", "chimera", "resolution_map"):
            assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), (name, key)
        assert a["steps"] == b["steps"] and a["stop"] == b["stop"]


def test_timed_run_changes_no_byte(gpu):
    """set_timing(True) records events around the stages and reads them after the step's own wait: the maps and the records keep their
    bytes and the seven stages report times (every step of this sweep assigns, the restatement says). run resets the times,
    set_timing does not"""
    xa, ctx, torch = gpu
    shape = SMALL[0]
    v1, _, mask, _, kw = e2e_inputs("single", shape, 5, 8)
    ref = R.run(v1, mask, **kw)
    assert len(ref["steps"]) >= 6 and all(s["assigned"] for s in ref["steps"])
    dv, dm = torch.from_numpy(v1).cuda(), torch.from_numpy(mask).cuda()
    m = xa.MonoRes(ctx, shape)
    keys = ("refined_mask", "chimera", "resolution_map")

    def run():
        out = m.run(dv, dm, sampling=kw["sampling"], max_res=kw["maxRes"], step=kw["freq_step"], significance=kw["significance"])
        return [out[k].cpu().numpy().tobytes() for k in keys], out["steps"], out["stop"]

    out = run()
    assert len(out[1]) == len(ref["steps"])
    assert set(m.stage_ms().values()) == {0.0}                  # an untimed run reports nothing
    m.set_timing(True)
    out_t = run()
    ms = m.stage_ms()
    print(f"stage ms: {ms}")
    assert out_t == out
    assert list(ms) == list(xa.MonoRes.STAGES) and len(ms) == 7
    assert all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
    m.set_timing(False)
    assert m.stage_ms() == ms                                   # the switch alone resets nothing
    assert run() == out
    assert set(m.stage_ms().values()) == {0.0}
    m.close()


def _wrong_tensors(torch, shape, good):
    """what a volume handle refuses in place of `good`: another shape, another type, a view that is not contiguous"""
    Z, Y, X = shape
    other = torch.float32 if good.dtype == torch.float64 else torch.float64
    return {"shape": torch.zeros((Z, Y, X - 2), dtype=good.dtype, device="cuda"), "type": good.to(other),
            "view": torch.zeros((Z, Y, 2 * X), dtype=good.dtype, device="cuda")[:, :, ::2]}


def test_wrong_tensor_is_refused(gpu):
    """a tensor of another shape or type, or one that is not contiguous, is an XhError before its pointer reaches the library: for the
    volumes, and for the int32 masks, which a float64 tensor of the right shape is not"""
    xa, ctx, torch = gpu
    shape = SMALL[0]
    v1, _, mask, _, _ = e2e_inputs("single", shape, 5, 8)
    dv, dm = torch.from_numpy(v1).cuda(), torch.from_numpy(mask).cuda()
    m = xa.MonoRes(ctx, shape)
    for what, bad in _wrong_tensors(torch, shape, dv).items():
        assert tuple(bad.shape) == shape or what == "shape"
        with pytest.raises(xa.XhError, match="MonoRes: the volume"):
            m.run(bad, dm, max_res=10.0)
        with pytest.raises(xa.XhError, match="MonoRes: the second half"):
            m.run(dv, dm, vol2=bad, max_res=10.0)
        with pytest.raises(xa.XhError, match="MonoRes: the volume"):
            m.amplitude(bad, 0.25, 0.2, 0.3)
        with pytest.raises(xa.XhError, match="MonoRes: the volume"):
            m.gaussian(bad, 3.0)
        with pytest.raises(xa.XhError, match="MonoRes: the volume"):
            m.shell_sums(bad)
    for what, bad in _wrong_tensors(torch, shape, dm).items():
        with pytest.raises(xa.XhError, match="MonoRes: the mask"):
            m.run(dv, bad, max_res=10.0)
        with pytest.raises(xa.XhError, match="MonoRes: the exclusion mask"):
            m.run(dv, dm, mask_excl=bad, max_res=10.0)
        with pytest.raises(xa.XhError, match="MonoRes: the mask"):
            m.statistics(dv, bad)
    with pytest.raises(xa.XhError, match="int32"):
        m.run(dv, dv, max_res=10.0)
    m.close()


def test_refusals(gpu):
    xa, ctx, torch = gpu
    v1, _, mask, _, _ = e2e_inputs("single")
    m = xa.MonoRes(ctx, SHAPE)
    dv = torch.from_numpy(v1).cuda()
    with pytest.raises(xa.XhError, match="no voxel equal to 1"):
        m.run(dv, torch.zeros(SHAPE, dtype=torch.int32, device="cuda"), max_res=10.0)
    # a mask that covers the whole noise sphere leaves no noise voxel
    with pytest.raises(xa.XhError, match="noise set"):
        m.run(dv, torch.ones(SHAPE, dtype=torch.int32, device="cuda"), max_res=10.0)


def _read_mrc(path):
    h = np.fromfile(path, np.int32, 256)
    assert h[3] == 2
    return np.fromfile(path, np.float32, offset=1024).reshape(h[2], h[1], h[0])


@pytest.mark.parametrize("name", ["halves", "single_maskexcl"])
def test_program_writes_what_the_api_returns(gpu, tmp_path, name):
    v1, v2, mask, excl, kw = e2e_inputs(name)
    out = device_run(gpu, name)
    xmipp_io.write_mrcs(str(tmp_path / "v1.mrc"), v1)
    xmipp_io.write_mrcs(str(tmp_path / "mask.mrc"), mask)
    args = ["--vol", str(tmp_path / "v1.mrc"), "--mask", str(tmp_path / "mask.mrc"), "-o", str(tmp_path), "--minRes", "30", "--maxRes", "10",
            "--sampling_rate", "1", "--threads", "3"]
    if v2 is not None:
        xmipp_io.write_mrcs(str(tmp_path / "v2.mrc"), v2)
        args += ["--vol2", str(tmp_path / "v2.mrc")]
    if excl is not None:
        xmipp_io.write_mrcs(str(tmp_path / "excl.mrc"), excl)
        args += ["--maskExcl", str(tmp_path / "excl.mrc")]
    r = subprocess.run([PROG] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    printed = [float(l.split("=")[1]) for l in r.stdout.splitlines() if l.startswith("resolution = ")]
    assert len(printed) == len(out["steps"]) and np.allclose(printed, [s["resolution"] for s in out["steps"]], rtol=1e-5)
    files = {"refinedMask.mrc": out["refined_mask"], "monoresResolutionChimera.mrc": out["chimera"], "monoresResolutionMap.mrc": out["resolution_map"]}
    if v2 is not None:
        files["meanMap.mrc"] = out["mean"]
    else:
        assert not (tmp_path / "meanMap.mrc").exists()
    for fn, t in files.items():
        assert np.array_equal(_read_mrc(str(tmp_path / fn)), t.cpu().numpy().astype(np.float32)), fn
