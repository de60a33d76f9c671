"""GPU checks of the real-space ray projector (xh_rsp), of the subtraction pipeline (xh_sub) and of xmipp_subtract_projection against
the numpy restatements in tests/subtract_projection_ref.py (reference libraries/data/projection.cpp:337-589 and
libraries/reconstruction/subtract_projection.cpp).

Values are held to 1e-10 x the plane's maximum: a pixel is a sum of at most about 3 D products whose alpha carry a few ulp, and a
near-tie between two diffs moves a term of weight about 0. The support (and > 0) is not continuous: outside the restatement's
marginal pixels it must match exactly, the marginal pixels may be at most 2 % of an image, and the orientations with an exact Euler
matrix exempt nothing.

The pipeline's planes (P, Pctf, Idiff) are held to 1e-10 x the plane's maximum (P on the Fourier path: 1e-9, the bound
test_gpu_continuous_assign2 holds the projector to), its masks exactly on inputs without a marginal pixel, the sums of the fit to
1e-10 x the sum of their terms' magnitudes, and b, the betas and R2 to 1e-8 relative after the restatement has asserted
cond(A1) <= 1e6 and |R21adj - R20adj| >= 1e-6: the restatement feeds its own sums to the same host fit.

At D = 16 and 17 every grid-stride loop of xh_sub.hip runs one lap, k_sub_fit one workgroup and rsp_run one chunk. The shapes that leave
that case are listed in tests/subtract_shapes.py, which restates the loop lengths and launch sizes and asserts (without a device, in
tests/test_subtract_shapes.py) that each shape reaches its path; the bounds above hold unchanged at all of them:
  D = 22, 40        the second lap of k_sub_models (264 half-spectrum cells; 840: three laps and a tail of 72) and up to seven laps of
                    both loops of k_sub_prepare (D D = 1600), on both projectors, with an ROI mask and a --mask volume
  D = 41            a padded size of 81 = 3^4 in fftP (the other sizes pad to 31, 43, 79 and 3 x 11)
  D = 168           a wi bin of 269 cells, the second lap of k_sub_bins; padding 1, so fftP has 168 = 2^3 3 7 points. The sums are the
                    closest figure of the file, 6.3e-11 of their magnitudes against 1e-10: the last bin (wi = 118, 3 cells) lies seven
                    orders below the largest cell of the spectrum, and a transform's rounding scales with the whole spectrum. The
                    restatement's own share, against long double transforms of the same images, is 3.8e-11
  65 particles      one chunk of 65: two workgroups of k_sub_fit, 17 of k_sub_translate (p = t / D up to 64), blockIdx.y = 64 in
                    k_sub_bins; against chunks of 64 and 1. 6 of the 65 choose model 1, under an ROI mask (DC cell from F[2 plane])
  boost, no ROI     particles that choose model 1: the y inv / t1 branch of k_sub_spectrum
  a timed run       the events of SUB_MARK change no byte
  4099 projections  the second chunk of rsp_run (d_out + 4096 D D, the re-uploaded parameter block), then a short call on the same handle"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import subtract_projection_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


def _cases(oracle, n_generic):
    """(angles, offset or None, exact) for every orientation, each without and with the offset"""
    out = []
    for exact, angs in ((True, ref.EXACT_ANGLES), (False, ref.generic_angles(n_generic))):
        for a in angs:
            out.append((a, None, exact))
            out.append((a, ref.OFFSET, exact))
    return out


def _volumes(D):
    rng = np.random.default_rng(100 + D)
    blob = ref.blob_mask(D)
    return {"random": rng.standard_normal((D, D, D)), "blob": blob, "sparse": rng.random((D, D, D)) * blob}


_REF = {}


def _reference(oracle, D, name, n_generic):
    """the restatement of every case of one volume, computed once and shared"""
    key = (D, name, n_generic)
    if key not in _REF:
        vol = _volumes(D)[name]
        _REF[key] = [ref.project_volume(vol, oracle.euler_matrix(*a), off) for a, off, _ in _cases(oracle, n_generic)]
        for r in _REF[key]:
            for x in r:
                x.setflags(write=False)
    return _REF[key]


def _project(gpu, vol, mode, cases):
    """all cases of one handle: the rows with an offset and those without are two calls (null offsets are their own path)"""
    xa, ctx, torch = gpu
    rp = xa.RealSpaceProjector(ctx, torch.from_numpy(np.ascontiguousarray(vol)).cuda(), mode)
    out = [None] * len(cases)
    for with_off in (False, True):
        sel = [k for k, c in enumerate(cases) if (c[1] is not None) == with_off]
        got = rp.project([cases[k][0] for k in sel], [cases[k][1] for k in sel] if with_off else None).cpu().numpy()
        for k, g in zip(sel, got):
            out[k] = g
    packed = rp.packed
    rp.close()
    return out, packed


@pytest.mark.parametrize("D,n_generic", [(16, 4), (17, 4), (33, 1)])
@pytest.mark.parametrize("name", ["random", "blob"])
def test_ray_projector_values(gpu, oracle, D, n_generic, name):
    cases = _cases(oracle, n_generic)
    exp = _reference(oracle, D, name, n_generic)
    got, _ = _project(gpu, _volumes(D)[name], "value", cases)
    for (a, off, _), (plane, _, _), g in zip(cases, exp, got):
        top = np.abs(plane).max()
        assert top > 0
        err = np.abs(g - plane).max()
        print(f"D {D} {name} angles {a} offset {off}: max err {err:.3e} of max {top:.3e}")
        assert err <= 1e-10 * top, (a, off, err, top)


@pytest.mark.parametrize("D,n_generic", [(16, 4), (17, 4), (33, 1)])
@pytest.mark.parametrize("name", ["blob", "sparse"])
def test_ray_projector_support(gpu, oracle, D, n_generic, name):
    cases = _cases(oracle, n_generic)
    exp = _reference(oracle, D, name, n_generic)
    vol = _volumes(D)[name]
    got, packed = _project(gpu, vol, "support", cases)
    val, _ = _project(gpu, vol, "value", cases)
    assert packed, "a volume without negative voxels goes to bits"
    for (a, off, exact), (plane, support, marginal), g, v in zip(cases, exp, got, val):
        assert set(np.unique(g)) <= {0.0, 1.0}
        assert support.any() and not support.all()
        frac = marginal.mean()
        print(f"D {D} {name} angles {a} offset {off}: marginal {marginal.sum()} of {marginal.size}")
        assert frac <= 0.02, (a, off, frac)                     # a condition on the inputs, met by the restatement alone
        keep = np.ones_like(marginal) if exact else ~marginal   # the exact matrices exempt nothing
        assert np.array_equal(g[keep] > 0, support[keep]), (a, off)
        assert np.array_equal(support[keep], plane[keep] > 0), (a, off)       # the equivalence the mode rests on
        assert np.array_equal(g[keep] > 0, v[keep] > 0), (a, off)


@pytest.mark.parametrize("D", [16, 17])
def test_ray_projector_negative_voxel_takes_the_fallback(gpu, oracle, D):
    cases = _cases(oracle, 4)
    vol = ref.blob_mask(D).copy()
    vol[0, 0, 0] = -1.0                                          # a corner the blob does not reach
    got, packed = _project(gpu, vol, "support", cases)
    val, _ = _project(gpu, vol, "value", cases)
    assert not packed
    for g, v in zip(got, val):
        assert np.array_equal(g, (v > 0).astype(np.float64))     # the same walk followed by > 0: no exemption
    # and the corner's rays are seen: some pixel's integral is negative
    assert min(v.min() for v in val) < 0


def test_ray_projector_is_repeatable_and_steps_are_fewer_on_bits(gpu, oracle):
    xa, ctx, torch = gpu
    D = 17
    cases = _cases(oracle, 4)
    vol = _volumes(D)["sparse"]
    a, _ = _project(gpu, vol, "value", cases)
    b, _ = _project(gpu, vol, "value", cases)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                              # no atomics: bit-identical
    dv = torch.from_numpy(vol).cuda()
    ang = [c[0] for c in cases]
    sv = xa.RealSpaceProjector(ctx, dv, "value").steps(ang).cpu().numpy()
    sb = xa.RealSpaceProjector(ctx, dv, "support").steps(ang).cpu().numpy()
    assert sv.min() >= 0 and sv.max() <= 4 * (3 * D + 8)
    assert (sb <= sv).all() and sb.sum() < sv.sum()              # a ray on bits ends at its first hit


def test_ray_projector_errors_are_loud(gpu):
    xa, ctx, torch = gpu
    vol = torch.zeros((8, 8, 8), dtype=torch.float64, device="cuda")
    with pytest.raises(xa.XhError):
        xa.RealSpaceProjector(ctx, vol, "density")
    with pytest.raises(xa.XhError):
        xa.RealSpaceProjector(ctx, vol.float(), "value")
    rp = xa.RealSpaceProjector(ctx, vol, "value")
    with pytest.raises(xa.XhError):
        rp.project([[0.0, float("nan"), 0.0]])
    with pytest.raises(xa.XhError):
        rp.project([[0.0, 0.0, 0.0]], [[0.0, 0.0], [1.0, 1.0]])
    assert rp.project(np.zeros((0, 3))).shape == (0, 8, 8)


# ------------------------------------------------------------------ the subtraction pipeline (xh_sub) against tests/subtract_projection_ref.Subtract
from tests import synth  # noqa: E402
from tests.test_gpu_continuous_assign2 import CTF, ctf_and_envelope  # noqa: E402


def _sub_inputs(oracle, D, n, seed, sign=1.0):
    """a phantom, n noisy shifted projections of it at seeded poses (scaled and offset, so that neither beta nor b is near 0) and their
    rows; every other row has a CTF with its own K"""
    rng = np.random.default_rng(seed)
    # scaled so that the fit's two diagonal terms, sum |PiMFourier|^2 and sum 2 wi, are of one order: a well-conditioned A1
    vol = (50.0 * synth.phantom(D, seed=11, nblobs=9)).astype(np.float32).astype(np.float64)
    fp = oracle.FP(vol, 2.0, 0.5, 3)
    imgs, rows = [], []
    for k, ang in enumerate(ref.generic_angles(n, seed=seed)):
        sh = (0.0, 0.0) if k == 3 else tuple(rng.uniform(-2.5, 2.5, 2))
        A = np.eye(3)
        A[0, 2], A[1, 2] = -sh[0], -sh[1]
        P = oracle.apply_geometry2d(fp.project(*ang), A, 1, False, True)
        img = sign * (1.3 * P + 0.1 * P.std() * rng.standard_normal((D, D)) + 0.4 * P.std())
        imgs.append(img.astype(np.float32))
        row = dict(rot=ang[0], tilt=ang[1], psi=ang[2], shift_x=sh[0], shift_y=sh[1])
        if k % 2 == 0:
            row["ctf"] = dict(CTF, DeltafU=CTF["DeltafU"] + 500.0 * k, K=0.9 + 0.05 * k)
        rows.append(row)
    return vol, np.stack(imgs), rows


def _soft_blob(D):
    z, y, x = np.mgrid[0:D, 0:D, 0:D] - D // 2
    r = np.sqrt(((x - 1.5) / (0.22 * D)) ** 2 + ((y + 2.0) / (0.3 * D)) ** 2 + ((z - 0.5) / (0.18 * D)) ** 2)
    return np.clip(1.5 - r, 0.0, 1.0)


def _sub_pair(gpu, oracle, vol, roi, maskvol, prm, capacity):
    xa, ctx, torch = gpu
    Ts = prm["sampling"]
    res = ref.Subtract(oracle, vol, roi, maskvol, prm, xa.sub_fit, xa.sub_choose, lambda kw, Np: ctf_and_envelope(oracle, kw, Np, Ts)[0])
    h = xa.SubtractProjection(ctx, vol, roi, maskvol, capacity=capacity, **prm)
    assert h.maxwi == res.maxwi and h.a11 == res.a11
    return res, h


def _dev_rows(rows):
    from xmipp3_amd.api import ctf_params
    return [dict(r, ctf=ctf_params(**r["ctf"]) if r.get("ctf") else None) for r in rows]


def _rel(a, b):
    return abs(a - b) / abs(b)


def _check_results(tag, got, exp):
    """b, betas, R2 at 1e-8 relative, after the restatement's own conditions: the fit is well conditioned and the model choice is clear"""
    assert exp["cond"] <= 1e6, (tag, exp["cond"])
    assert exp["R2_gap"] >= 1e-6, (tag, exp["R2_gap"])
    figs = {k: _rel(got[k], exp[k]) for k in ("b", "beta0", "beta00", "R2adj", "R20adj")}
    if exp["model"] == 1:
        figs["beta1"] = _rel(got["beta1"], exp["beta1"])
    print(f"{tag}: model {exp['model']} cond {exp['cond']:.3e} R2 gap {exp['R2_gap']:.3e} relative errors {figs}")
    assert got["model"] == exp["model"] and got["disable"] == int(exp["disable"]) and got["enabled"] == exp["enabled"], tag
    if exp["model"] == 0:
        assert got["beta1"] == 0.0
    for k, v in figs.items():
        assert v <= 1e-8, (tag, k, v)


def _check_planes(tag, got, exp, fourier_path):
    assert not exp["marginal"].any(), tag                       # the inputs are chosen so: the masks are compared exactly
    for k in ("M", "iM", "PmaskImg"):
        assert np.array_equal(got[k], exp[k]), (tag, k)
    for k in ("P", "Pctf", "Idiff"):
        tol = 1e-9 if (k == "P" and fourier_path) else 1e-10    # P on the Fourier path: the bound test_gpu_continuous_assign2 holds it to
        err, top = np.abs(got[k] - exp[k]).max(), np.abs(exp[k]).max()
        print(f"{tag}: {k} max err {err:.3e} of max {top:.3e}")
        assert err <= tol * top, (tag, k, err, top)
    err = np.abs(got["sums"] - exp["sums"])
    bound = 1e-10 * exp["sum_magnitudes"]
    print(f"{tag}: sums worst err / magnitude {np.max(err / np.maximum(exp['sum_magnitudes'], 1e-300)):.3e}")
    assert (err <= bound).all(), (tag, err.max())


@pytest.mark.parametrize("D", [16, 17])
def test_subtract_stages_of_a_chunk(gpu, oracle, D):
    """5 particles at capacity 2: the last chunk ends short. Rows with and without a CTF, with shifts (one without). ROI mask, the disc."""
    vol, imgs, rows = _sub_inputs(oracle, D, 5, 40 + D)
    prm = dict(ref.PRM)
    res, h = _sub_pair(gpu, oracle, vol, ref.blob_mask(D), None, prm, 2)
    exp = [res.process(im, r) for im, r in zip(imgs, rows)]
    h.load(imgs, _dev_rows(rows))
    out, results = h.run()
    _check_planes(f"D {D} particle 4", dict(h.last(0), Idiff=out[4]), exp[4], True)
    with pytest.raises(gpu[0].XhError):
        h.last(1)                                               # the last chunk held one particle
    for i in range(5):
        err, top = np.abs(out[i] - exp[i]["Idiff"]).max(), np.abs(exp[i]["Idiff"]).max()
        assert err <= 1e-10 * top, (i, err, top)
        _check_results(f"D {D} particle {i}", results[i], exp[i])
    # repeatable: no atomics
    out2, results2 = h.run()
    assert out2.tobytes() == out.tobytes() and results2 == results
    # the planes of the other particles: a load of two is one full chunk
    h.load(imgs[:2], _dev_rows(rows[:2]))
    out3, _ = h.run()
    assert out3.tobytes() == out[:2].tobytes()                  # a particle does not depend on what shares its load
    for i in range(2):
        _check_planes(f"D {D} particle {i}", h.last(i), exp[i], True)
    h.close()


VARIANTS = {
    "no_roi": dict(roi=None),
    "subtract": dict(subtract=1),
    "mask_volume": dict(maskvol=True),
    "real_space": dict(real_space=1),
    "ignore_ctf": dict(ignore_ctf=1),
    "boost": dict(boost=1),
    "non_negative_flipped": dict(non_negative=1, sign=-1.0),
    "padding_1": dict(padding=1.0),
    "max_resolution": dict(max_resolution=2.0),
    "soft_roi": dict(roi="soft"),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_subtract_variants(gpu, oracle, name):
    D, v = 16, dict(VARIANTS[name])
    roi = v.pop("roi", "blob")
    roi = {"blob": ref.blob_mask(D), "soft": _soft_blob(D), None: None}[roi]
    maskvol = ref.blob_mask(D, centre=(0.0, 0.0, 0.0), radii=(0.42, 0.4, 0.38)) if v.pop("maskvol", False) else None
    vol, imgs, rows = _sub_inputs(oracle, D, 3, 77, v.pop("sign", 1.0))
    prm = dict(ref.PRM, **v)
    res, h = _sub_pair(gpu, oracle, vol, roi, maskvol, prm, 2)
    exp = [res.process(im, r) for im, r in zip(imgs, rows)]
    h.load(imgs, _dev_rows(rows))
    out, results = h.run()
    _check_planes(f"{name} particle 2", dict(h.last(0), Idiff=out[2]), exp[2], not prm["real_space"])
    for i in range(3):
        err, top = np.abs(out[i] - exp[i]["Idiff"]).max(), np.abs(exp[i]["Idiff"]).max()
        assert err <= 1e-10 * top, (name, i, err, top)
        _check_results(f"{name} particle {i}", results[i], exp[i])
    if name == "non_negative_flipped":
        # every particle leaves disabled: by a negative beta00, or by a negative R2 alone (particle 0, whose CTF row turns the sign back)
        assert all(r["enabled"] == -1 for r in results) and [r["disable"] for r in results] == [int(e["beta00"] < 0) for e in exp]
        assert sorted(r["disable"] for r in results) == [0, 1, 1]
    if name == "ignore_ctf":
        assert np.array_equal(exp[0]["P"], exp[0]["Pctf"])
    h.close()


# ------------------------------------------------------------------ past the 16-pixel case: the shapes of tests/subtract_shapes.py
from tests import subtract_shapes as S  # noqa: E402

MASKVOL = dict(centre=(0.0, 0.0, 0.0), radii=(0.42, 0.4, 0.38))
_SUB_IN, _SUB_REF = {}, {}


def _inputs(oracle, D, n, seed):
    """_sub_inputs, computed once per (D, n, seed) and left unchanged"""
    key = (D, n, seed)
    if key not in _SUB_IN:
        _SUB_IN[key] = _sub_inputs(oracle, D, n, seed)
        for a in _SUB_IN[key][:2]:
            a.setflags(write=False)
    return _SUB_IN[key]


def _expected(key, res, imgs, rows):
    """the restatement of every particle of a case, computed once per case"""
    if key not in _SUB_REF:
        _SUB_REF[key] = [res.process(im, r) for im, r in zip(imgs, rows)]
    return _SUB_REF[key]


def _check_particles(tag, out, results, exp):
    for i, e in enumerate(exp):
        err, top = np.abs(out[i] - e["Idiff"]).max(), np.abs(e["Idiff"]).max()
        print(f"{tag} particle {i}: Idiff max err {err:.3e} of max {top:.3e}")
        assert err <= 1e-10 * top, (tag, i, err, top)
        _check_results(f"{tag} particle {i}", results[i], e)


@pytest.mark.parametrize("real_space", [0, 1])
@pytest.mark.parametrize("D", [S.LAP_MODELS, S.LAPS])
def test_subtract_laps_of_the_model_and_prepare_loops(gpu, oracle, D, real_space):
    """D = 22: the half spectrum has 264 cells, k_sub_models enters its second lap. D = 40: 840 cells (three laps and a tail of 72) and
    D D = 1600 in both loops of k_sub_prepare (six laps and a tail of 64). ROI mask and --mask volume, both projectors; 5 particles at
    capacity 2."""
    assert S.laps(S.half_cells(D))[0] > 1 and S.laps(S.full_cells(D))[0] > 1
    vol, imgs, rows = _inputs(oracle, D, 5, 40 + D)
    prm = dict(ref.PRM, real_space=real_space)
    res, h = _sub_pair(gpu, oracle, vol, ref.blob_mask(D), ref.blob_mask(D, **MASKVOL), prm, 2)
    exp = _expected(("laps", D, real_space), res, imgs, rows)
    h.load(imgs, _dev_rows(rows))
    out, results = h.run()
    tag = f"D {D} real_space {real_space}"
    _check_planes(f"{tag} particle 4", dict(h.last(0), Idiff=out[4]), exp[4], not real_space)
    _check_particles(tag, out, results, exp)
    h.close()


def test_subtract_composite_padded_size(gpu, oracle):
    """D = 41 pads to 81 = 3^4 (the other sizes here pad to primes or to 3 x 11). Fourier path, ROI mask, the disc; 3 particles"""
    D = S.COMPOSITE
    vol, imgs, rows = _inputs(oracle, D, 3, 40 + D)
    res, h = _sub_pair(gpu, oracle, vol, ref.blob_mask(D), None, dict(ref.PRM), 2)
    assert h.padded == S.padded(D) == 81
    exp = _expected(("composite", D), res, imgs, rows)
    h.load(imgs, _dev_rows(rows))
    out, results = h.run()
    _check_planes(f"D {D} particle 2", dict(h.last(0), Idiff=out[2]), exp[2], True)
    _check_particles(f"D {D}", out, results, exp)
    h.load(imgs[:2], _dev_rows(rows[:2]))
    h.run()
    for i in range(2):
        _check_planes(f"D {D} particle {i}", h.last(i), exp[i], True)
    h.close()


def test_subtract_a_bin_past_one_lap(gpu, oracle):
    """D = 168: the largest wi bin has 269 cells, so k_sub_bins enters its second lap (none does below D = 168: 160 stays within 256).
    Padding 1 (a window of 168 = 2^3 3 7) only to keep the restatement short; no ROI, the disc. Two particles at capacity 1, the first
    with a CTF: the sums of each are read through last(0), after the two-chunk run and after a run of particle 0 alone."""
    D = S.BIN
    cells = S.bin_cells(D)
    long_bins = np.nonzero(cells > S.THREADS)[0]
    assert len(long_bins) >= 1 and cells.max() == 269
    vol, imgs, rows = _inputs(oracle, D, 2, 208)
    assert rows[0].get("ctf") and not rows[1].get("ctf")
    res, h = _sub_pair(gpu, oracle, vol, None, None, dict(ref.PRM, padding=1.0), 1)
    assert h.padded == S.padded(D, 1.0) == D and len(cells) == h.maxwi + 1
    exp = _expected(("bin", D), res, imgs, rows)
    for e in exp:
        assert (e["sum_magnitudes"][long_bins] > 0).all()      # the compared sums include the bins of more than 256 cells
        assert (e["sum_magnitudes"][cells > 0] > 0).all()
    h.load(imgs, _dev_rows(rows))
    out, results = h.run()
    _check_planes(f"D {D} particle 1", dict(h.last(0), Idiff=out[1]), exp[1], True)
    _check_particles(f"D {D}", out, results, exp)
    h.load(imgs[:1], _dev_rows(rows[:1]))
    out0, results0 = h.run()
    assert out0.tobytes() == out[:1].tobytes() and results0 == results[:1]
    _check_planes(f"D {D} particle 0", dict(h.last(0), Idiff=out0[0]), exp[0], True)
    h.close()


def test_subtract_a_chunk_of_65(gpu, oracle):
    """65 particles in one chunk: k_sub_fit launches two workgroups, k_sub_translate 17 with p = t / D up to 64, blockIdx.y of k_sub_bins
    reaches 64. At capacity 64 the same load is a chunk of 64 and one of 1: the same bytes. Both models occur, so model 1 is compared
    under an ROI mask, where its DC cell (F[2 plane], the spectrum of (I - b) iM) differs from IFourier(0, 0)."""
    D, n = 16, S.CHUNK_M
    assert S.fit_blocks(n) == 2 and S.fit_blocks(n - 1) == 1
    vol, imgs, rows = _inputs(oracle, D, n, 123)
    roi = ref.blob_mask(D)
    res, h = _sub_pair(gpu, oracle, vol, roi, None, dict(ref.PRM), n)
    exp = _expected(("chunk65", D), res, imgs, rows)
    models = [e["model"] for e in exp]
    print(f"models: {models.count(0)} x 0, {models.count(1)} x 1")
    assert 0 in models and 1 in models
    assert any(e["model"] == 1 and not e["iM"].all() for e in exp)
    h.load(imgs, _dev_rows(rows))
    out, results = h.run()
    _check_particles("capacity 65", out, results, exp)
    for i in range(n):
        _check_planes(f"capacity 65 particle {i}", h.last(i), exp[i], True)
    h.close()
    h = gpu[0].SubtractProjection(gpu[1], vol, roi, None, capacity=n - 1, **ref.PRM)
    h.load(imgs, _dev_rows(rows))
    out2, results2 = h.run()
    assert out2.tobytes() == out.tobytes() and results2 == results
    _check_planes("capacity 64 particle 64", h.last(0), exp[n - 1], True)
    with pytest.raises(gpu[0].XhError):
        h.last(1)
    h.close()


def test_subtract_boost_with_model_1(gpu, oracle):
    """--boost on particles that choose model 1: the branch y inv / t1 of k_sub_spectrum (under an ROI mask the three particles of the
    boost variant all choose model 0). The step divides by T(w) = beta01 + beta1 wi, so the restatement first shows it away from 0."""
    D = 16
    vol, imgs, rows = _inputs(oracle, D, 3, 77)
    res, h = _sub_pair(gpu, oracle, vol, None, None, dict(ref.PRM, boost=1), 2)
    exp = _expected(("boost1", D), res, imgs, rows)
    models = [e["model"] for e in exp]
    assert any(m == 1 for m in models), models
    for i, e in enumerate(exp):
        t1 = np.abs(e["betas"][1] + e["betas"][2] * res.wi).min()
        print(f"boost particle {i}: model {e['model']} min |T1| {t1:.3f}")
        assert t1 >= 0.5, (i, t1)
    h.load(imgs, _dev_rows(rows))
    out, results = h.run()
    assert [r["model"] for r in results] == models
    _check_planes("boost model 1 particle 2", dict(h.last(0), Idiff=out[2]), exp[2], True)
    _check_particles("boost model 1", out, results, exp)
    h.load(imgs[:2], _dev_rows(rows[:2]))
    h.run()
    for i in range(2):
        _check_planes(f"boost model 1 particle {i}", h.last(i), exp[i], True)
    h.close()


def test_subtract_timed_run_changes_no_byte(gpu, oracle):
    """set_timing(True) puts an event before every stage of every chunk: Idiff and the results keep their bytes, and the seven stages
    report times. 5 particles at capacity 2: three chunks, summed."""
    xa = gpu[0]
    D = S.LAP_MODELS
    vol, imgs, rows = _inputs(oracle, D, 5, 40 + D)
    h = xa.SubtractProjection(gpu[1], vol, ref.blob_mask(D), ref.blob_mask(D, **MASKVOL), capacity=2, **ref.PRM)
    h.load(imgs, _dev_rows(rows))
    out, results = h.run()
    assert set(h.stage_ms().values()) == {0.0}                  # an untimed run reports nothing
    h.set_timing(True)
    out_t, results_t = h.run()
    ms = h.stage_ms()
    print(f"stage ms: {ms}")
    assert out_t.tobytes() == out.tobytes() and results_t == results
    assert list(ms) == list(xa.SubtractProjection.STAGES) and len(ms) == 7
    assert all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
    last_t = h.last(0)
    h.set_timing(False)
    out_u, results_u = h.run()
    assert out_u.tobytes() == out.tobytes() and results_u == results
    assert set(h.stage_ms().values()) == {0.0}
    last_u = h.last(0)
    for k in last_u:
        assert last_t[k].tobytes() == last_u[k].tobytes(), k
    h.close()


def _rsp_volume():
    return np.random.default_rng(4099).random((S.RSP_D,) * 3) * ref.blob_mask(S.RSP_D)


def _rsp_reference(oracle, with_off):
    key = ("rsp", with_off)
    if key not in _REF:
        _REF[key] = [ref.project_volume(_rsp_volume(), oracle.euler_matrix(*a), ref.OFFSET if with_off else None) for a in S.rsp_angles()]
        for r in _REF[key]:
            for x in r:
                x.setflags(write=False)
    return _REF[key]


@pytest.mark.parametrize("with_off", [False, True])
def test_ray_projector_two_chunks_of_projections(gpu, oracle, with_off):
    """4099 projections in one call: rsp_run launches 4096 and then 3, the second launch writes from d_out + 4096 D D on and reads a
    re-uploaded parameter block. The rows repeat six orientations, and the seam lies between two of them. Every row is held to the
    restatement of its orientation, in value and in support mode; a call of 3 on the same handle afterwards still answers right."""
    xa, ctx, torch = gpu
    D, n = S.RSP_D, S.RSP_N
    assert S.rsp_chunks(n) == [S.RSP_CHUNK, 3]
    ang6, which = S.rsp_angles(), S.rsp_rows(n)
    exact = [a in ref.EXACT_ANGLES for a in ang6]
    ang = np.array(ang6)[which]
    off = np.tile(np.array(ref.OFFSET), (n, 1)) if with_off else None
    exp = _rsp_reference(oracle, with_off)
    dv = torch.from_numpy(_rsp_volume()).cuda()
    got = {}
    for mode in ("value", "support"):
        rp = xa.RealSpaceProjector(ctx, dv, mode)
        assert rp.packed == (mode == "support")
        got[mode] = rp.project(ang, off).cpu().numpy()
        st = rp.steps(ang, off).cpu().numpy()
        st6 = rp.steps(ang[:6], None if off is None else off[:6]).cpu().numpy()
        assert st6.min() >= 0 and st6.max() > 0
        assert np.array_equal(st, st6[which]), mode
        # the parameter buffer was reserved for 4096: a short call afterwards
        few = rp.project(ang[:3], None if off is None else off[:3]).cpu().numpy()
        assert few.tobytes() == got[mode][:3].tobytes(), mode
        rp.close()
    assert got["value"].shape == (n, D, D)
    for k, (plane, support, marginal) in enumerate(exp):
        v, s = got["value"][k::6], got["support"][k::6]
        assert len(v) in (n // 6, n // 6 + 1)
        top = np.abs(plane).max()
        assert top > 0
        err = np.abs(v - plane).max()
        print(f"offset {with_off} orientation {ang6[k]}: {len(v)} rows, max err {err:.3e} of max {top:.3e}, marginal {marginal.sum()} of {marginal.size}")
        assert err <= 1e-10 * top, (k, err, top)
        assert set(np.unique(s)) <= {0.0, 1.0}
        assert support.any() and not support.all()
        assert marginal.mean() <= 0.02, (k, marginal.mean())   # a condition on the inputs, met by the restatement alone
        keep = np.ones_like(marginal) if exact[k] else ~marginal
        assert np.array_equal(s[:, keep] > 0, np.broadcast_to(support[keep], (len(s), keep.sum()))), k
        assert np.array_equal(support[keep], plane[keep] > 0), k
        assert np.array_equal(s[:, keep] > 0, v[:, keep] > 0), k


def test_subtract_errors_are_loud(gpu, oracle):
    xa, ctx, torch = gpu
    vol = np.zeros((16, 16, 16))
    with pytest.raises(xa.XhError):
        xa.SubtractProjection(ctx, vol, bogus=1)
    with pytest.raises(xa.XhError):
        xa.SubtractProjection(ctx, np.zeros((16, 16, 8)))
    with pytest.raises(xa.XhError):
        xa.SubtractProjection(ctx, vol, roi=np.zeros((8, 8, 8)))
    h = xa.SubtractProjection(ctx, vol, capacity=2)
    with pytest.raises(xa.XhError):
        h.load(np.zeros((1, 16, 12), np.float32), [dict()])     # not square
    with pytest.raises(xa.XhError):
        h.load(np.zeros((1, 8, 8), np.float32), [dict()])       # another size than the volume
    with pytest.raises(xa.XhError):
        h.load(np.zeros((1, 16, 16), np.float32), [dict(rot=float("nan"))])
    with pytest.raises(xa.XhError):
        h.run()                                                 # nothing loaded
    h.close()


# ------------------------------------------------------------------ the program end to end
import os  # noqa: E402
import subprocess  # noqa: E402

from tests import xmipp_io  # noqa: E402

PROG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xmipp3_amd", "bin", "xmipp_subtract_projection")
CTF_LABELS = dict(kV="ctfVoltage", Cs="ctfSphericalAberration", Ca="ctfChromaticAberration", espr="ctfEnergyLoss", Q0="ctfQ0", DeltafU="ctfDefocusU",
                  DeltafV="ctfDefocusV", azimuthal_angle="ctfDefocusAngle", alpha="ctfConvergenceCone", DeltaF="ctfLongitudinalDisplacement",
                  DeltaR="ctfTransversalDisplacement", K="ctfK")


def test_program_end_to_end(gpu, oracle, tmp_path):
    """A volume, an ROI mask, a --mask volume, a stack and an .xmd go in; the output stack (float32) and the four columns (six decimals)
    are held to the restatement: the stack to 1e-10 x its maximum plus half a float32 ulp, a column to 1e-8 relative plus half a unit of
    its last printed decimal. All rows carry a CTF here: the columns are per table. Two runs give the same bytes."""
    xa, ctx, torch = gpu
    D, n = 16, 5
    vol, imgs, rows = _sub_inputs(oracle, D, n, 91)
    for k, r in enumerate(rows):
        r["ctf"] = dict(CTF, DeltafU=CTF["DeltafU"] + 500.0 * k, K=0.9 + 0.05 * k)
    roi = ref.blob_mask(D)
    maskvol = ref.blob_mask(D, centre=(0.0, 0.0, 0.0), radii=(0.42, 0.4, 0.38))
    xmipp_io.write_volume(str(tmp_path / "ref.vol"), vol)
    xmipp_io.write_volume(str(tmp_path / "roi.vol"), roi)
    xmipp_io.write_volume(str(tmp_path / "mask.vol"), maskvol)
    xmipp_io.write_stack(str(tmp_path / "in.stk"), imgs)
    keys = list(CTF_LABELS)
    labels = ["image", "itemId", "angleRot", "angleTilt", "anglePsi", "shiftX", "shiftY"] + [CTF_LABELS[k] for k in keys]
    # poses and CTF go through six printed decimals: the restatement reads what the program reads
    table = []
    for i, r in enumerate(rows):
        for k in ("rot", "tilt", "psi", "shift_x", "shift_y"):
            r[k] = float(f"{r[k]:.6f}")
        table.append([f"{i + 1}@{tmp_path / 'in.stk'}", 100 + i, r["rot"], r["tilt"], r["psi"], r["shift_x"], r["shift_y"]] + [r["ctf"][k] for k in keys])
    xmipp_io.write_xmd(str(tmp_path / "in.xmd"), [("noname", labels, table)])
    prm = dict(ref.PRM, sampling=1.0, max_resolution=2.5)

    def run(name, batch):
        r = subprocess.run([PROG, "-i", str(tmp_path / "in.xmd"), "-o", str(tmp_path / f"{name}.stk"), "--ref", str(tmp_path / "ref.vol"), "--mask_roi",
                            str(tmp_path / "roi.vol"), "--mask", str(tmp_path / "mask.vol"), "--max_resolution", "2.5", "--batch", str(batch), "--save", "x"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return xmipp_io.read_xmd(str(tmp_path / f"{name}.xmd")), xmipp_io.read_stack(str(tmp_path / f"{name}.stk"))

    (lab, out), stack = run("a", 2)
    (lab2, out2), stack2 = run("b", 256)
    assert lab2 == lab and [[v.replace("b.stk", "a.stk") for v in r] for r in out2] == out and stack2.tobytes() == stack.tobytes()
    col = {l: k for k, l in enumerate(lab)}
    for l in labels + ["subtractionR2", "subtractionBeta0", "subtractionBeta1", "subtractionB"]:
        assert l in col, l
    res = ref.Subtract(oracle, vol, roi, maskvol, prm, xa.sub_fit, xa.sub_choose, lambda kw, Np: ctf_and_envelope(oracle, kw, Np, 1.0)[0])
    assert len(out) == n
    for i, r in enumerate(out):
        exp = res.process(imgs[i], rows[i])
        assert not exp["marginal"].any() and exp["cond"] <= 1e6 and exp["R2_gap"] >= 1e-6
        assert r[col["image"]] == f"{i + 1}@{tmp_path / 'a.stk'}" and int(float(r[col["itemId"]])) == 100 + i
        for l, k in (("subtractionR2", "R2adj"), ("subtractionBeta0", "beta0"), ("subtractionBeta1", "beta1"), ("subtractionB", "b")):
            assert abs(float(r[col[l]]) - exp[k]) <= 1e-8 * abs(exp[k]) + 0.5e-6, (i, l, r[col[l]], exp[k])
        top = np.abs(exp["Idiff"]).max()
        slack = 1e-10 * top + 0.5 * np.spacing(np.abs(exp["Idiff"]).astype(np.float32)).astype(np.float64)
        assert (np.abs(stack[i].astype(np.float64) - exp["Idiff"]) <= slack).all(), i
