"""GPU parity of the FourierProjector (central-slice gallery generation) against the
CPU oracle, through the C ABI. fp64 on the device like the reference; the images leave as float."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import fp_reference as ref  # noqa: E402
from tests import synth  # noqa: E402


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


@pytest.mark.parametrize("D,padding,maxf", [(32, 2.0, 0.5), (32, 1.0, 0.25), (25, 2.0, 0.3), (45, 1.0, 0.5), (49, 1.5, 0.4),
                                             (96, 2.0, 0.5)])
def test_coefficients_and_projections_match_the_oracle(gpu, oracle, D, padding, maxf):
    """45 at padding 1 (odd image, odd padded volume: k_fp_center_split's (k + P/2) % P, no Nyquist row in k_fp_c2r_rows), 49 at
    padding 1.5 (P = 73) and 96 at padding 2 (P = 192) next to the small boxes."""
    xa, ctx, torch = gpu
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    o = oracle.FP(vol, padding, maxf, 3)
    fp = xa.FourierProjector(ctx, torch.from_numpy(vol).cuda(), padding, maxf, 3)
    assert (fp.P, fp.cdim, fp.cstart) == (o.P, o.cdim, o.cstart)
    gre, gim = fp.coefs()
    ere, eim = o.coefs()
    scale = max(np.abs(ere).max(), np.abs(eim).max())
    # fp64 both sides; the 3-D FFT algorithms differ (radix-2 / Bluestein in LDS vs mixed radix)
    assert np.abs(gre - ere).max() <= 1e-11 * scale and np.abs(gim - eim).max() <= 1e-11 * scale
    ang = np.concatenate([[[0, 0, 0], [90, 90, 0], [10, 170, 33]], synth.random_angles(6, np.random.default_rng(D))])
    got = fp.project(ang).cpu().numpy()
    for a, g in zip(ang, got):
        exp = o.project(*a)
        assert np.abs(g - exp).max() <= 3e-7 * np.abs(exp).max()        # float32 output


def test_project_spanning_two_chunks(gpu):
    """xh_fp_project cuts a call into chunks of 512 MB of half spectra (1016 projections at D = 256): 1100 projections in one call
    (two chunks, the second short) are the same bits as the same angles in calls of 100. Every projection is computed alone, so
    no oracle is needed."""
    xa, ctx, torch = gpu
    D = 256
    g = torch.Generator(device="cuda").manual_seed(3)
    vol = torch.randn((D, D, D), generator=g, device="cuda")
    fp = xa.FourierProjector(ctx, vol, 1.0, 0.25, 3)
    ang = synth.random_angles(1100, np.random.default_rng(7))
    whole = fp.project(ang)
    parts = torch.cat([fp.project(ang[i:i + 100]) for i in range(0, len(ang), 100)])
    assert whole.shape == (1100, D, D) and bool(whole.abs().amax() > 0)
    assert torch.equal(whole, parts)


def test_ctf_multiplier_and_batching(gpu, oracle):
    xa, ctx, torch = gpu
    D = 32
    vol = synth.phantom(D, seed=4, nblobs=6).astype(np.float32)
    o = oracle.FP(vol, 2.0, 0.5, 3)
    fp = xa.FourierProjector(ctx, torch.from_numpy(vol).cuda(), 2.0, 0.5, 3)
    fy = np.fft.fftfreq(D)[:, None]
    fx = np.fft.rfftfreq(D)[None, :]
    ctf = np.cos(30.0 * (fx * fx + fy * fy)) * np.exp(-4.0 * (fx * fx + fy * fy))
    ang = synth.random_angles(40, np.random.default_rng(1))
    got = fp.project(ang, ctf=torch.from_numpy(ctf).cuda()).cpu().numpy()
    for i in (0, 17, 39):
        exp = o.project(*ang[i], ctf=ctf)
        assert np.abs(got[i] - exp).max() <= 3e-7 * np.abs(exp).max()


def test_gallery_feeds_projection_matching(gpu, oracle):
    """volume -> gallery (device) -> matcher (device): a projection at a gallery direction, rotated in
    plane by a multiple of the angular step, is assigned to that reference with that in-plane angle."""
    xa, ctx, torch = gpu
    D, nrefs = 64, 60
    vol = synth.phantom(D, seed=2, nblobs=14).astype(np.float32)
    dirs = synth.fibonacci_directions(nrefs)
    fp = xa.FourierProjector(ctx, torch.from_numpy(vol).cuda(), 2.0, 0.5, 3)
    gallery = fp.project(np.concatenate([dirs, np.zeros((nrefs, 1))], 1))
    pm = xa.ProjectionMatcher(ctx, gallery.contiguous())
    step = 360.0 / pm.N
    picks = [(7, 25), (31, 100), (55, 3)]
    parts = fp.project(np.array([[dirs[r, 0], dirs[r, 1], k * step] for r, k in picks]))
    refno, psi, flip = pm.match(parts.contiguous())
    assert refno.cpu().tolist() == [r for r, _ in picks]
    assert flip.cpu().tolist() == [0, 0, 0]
    got_psi = psi.cpu().numpy()
    for (r, k), g in zip(picks, got_psi):
        assert min((g - k) % pm.N, (k - g) % pm.N) <= 1 or min((g + k) % pm.N, (-g - k) % pm.N) <= 1


def test_errors_are_loud(gpu):
    xa, ctx, torch = gpu
    vol = torch.zeros((16, 16, 16), device="cuda")
    with pytest.raises(xa.XhError):
        xa.FourierProjector(ctx, vol, 2.0, 0.5, 1)       # linear interpolation is not on the device
    with pytest.raises(xa.XhError):
        xa.FourierProjector(ctx, vol, 0.5, 0.5, 3)
    # a padded size above 1024 is refused by name, by the check that stands before the first allocation (three cubes of 1026^3
    # would be 34 GB)
    with pytest.raises(xa.XhError, match="padded size 1026 exceeds 1024"):
        xa.FourierProjector(ctx, torch.empty((513, 513, 513), device="cuda"), 2.0, 0.5, 3)


# ---- against references that share no code with the projector or its oracle (tests/fp_reference.py) ------------------------------

def _device_axis_sums(torch, vol):
    """The three axis sums of a device volume in float64: only D x D arrays cross the link."""
    return {k: vol.sum(d, dtype=torch.float64).cpu().numpy() for k, d in (("z", 0), ("y", 1), ("x", 2))}


def _check_exact_views(xa, ctx, torch, vol, padding, maxf, ctf=None):
    """All eight axis-aligned views in one call against reference A, within the float32 output's 3e-7 of the image maximum."""
    sums = _device_axis_sums(torch, vol)
    fp = xa.FourierProjector(ctx, vol, padding, maxf, 3)
    try:
        got = fp.project(np.array(ref.EXACT_VIEWS, float), ctf=None if ctf is None else torch.from_numpy(ctf).cuda()).cpu().numpy()
        P = fp.P
    finally:
        fp.close()
    devs = []
    for view, g in zip(ref.EXACT_VIEWS, got):
        exp = ref.exact_view(sums, *view, maxf, ctf)
        devs.append(np.abs(g - exp).max() / np.abs(exp).max())
    print(f"exact views D={vol.shape[0]} P={P} max_freq={maxf} ctf={ctf is not None}: worst {max(devs):.2e} (bound 3e-7)")
    for view, d in zip(ref.EXACT_VIEWS, devs):
        assert d <= 3e-7, (view, d)


def _ctf_image(D):
    """A multiplier of both signs on the half spectrum."""
    fy = np.fft.fftfreq(D)[:, None]
    fx = np.fft.rfftfreq(D)[None, :]
    return np.cos(30.0 * (fx * fx + fy * fy)) * np.exp(-4.0 * (fx * fx + fy * fy))


@pytest.mark.parametrize("D,padding,maxf", [(64, 2, 0.49), (45, 3, 0.49), (50, 1, 0.45), (200, 2, 0.49), (256, 2, 0.49), (384, 2, 0.49),
                                             (512, 2, 0.49)])
def test_exact_views_on_noise(gpu, D, padding, maxf):
    """float32 white noise made on the device; at an axis-aligned view, integer padding and max_freq < 0.5 the projection is the
    band-limited axis sum exactly, so every stage of create is checked at full size without an oracle that could run there. What
    each shape reaches, and what it holds on the device while create runs (32 P^3 bytes of transform and Re / Im volumes, 16 cdim^3
    of coefficients, 4 D^3 of volume):
      (64, 2)   P = 128, radix-2 lines;                                                                     0.1 GB
      (45, 3)   odd D, odd P = 135: no Nyquist row, (k + P/2) % P with an odd P, Bluestein on 512;          0.1 GB
      (50, 1)   P = D < 64: the prefilter's exact-sum branch, the crop is the whole cube;                   6 MB
      (200, 2)  P = 400: Bluestein on 1024 for the volume and on 512 for the image;                         3 GB
      (256, 2)  P = 512: the production size;                                                               6.5 GB
      (384, 2)  P = 768: Bluestein on 2048, two lines per workgroup;                                        22 GB
      (512, 2)  P = 1024: the cap; the z pass of the prefilter strides by 2^20 doubles, 1023 of them;       52 GB"""
    xa, ctx, torch = gpu
    g = torch.Generator(device="cuda").manual_seed(D)
    vol = torch.randn((D, D, D), generator=g, device="cuda")
    _check_exact_views(xa, ctx, torch, vol, padding, maxf)


@pytest.mark.parametrize("maxf,with_ctf", [(0.5, False), (0.49, True)])
def test_exact_views_at_production_parameters(gpu, maxf, with_ctf):
    """D = 256, padding 2 on the benchmark's phantom (6.5 GB on the device while create runs). At max_freq = 0.5 the two Nyquist
    nodes of the disc are interpolated across the crop boundary's mirror; a smooth volume moves by 1e-8 of the image maximum there
    (tests/test_fp_reference.py), well inside the float32 bound. Smooth means that the box does not cut the volume: the benchmark's
    default spread (rmax = 20) leaves 5e-4 of the maximum on the box faces, and there the oracle itself is 4e-7 (D = 128) to 9e-7
    (D = 64) from reference A at max_freq = 0.5 and 4e-14 at 0.49; the device measured 4.5e-6 at D = 256. That is the reference
    method's mirror, not an error of the device, so this test uses the phantom's compact spread (rmax = 9.6, what the tests'
    synth.phantom has), where the oracle is 3e-10 from reference A at both sizes. The CTF image has multipliers of both signs."""
    import bench
    xa, ctx, torch = gpu
    D = 256
    vol = bench.phantom_volume(torch, D, torch.Generator(device="cuda").manual_seed(11), "cuda", rmax=9.6)
    _check_exact_views(xa, ctx, torch, vol, 2.0, maxf, _ctf_image(D) if with_ctf else None)


@pytest.mark.parametrize("D,padding,maxf", [(32, 2, 0.45), (45, 2, 0.4), (32, 3, 0.45), (32, 1, 0.45)])
def test_general_angles_against_the_direct_sum(gpu, oracle, D, padding, maxf):
    """Reference B is the continuous transform that padding and interpolating approximate; the oracle's distance from it is the
    method's own error (tests/test_fp_reference.py bounds it). The device may be no further from it than the oracle is, plus the
    float32 output's 3e-7 of the image maximum. (-30, -75, 400) leaves the angles' principal ranges."""
    xa, ctx, torch = gpu
    vol = synth.phantom(D, seed=5, nblobs=9).astype(np.float32)
    ang = np.array([(10, 170, 33), (123, 57, -40), (271.5, 91, 12), (-30, -75, 400), (0, 0, 0)], float)
    o = oracle.FP(vol, padding, maxf, 3)
    fp = xa.FourierProjector(ctx, torch.from_numpy(vol).cuda(), padding, maxf, 3)
    try:
        got = fp.project(ang).cpu().numpy()
    finally:
        fp.close()
    for a, g in zip(ang, got):
        exp = ref.direct_sum(vol, *a, maxf)
        m = np.abs(exp).max()
        dev_o, dev_g = np.abs(o.project(*a) - exp).max() / m, np.abs(g - exp).max() / m
        print(f"direct sum D={D} pad={padding} max_freq={maxf} angles={tuple(a)}: device {dev_g:.3e} oracle {dev_o:.3e}")
        assert dev_g <= dev_o + 3e-7, (a, dev_g, dev_o)


@pytest.mark.parametrize("D,padding,maxf", [(128, 2.0, 0.5), (256, 1.0, 0.5), (200, 1.5, 0.4)])
def test_oracle_parity_at_real_sizes(gpu, oracle, D, padding, maxf):
    """The bounds and angles of test_coefficients_and_projections_match_the_oracle at sizes the oracle still creates in seconds:
    (128, 2) P = 256; (256, 1) P = D = 256, where the slice reaches the crop boundary's mirror at the production box; (200, 1.5)
    P = 300, Bluestein on 1024 with a fractional padding. (256, 2) takes the oracle 21 s: reference A stands in for it above."""
    xa, ctx, torch = gpu
    vol = synth.phantom(D, seed=11, nblobs=9).astype(np.float32)
    o = oracle.FP(vol, padding, maxf, 3)
    fp = xa.FourierProjector(ctx, torch.from_numpy(vol).cuda(), padding, maxf, 3)
    try:
        assert (fp.P, fp.cdim, fp.cstart) == (o.P, o.cdim, o.cstart)
        gre, gim = fp.coefs()
        ere, eim = o.coefs()
        scale = max(np.abs(ere).max(), np.abs(eim).max())
        dre, dim = np.abs(gre - ere).max() / scale, np.abs(gim - eim).max() / scale
        print(f"oracle parity D={D} P={fp.P}: coefficients re {dre:.2e} im {dim:.2e} (bound 1e-11)")
        assert dre <= 1e-11 and dim <= 1e-11
        ang = np.concatenate([[[0, 0, 0], [90, 90, 0], [10, 170, 33]], synth.random_angles(6, np.random.default_rng(D))])
        got = fp.project(ang).cpu().numpy()
    finally:
        fp.close()
    devs = []
    for a, g in zip(ang, got):
        exp = o.project(*a)
        devs.append(np.abs(g - exp).max() / np.abs(exp).max())
    print(f"oracle parity D={D} P={o.P}: projections worst {max(devs):.2e} (bound 3e-7)")
    assert max(devs) <= 3e-7, devs


def test_angle_identities(gpu):
    """(rot, tilt, psi), (rot + 360, tilt, psi - 360) and (rot + 180, -tilt, psi + 180) are one Euler matrix up to the rounding of
    the sines, so one image within the float32 bound; no projections is an empty stack."""
    xa, ctx, torch = gpu
    D = 64
    g = torch.Generator(device="cuda").manual_seed(5)
    vol = torch.randn((D, D, D), generator=g, device="cuda")
    fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
    ang = np.concatenate([[[10, 170, 33], [0, 0, 0], [271.5, 91, 12]], synth.random_angles(5, np.random.default_rng(2))])
    base = fp.project(ang)
    full_turn = fp.project(ang + [360, 0, -360])
    other_side = fp.project(ang * [1, -1, 1] + [180, 0, 180])
    m = base.abs().amax(dim=(1, 2))
    assert bool((m > 0).all())
    d1 = ((full_turn - base).abs().amax(dim=(1, 2)) / m).max().item()
    d2 = ((other_side - base).abs().amax(dim=(1, 2)) / m).max().item()
    print(f"angle identities: +360/-360 {d1:.2e}, +180/-tilt/+180 {d2:.2e} (bound 3e-7)")
    assert d1 <= 3e-7 and d2 <= 3e-7
    none = fp.project(np.zeros((0, 3)))
    assert none.shape == (0, D, D) and none.dtype == torch.float32
    assert torch.equal(fp.project(ang), base)           # and the handle is as usable as before
    fp.close()


def test_ctf_image_across_the_chunk_seam(gpu):
    """test_project_spanning_two_chunks with a CTF image: the one image multiplies every projection of both chunks, so 1100 in
    one call are the same bits as the same angles in calls of 100."""
    xa, ctx, torch = gpu
    D = 256
    g = torch.Generator(device="cuda").manual_seed(3)
    vol = torch.randn((D, D, D), generator=g, device="cuda")
    fp = xa.FourierProjector(ctx, vol, 1.0, 0.25, 3)
    ctf = torch.from_numpy(_ctf_image(D)).cuda()
    ang = synth.random_angles(1100, np.random.default_rng(7))
    whole = fp.project(ang, ctf=ctf)
    parts = torch.cat([fp.project(ang[i:i + 100], ctf=ctf) for i in range(0, len(ang), 100)])
    assert whole.shape == (1100, D, D) and bool(whole.abs().amax() > 0)
    assert torch.equal(whole, parts)
    assert not torch.equal(whole[:8], fp.project(ang[:8]))          # the multiplier was applied
    fp.close()
