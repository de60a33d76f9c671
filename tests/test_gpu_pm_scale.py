"""The translational search (S6 of xh_pm_translate) at any particle / reference scale.

Nothing in the library or in the programs normalises particles or references: a gallery projected from a volume has the
volume's scale, often 1e2-1e3 away from normalised particles. S6 packs two real signals into one complex transform twice
(z = Mref + i Mimg; P_a + i P_b for two particles that share one inverse transform), and the rounding of either half follows
the size of the other. These tests hold the results to the oracle at particle scales 1e-3 .. 1e3 relative to the gallery,
with galleries scaled instead, with batches whose paired particles differ by 1e3, with blank particles, and check that the
fp32 map stays within its margin and that the results are the same from run to run. Bounds as in tests/test_gpu_pm.py:
shifts 1e-3 px, maxCC 1e-5, discrete results identical to the oracle; against the library itself 1e-4 px and 1e-6.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import synth  # noqa: E402

# (particle scale, gallery scale)
SCALES = [(1e-3, 1.0), (1e-2, 1.0), (1.0, 1.0), (1e2, 1.0), (1e3, 1.0), (1.0, 1e-3), (1.0, 1e3)]
SIZES = [64, 128, 256, 50]          # 64 / 128 / 256: the paired register-blocked chain; 50: the generic path


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_DATA = {}


def _data(D):
    """References normalised to std 1, particles = references + noise at SNR 0.1 (the suite's kind of data)."""
    if D not in _DATA:
        nrefs, n = (6, 16) if D == 256 else (8, 24)
        vol = synth.phantom(D, seed=11, nblobs=14)
        refs, _ = synth.make_refs(vol, nrefs)
        refs = ((refs - refs.mean()) / refs.std()).astype(np.float32)
        parts, _ = synth.make_particles(refs, n, np.random.default_rng(D + 5), snr=0.1, max_shift=3)
        _DATA[D] = (refs, parts)
    return _DATA[D]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _assert_oracle(got, exp, what):
    sx, sy, cc = got
    ex, ey, ec = exp
    assert np.abs(sx - ex).max() <= 1e-3 and np.abs(sy - ey).max() <= 1e-3, (what, np.abs(sx - ex).max(), np.abs(sy - ey).max())
    assert np.abs(cc - ec).max() <= 1e-5, (what, np.abs(cc - ec).max())


@pytest.mark.parametrize("ps,gs", SCALES)
@pytest.mark.parametrize("D", SIZES)
def test_translate_and_match_at_any_scale_against_the_oracle(gpu, oracle, D, ps, gs):
    """match (refno, psi, flip identical -- the rotational rows are normalised, a guard) and translate (1e-3 px, 1e-5) against the
    oracle on the same scaled inputs, with the product defaults."""
    xa, ctx, torch = gpu
    refs, parts = _data(D)
    refs = (refs * np.float32(gs)).astype(np.float32)
    parts = (parts * np.float32(ps)).astype(np.float32)
    pm = xa.ProjectionMatcher(ctx, _dev(torch, refs))
    o = oracle.PM(refs)
    dp = _dev(torch, parts)
    refno, psi, flip = pm.match(dp)
    er, ep, ef, _ = o.match(parts)
    assert np.array_equal(_host(refno), er[:, 0]) and np.array_equal(_host(psi), ep[:, 0]) and np.array_equal(_host(flip), ef[:, 0])
    got = [_host(t) for t in pm.translate(dp, refno, psi, flip)]
    _assert_oracle(got, o.translate(parts, er[:, 0], ep[:, 0], ef[:, 0]), (D, ps, gs))
    pm.close()


def _mixed(parts, order):
    """particles in the given order, every second one (by position) scaled by 1e3: every pair of the paired inverse is unbalanced"""
    out = parts[order].copy()
    big = np.arange(len(order)) % 2 == 1
    out[big] *= np.float32(1e3)
    return out, big


@pytest.mark.parametrize("D", SIZES)
def test_mixed_scale_batches(gpu, oracle, D):
    """Particles of scale 1 and 1e3 alternate (and, in a second order, get other partners): each one's result equals the oracle's and
    that of the same particle translated in a batch of its own scale (1e-4 px, 1e-6, the same assignment)."""
    xa, ctx, torch = gpu
    refs, parts = _data(D)
    n = len(parts)
    pm = xa.ProjectionMatcher(ctx, _dev(torch, refs))
    o = oracle.PM(refs)
    for order in (np.arange(n), np.roll(np.arange(n)[::-1], 3)):
        mixed, big = _mixed(parts, order)
        dp = _dev(torch, mixed)
        refno, psi, flip = pm.match(dp)
        r, p, f = _host(refno), _host(psi), _host(flip)
        er, ep, ef, _ = o.match(mixed)
        assert np.array_equal(r, er[:, 0]) and np.array_equal(p, ep[:, 0]) and np.array_equal(f, ef[:, 0])
        got = [_host(t) for t in pm.translate(dp, refno, psi, flip)]
        _assert_oracle(got, o.translate(mixed, r, p, f), (D, "mixed"))
        for sel in (big, ~big):
            idx = np.nonzero(sel)[0]
            alone = [_host(t) for t in pm.translate(_dev(torch, mixed[idx]), _dev(torch, r[idx]), _dev(torch, p[idx]), _dev(torch, f[idx]))]
            assert np.abs(got[0][idx] - alone[0]).max() <= 1e-4 and np.abs(got[1][idx] - alone[1]).max() <= 1e-4, D
            assert np.abs(got[2][idx] - alone[2]).max() <= 1e-6, D
    pm.close()


def _map_error(pm, dp, refno, psi, flip, n):
    pm.set_option("s6_capture", 64)
    pm.translate(dp, refno, psi, flip)
    r64 = pm.debug_s6_maps(n)
    pm.set_option("s6_capture", 32)
    pm.translate(dp, refno, psi, flip)
    r32 = pm.debug_s6_maps(n)
    pm.set_option("s6_capture", 0)
    peak = np.abs(r64).reshape(n, -1).max(1)
    assert peak.min() > 0
    return np.abs(r32 - r64).reshape(n, -1).max(1) / peak


@pytest.mark.parametrize("D", [64, 128, 256])
def test_fp32_map_error_against_the_margin_at_any_scale(gpu, D):
    """The fp32 pass is exact only while its map is much closer to the double one than the margin s6_eps it flags by:
    max |R32 - R64| <= s6_eps / 4 of each map's own peak, on the scale grid and on mixed batches."""
    xa, ctx, torch = gpu
    refs, parts = _data(D)
    n = len(parts)
    worst = {}
    for ps, gs in SCALES + [("mixed", 1.0)]:
        pm = xa.ProjectionMatcher(ctx, _dev(torch, (refs * np.float32(gs)).astype(np.float32)))
        eps = pm.get_option("s6_eps")
        p = _mixed(parts, np.arange(n))[0] if ps == "mixed" else (parts * np.float32(ps)).astype(np.float32)
        dp = _dev(torch, p)
        refno, psi, flip = pm.match(dp)
        worst[(ps, gs)] = float(_map_error(pm, dp, refno, psi, flip, n).max())
        pm.close()
    print("D", D, "max |R32 - R64| / peak:", worst, "s6_eps", eps)
    bad = {k: v for k, v in worst.items() if not v <= eps / 4}
    assert not bad, bad


def _close(a, b, tol):
    """|a - b| <= tol, NaN only against NaN"""
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)))


@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("fp32", [1, 0])
def test_blank_particles_and_references(gpu, oracle, D, fp32):
    """Constant and all-zero particles among normal ones, and an all-zero reference: their correlation map is constant and the
    oracle's bestShift returns (0, 0) for it; the device must too, whatever its packed partner leaves in the map. Where the
    oracle's own transform leaves rounding in the map of a constant particle (D = 50 here), its arg-max is that rounding's and
    no other arithmetic can reproduce it: there the device's (0, 0) -- the outcome of the exact map -- is checked instead. (A
    mirrored constant particle is not blank -- its first column is zero -- and its map has exact ties along one axis; it is
    left out.)"""
    xa, ctx, torch = gpu
    refs, parts = _data(D)
    refs = refs.copy()
    refs[-1] = 0.0
    parts = parts.copy()
    n, nrefs = len(parts), len(refs)
    rng = np.random.default_rng(D)
    o = oracle.PM(refs)
    r = rng.integers(0, nrefs - 1, n).astype(np.int32)
    p = rng.integers(0, o.N, n).astype(np.int32)
    f = rng.integers(0, 2, n).astype(np.uint8)
    blanks = {1: (1.0, 0), 4: (0.0, 0), 7: (0.0, 1), 10: (-2.5e3, 0), 13: (1e-3, 0)}
    for i, (v, fl) in blanks.items():
        parts[i] = v
        f[i] = fl
    r[5] = r[8] = nrefs - 1                                    # the all-zero reference, with a normal particle
    # blanks whose map the oracle itself computes as exactly constant
    exact = [i for i in blanks if np.ptp(oracle.correlation_matrix(oracle.rotate2d(refs[r[i]].astype(np.float64), p[i] * 360.0 / o.N),
                                                                   parts[i].astype(np.float64))) == 0]
    assert 4 in exact and 7 in exact and (D == 50 or len(exact) == len(blanks)), exact
    pm = xa.ProjectionMatcher(ctx, _dev(torch, refs))
    pm.set_option("s6_fp32", fp32)
    for max_shift in (-1.0, 4.0):
        sx, sy, cc = [_host(t) for t in pm.translate(_dev(torch, parts), _dev(torch, r), _dev(torch, p), _dev(torch, f), max_shift)]
        ex, ey, ec = o.translate(parts, r, p, f, max_shift)
        for i in blanks:
            assert sx[i] == 0 and sy[i] == 0, (D, fp32, i, sx[i], sy[i])
            if i not in exact:
                ex[i] = ey[i] = 0.0
        assert _close(sx, ex, 1e-3) and _close(sy, ey, 1e-3), (D, fp32, max_shift, np.c_[sx, ex, sy, ey][list(blanks) + [5, 8]])
        assert _close(cc, ec, 1e-5), (D, fp32, max_shift, np.abs(cc - ec).max())
    pm.close()


def test_results_are_the_same_from_run_to_run(gpu):
    """At 256 px on the bench's kind of data (1000 phantom projections, 1024 particles at SNR 0.1) with s6_eps raised so that hundreds
    of particles take the double-precision repeat: translate three times on one handle and once on a fresh one, and match, give
    bitwise identical outputs; so does a batch of mixed scales."""
    xa, ctx, torch = gpu
    D, nrefs, n = 256, 1000, 1024
    g = torch.Generator(device="cuda").manual_seed(7)
    vol = torch.from_numpy(synth.phantom(D, seed=4, nblobs=20).astype(np.float32)).cuda()
    fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
    refs = fp.project(np.concatenate([synth.fibonacci_directions(nrefs), np.zeros((nrefs, 1))], 1))
    fp.close()
    refs = ((refs - refs.mean()) / refs.std()).contiguous()
    idx = torch.randint(0, nrefs, (n,), generator=g, device="cuda")
    parts = (torch.roll(refs[idx], shifts=(2, -3), dims=(1, 2)) + np.sqrt(10.0) * torch.randn((n, D, D), generator=g, device="cuda")).contiguous()
    mixed = parts.clone()
    mixed[1::2] *= 1e3

    def runs(pm, dp):
        refno, psi, flip = pm.match(dp)
        again = pm.match(dp)
        assert all(torch.equal(a, b) for a, b in zip((refno, psi, flip), again))
        out = [pm.translate(dp, refno, psi, flip) for _ in range(3)]
        return (refno, psi, flip), out

    pm = xa.ProjectionMatcher(ctx, refs)
    pm.set_option("s6_eps", 1e-3)
    for dp in (parts, mixed):
        asg, out = runs(pm, dp)
        rep = pm.translate_repeated()
        print("repeated in double", rep, "of", n)
        assert rep >= 100
        pm2 = xa.ProjectionMatcher(ctx, refs)
        pm2.set_option("s6_eps", 1e-3)
        asg2, out2 = runs(pm2, dp)
        pm2.close()
        assert all(torch.equal(a, b) for a, b in zip(asg, asg2))
        for o in out[1:] + out2[:1]:
            assert all(torch.equal(a, b) for a, b in zip(out[0], o))
    pm.close()
