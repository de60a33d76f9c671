"""The matrix-core ring DFT multiplies out the frequencies 0..h/2 of a ring (h = n/2) and forms the other half of the spectrum,
X[h-k], from the same four partial sums in its epilogue. Every coefficient of every ring of debug_prepare is held against the
CPU oracle's prepare_particle, with the bounds of test_gpu_pm.py::test_particle_polar_fourier_transform (1e-12 in fp64, 5e-6
in fp32, of the particle's largest coefficient), and ring by ring the two halves are stated separately: a wrong sign or pairing
in the epilogue shows in k > h/2 alone.

Shapes: 64 px, 37 particles -- rings r = 1..31 have odd and even h, self-paired frequencies (n = 12, 24, ...), the shortest
ring (n = 6) and a slot tail (37 is no multiple of the 32 / 16 slots of a block); 256 px, 3 particles -- rings with more than
256 (fp32) / 128 (fp64) folded samples cross the chunk seam of the staging loop and need several frequency tiles per wave.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import synth  # noqa: E402


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


def _case(D, nrefs, nparts):
    vol = synth.phantom(D, seed=1, nblobs=14)
    refs, _ = synth.make_refs(vol, nrefs)
    parts, _ = synth.make_particles(refs, nparts, np.random.default_rng(3), snr=0.1, max_shift=2)
    return refs, parts


@pytest.fixture(scope="module", params=[(64, 48, 37), (256, 2, 3)], ids=["64px-37", "256px-3"])
def case(request, oracle):
    """particles and the oracle's spectra of them, computed once for both precisions"""
    D, nrefs, nparts = request.param
    refs, parts = _case(D, nrefs, nparts)
    o = oracle.PM(refs)
    exp = [o.prepare_particle(p) for p in parts]
    return D, refs, parts, o, exp


def _rings(o):
    """(n, first coefficient) of every ring: n = 2 floor(pi r) samples, n / 2 + 1 coefficients"""
    out, c = [], 0
    for r in range(o.Ri, o.Ro + 1):
        n = 2 * int(np.pi * r)
        out.append((n, c))
        c += n // 2 + 1
    assert c == o.ncoef and out[-1][0] == o.N
    return out


@pytest.mark.parametrize("precision,tol", [(64, 1e-12), (32, 5e-6)])
def test_every_coefficient_of_every_ring(gpu, case, precision, tol):
    xa, ctx, torch = gpu
    D, refs, parts, o, exp = case
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    assert (pm.N, pm.ncoef) == (o.N, o.ncoef)
    c, s = pm.debug_prepare(torch.from_numpy(parts).cuda(), precision)
    rings = _rings(o)
    if D == 64:
        ns = [n for n, _ in rings]
        assert min(ns) == 6 and any(n % 4 == 0 for n in ns) and any(n % 4 == 2 for n in ns)
    else:
        assert o.N // 2 + 1 > 256 and o.N // 4 + 1 > 4 * 32
    worst_lo = worst_hi = 0.0
    bad = []
    for i, (fP, fPm, sig) in enumerate(exp):
        assert abs(s[i] - sig) <= tol * sig
        big = np.abs(fP).max()
        err = np.abs(c[i] - fP) / big
        for ri, (n, c0) in enumerate(rings):
            h = n // 2
            lo = err[c0:c0 + h // 2 + 1].max()                   # multiplied out
            hi = err[c0 + h // 2 + 1:c0 + h + 1].max()           # formed in the epilogue (n >= 2: never empty)
            worst_lo, worst_hi = max(worst_lo, lo), max(worst_hi, hi)
            if lo > tol or hi > tol:
                bad.append((i, ri + o.Ri, n, lo, hi))
    print(f"D {D} fp{precision}: largest error / largest coefficient: k <= h/2 {worst_lo:.3g}, k > h/2 {worst_hi:.3g}")
    assert not bad, "particle, ring radius, n, error for k <= h/2, error for k > h/2: " + "; ".join(
        f"{i} {r} {n} {lo:.3g} {hi:.3g}" for i, r, n, lo, hi in bad[:12]) + f" ({len(bad)} rings beyond {tol})"
    assert max(worst_lo, worst_hi) <= tol
