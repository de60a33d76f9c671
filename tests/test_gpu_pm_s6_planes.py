"""S6 (xh_pm_translate) with the particle kept out of z: the coarse pass builds the rotated reference alone and its row and
bestShift kernels read the particle where it lies, mirrored by the read.

Shapes are the smallest at which these kernels can go wrong: 64 px (the column pass's block with columns 0 and D/2 plus
ordinary ones), 128 px (the 32 x 32 build-tile seam in both directions), 32 px (the generic path beside them), one particle of
256 px for the bands that the coarse bestShift stages in LDS; batches of 1, 2 and 5 (an odd batch pairs its last particle with
itself); flips mixed in a batch; a refno = -1 entry; a batch whose pointer is aligned to its floats only.
Reference values come from the CPU oracle at the tolerances of tests/test_gpu_pm.py: shifts 1e-3 px, maxCC 1e-5.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import synth  # noqa: E402

MAX_SHIFT = 6.0
MODES = {
    "default": None,       # fp32 pass, the ambiguous particles repeated in double precision
    "all_repeated": 1e30,  # s6_eps: every decision is "within the margin", so every particle goes through the repeat
    "none_repeated": 0.0,  # nothing is within a margin of zero: the fp32 pass alone
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


_cases = {}


def _case(oracle, D):
    """Five particles of D px, nonzero in column 0 and column D - 1, flips mixed, entry 3 without a reference; the oracle's
    translation of them, computed once per size (a particle's result does not depend on the rest of its batch)."""
    if D in _cases:
        return _cases[D]
    nrefs, n = (6, 12) if D <= 128 else (2, 5)         # 256 px serves the one-particle test below: no more than it needs
    refs, _ = synth.make_refs(synth.phantom(D, seed=2, nblobs=14), nrefs)
    rng = np.random.default_rng(100 + D)
    parts, truth = synth.make_particles(refs, n, rng, snr=0.5, max_shift=3)
    sd = parts.std()
    parts[:, :, 0] += 3 * sd
    parts[:, :, D - 1] -= 2 * sd
    o = oracle.PM(refs)
    if D <= 128:
        er, ep, ef, _ = o.match(parts)
        er, ep, ef = er[:, 0], ep[:, 0], ef[:, 0]
    else:                                              # 256 px: the true reference and mirror, any in-plane angle (no CPU search)
        er = np.array([t[0] for t in truth], np.int32)
        ef = np.array([i % 2 == 0 for i in range(n)], np.uint8)
        ep = rng.integers(0, o.N, n).astype(np.int32)
    fl, un = [i for i in range(n) if ef[i]], [i for i in range(n) if not ef[i]]
    assert len(fl) >= 3 and len(un) >= 2, "the seed no longer gives mixed flips"
    pick = [fl[0], un[0], fl[1], un[1], fl[2]]         # m = 1: a mirrored particle alone; m = 2: a mirrored and a plain one
    parts = np.ascontiguousarray(parts[pick])
    er, ep, ef = er[pick].astype(np.int32), ep[pick].astype(np.int32), ef[pick].astype(np.uint8)
    er[3] = -1
    expect = o.translate(parts, er, ep, ef, MAX_SHIFT) if D <= 128 else None
    _cases[D] = refs, parts, er, ep, ef, expect
    return _cases[D]


def _translate(gpu, pm, parts, er, ep, ef, m):
    xa, ctx, torch = gpu
    out = pm.translate(torch.from_numpy(parts[:m]).cuda(), torch.from_numpy(er[:m]).cuda(), torch.from_numpy(ep[:m]).cuda(),
                       torch.from_numpy(ef[:m]).cuda(), MAX_SHIFT)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("D,m", [(32, 1), (32, 2), (32, 5), (64, 1), (64, 2), (64, 5), (128, 5)])
def test_translation_against_the_oracle_and_twice_the_same_bits(gpu, oracle, D, m, mode):
    xa, ctx, torch = gpu
    refs, parts, er, ep, ef, expect = _case(oracle, D)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    if MODES[mode] is not None:
        pm.set_option("s6_eps", MODES[mode])
    sx, sy, cc = _translate(gpu, pm, parts, er, ep, ef, m)
    rep = pm.translate_repeated()
    ex, ey, ec = (np.asarray(v)[:m] for v in expect)
    print("D", D, "m", m, mode, "repeated", rep, "max |dsx|", np.abs(sx - ex).max(), "|dsy|", np.abs(sy - ey).max(),
          "|dcc|", np.abs(cc - ec).max())
    if D != 32:                                        # 32 px takes the generic double-precision path: no repeats to count
        if mode == "all_repeated":
            assert rep == int((er[:m] >= 0).sum())
        if mode == "none_repeated":
            assert rep == 0
    assert np.abs(sx - ex).max() <= 1e-3
    assert np.abs(sy - ey).max() <= 1e-3
    assert np.abs(cc - ec).max() <= 1e-5
    if m == 5:
        assert sx[3] == 0 and sy[3] == 0 and cc[3] == 0          # refno = -1
    # the same call once more in the same process: an order of additions that depended on scheduling would show here
    again = _translate(gpu, pm, parts, er, ep, ef, m)
    for a, b in zip((sx, sy, cc), again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("mode", ["none_repeated", "all_repeated"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_column_zero_of_a_mirrored_particle_is_not_read_and_a_plain_one_is_read_as_it_lies(gpu, oracle, D, mode):
    """The mirror of an even box sends column 0 outside the image: Mimg's column 0 is zero and the particle's column 0 is never
    used. Particle B is particle A with column 0 negated -- the same sum of squares, so the same balance exponent -- and each
    is translated alone (a batch of one pairs with itself). Mirrored, A and B must give the same bits; plain, they must not,
    and either agrees with the oracle, which reads column D - 1 and column 0 where they lie. At 256 px the coarse pass takes
    the particle's bands through LDS (17 staged rows, read backwards for a mirrored particle)."""
    xa, ctx, torch = gpu
    refs, parts, er, ep, ef, _ = _case(oracle, D)
    a = parts[0:1].copy()
    b = a.copy()
    b[:, :, 0] = -b[:, :, 0]
    assert np.abs(a[:, :, 0]).min() > 0 and np.abs(a[:, :, D - 1]).min() > 0
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    pm.set_option("s6_eps", MODES[mode])
    o = oracle.PM(refs)
    res = {}
    for name, img in (("a", a), ("b", b)):
        for flip in (1, 0):
            f = np.array([flip], np.uint8)
            got = _translate(gpu, pm, img, er, ep, f, 1)
            ex, ey, ec = o.translate(img, er[:1], ep[:1], f, MAX_SHIFT)
            assert abs(got[0][0] - ex[0]) <= 1e-3 and abs(got[1][0] - ey[0]) <= 1e-3 and abs(got[2][0] - ec[0]) <= 1e-5
            res[name, flip] = got
    for u, v in zip(res["a", 1], res["b", 1]):
        assert u.tobytes() == v.tobytes()
    assert res["a", 0][2][0] != res["b", 0][2][0]


def test_particles_at_a_pointer_that_is_only_float_aligned(gpu, oracle):
    """The row kernel takes a plain particle in 8-byte loads where the pointer allows it and float by float where it does not:
    the same batch (a mirrored and a plain particle) from a buffer that starts one float into an allocation gives the same bits."""
    xa, ctx, torch = gpu
    D, m = 64, 2
    refs, parts, er, ep, ef, _ = _case(oracle, D)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    pm.set_option("s6_eps", 0.0)
    aligned = _translate(gpu, pm, parts, er, ep, ef, m)
    buf = torch.empty(m * D * D + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(m, D, D)
    view.copy_(torch.from_numpy(parts[:m]))
    assert view.is_contiguous() and view.data_ptr() % 8 == 4
    out = pm.translate(view, torch.from_numpy(er[:m]).cuda(), torch.from_numpy(ep[:m]).cuda(), torch.from_numpy(ef[:m]).cuda(), MAX_SHIFT)
    for a, b in zip(aligned, out):
        assert a.tobytes() == b.cpu().numpy().tobytes()
