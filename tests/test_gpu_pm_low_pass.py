"""The second stage of the S3 branch and bound (xh_pm.hip, k_pm_low_keep; option "low_pass"): the rows that survive the
sum-of-moduli bounds are transformed from their frequencies below K0 alone, and only those whose low-only maximum plus the tail
bound still reaches the particle's best lower bound minus two ambiguity margins are finished.  Nothing a caller sees may change:
every case compares low_pass 1 with low_pass 0 (same rows finished by the same arithmetic, so the re-scored particles and rows are
compared too) and with the search that transforms every row (prune 0: reference, angle and mirror).

Shapes: the smallest at which the two-level path exists, 64-px boxes, 24-32 references, 48 particles; the cut K0 is forced below nk
with the "k0" option and "high_cap" leaves room for seven rows in the store of k_pm_rows_high, so the rest are finished by the
transforming wave itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import synth  # noqa: E402

D, NREFS, N = 64, 32, 48
FIGURES = ("low_pass_rows_in", "low_pass_rows_out", "low_pass_rows_transformed")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return xa, xa.Context(0), torch


@pytest.fixture(scope="module")
def gallery():
    """phantom projections and particles made from them (read only)"""
    refs, _ = synth.make_refs(synth.phantom(D, seed=2, nblobs=14), NREFS)
    rng = np.random.default_rng(41)
    parts, _ = synth.make_particles(refs, N, rng, snr=0.1, max_shift=2)
    refs.setflags(write=False)
    parts.setflags(write=False)
    return refs, parts


def _dev(torch, a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()          # (a copy: the fixtures are read only)


def _run(pm, dp, low_pass, prune=1, **kw):
    pm.set_option("prune", prune)
    pm.set_option("low_pass", low_pass)
    out = [t.cpu().numpy() for t in pm.match(dp, **kw)]
    st = pm.last_stats()
    fig = {k: int(pm.get_option(k)) for k in FIGURES}
    return out, st, fig


def _three_ways(pm, dp, **kw):
    """low_pass 1, low_pass 0 and prune 0: the common assertions of every case; returns the first two runs' statistics and figures"""
    on, st1, fig1 = _run(pm, dp, 1, **kw)
    off, st0, fig0 = _run(pm, dp, 0, **kw)
    full, stf, _ = _run(pm, dp, 1, prune=0, **kw)
    pm.set_option("prune", 1)
    print("low pass on:", st1, fig1, "| off:", st0, fig0)
    for a, b, c in zip(on, off, full):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert st1["rows"] == st0["rows"] and st1["pruned_rows"] == st0["pruned_rows"]          # the first stage is counted as before
    assert st1["rescored_particles"] == st0["rescored_particles"] and st1["rescored_rows"] == st0["rescored_rows"]
    assert stf["pruned_rows"] == 0
    assert fig0 == {k: 0 for k in FIGURES}
    survivors = st1["rows"] - st1["pruned_rows"]
    assert 0 <= fig1["low_pass_rows_out"] <= fig1["low_pass_rows_in"] <= survivors
    assert fig1["low_pass_rows_transformed"] <= fig1["low_pass_rows_in"]
    return on, st1, fig1


def _matcher(gpu, refs, k0=8, high_cap=7):
    xa, ctx, torch = gpu
    pm = xa.ProjectionMatcher(ctx, _dev(torch, refs))
    pm.set_option("adaptive_finish", 0)        # the two-level form whatever survives
    pm.set_option("high_cap", high_cap)
    pm.set_option("k0", k0)
    K0, nk = pm.two_level_cut()
    return pm, K0, nk


def _band_limited_gallery(rng, nrefs, kmax=5):
    """References whose angular frequencies stop at kmax: sum over k of Re(c_k(r) exp(i k theta)) under a smooth radial window.
    c_k(r) is a smooth random radial profile, except for reference 0, whose phases are drawn anew at every radius: as much
    low-frequency modulus per ring as anybody, rings that never add up -- a large bound and a small maximum."""
    y, x = np.mgrid[0:D, 0:D] - D // 2
    r, th = np.hypot(x, y), np.arctan2(y, x)
    win = np.exp(-0.5 * ((r - 14.0) / 8.0) ** 2) * (r < D // 2 - 1)
    refs = np.zeros((nrefs, D, D))
    for j in range(nrefs):
        for k in range(kmax + 1):
            if j == 0:
                ph = rng.uniform(0, 2 * np.pi, D)[np.clip(np.rint(r).astype(int), 0, D - 1)]
                c = np.exp(1j * ph)
            else:
                c = sum(rng.standard_normal() * np.exp(-0.5 * ((r - rng.uniform(4, 26)) / rng.uniform(3, 8)) ** 2 + 1j * rng.uniform(0, 2 * np.pi))
                        for _ in range(3))
            refs[j] += (c * np.exp(1j * k * th)).real
        refs[j] *= win
        refs[j] -= refs[j].mean()
    return (refs / refs.std()).astype(np.float32)


def test_a_planned_row_is_dropped_by_the_second_stage(gpu):
    """(a) A gallery that is band limited below the cut, unrelated references: the planned rows of a particle are the four largest
    sums of moduli, of which one is its own reference; the others' low-only maxima are far below it and they are dropped although
    they were transformed first.  More rows leave than the low pass transformed: some of them were planned rows."""
    xa, ctx, torch = gpu
    rng = np.random.default_rng(7)
    refs = _band_limited_gallery(rng, 24)
    parts, _ = synth.make_particles(refs[1:], N, rng, snr=0.5, max_shift=1)
    pm, K0, nk = _matcher(gpu, refs, k0=8)
    assert K0 < nk
    on, st, fig = _three_ways(pm, _dev(torch, parts))
    dropped = fig["low_pass_rows_in"] - fig["low_pass_rows_out"]
    assert fig["low_pass_rows_in"] == st["rows"] - st["pruned_rows"] > 0
    assert dropped > fig["low_pass_rows_transformed"], fig       # otherwise no planned row was dropped and the case proves nothing
    assert fig["low_pass_rows_out"] >= N                          # every particle keeps its winner


def test_b_identical_references_both_survive(gpu):
    """(b) Two identical references have identical rows: neither can be dropped against the other, and which of the two is
    returned follows the visiting order and its tie rule, as in the exhaustive search.  (Unrelated references, so that the twelve
    particles made from the twin are won by the twin: both of its rows are then among the rows left to finish.)"""
    xa, ctx, torch = gpu
    rng = np.random.default_rng(19)
    refs = _band_limited_gallery(rng, 24)
    refs[9] = refs[4]
    own, _ = synth.make_particles(refs[4:5], 12, rng, snr=4.0, max_shift=0)
    others, _ = synth.make_particles(refs, N - 12, rng, snr=0.5, max_shift=1)
    parts = np.concatenate([own, others]).astype(np.float32)
    pm, K0, nk = _matcher(gpu, refs, k0=8)
    assert K0 < nk
    on, st, fig = _three_ways(pm, _dev(torch, parts))       # (equal to the exhaustive search: the tie went the same way)
    assert np.isin(on[0][:12], (4, 9)).all(), on[0][:12]
    assert fig["low_pass_rows_out"] >= N + 12                # the winner's row stays, and its twin has the same low-only result


def test_c_constant_particle_prunes_nothing(gpu, gallery):
    """(c) Particles of constant pixels.  Where the polar samples of such a particle come out exactly equal its sigma is 0, every
    normalised value is infinite or NaN and so are the thresholds of both stages: none of its rows may be dropped.  Where rounding
    leaves a sigma of 1e-8 the particle is an ordinary one made of rounding noise.  xh_pm_debug_prepare tells which is which.
    (Measured at this size: sigma 2.5e-8 to 1.9e-7 for the six constants below, none exactly 0 -- the bound for the sigma = 0 kind
    is asserted whenever one turns up.)"""
    xa, ctx, torch = gpu
    refs, parts = gallery
    pm, K0, nk = _matcher(gpu, refs, k0=8)
    const = np.stack([np.full((D, D), v, np.float32) for v in (1.0, 2.0, 0.5, 3.0, -1.0, 0.75)])
    sigma = pm.debug_prepare(_dev(torch, const), 32)[1]
    nzero = int((sigma == 0).sum())
    print("constant particles: sigma", sigma)
    on, st, fig = _three_ways(pm, _dev(torch, const))
    assert fig["low_pass_rows_out"] >= nzero * NREFS + (len(const) - nzero)
    if nzero == len(const):
        assert st["pruned_rows"] == 0 and fig["low_pass_rows_in"] == fig["low_pass_rows_out"] == len(const) * NREFS
    # ... and one among ordinary particles
    mixed = parts.copy()
    mixed[5] = 1.0
    sigma = pm.debug_prepare(_dev(torch, mixed), 32)[1]
    on, st, fig = _three_ways(pm, _dev(torch, mixed))
    assert fig["low_pass_rows_out"] >= (NREFS if sigma[5] == 0 else 1) + N - 1


def test_d_neighbour_lists_with_off_list_references(gpu, gallery):
    """(d) Ascending neighbour lists run over the whole bank with the off-list references masked (rowBound = -inf): those rows
    belong to neither stage."""
    xa, ctx, torch = gpu
    refs, parts = gallery
    rng = np.random.default_rng(12)
    lists = [np.sort(rng.choice(NREFS, size=int(rng.integers(1, 12)), replace=False)) for _ in range(N)]
    lists[3] = np.array([7])
    off = np.zeros(N + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    ids = np.concatenate(lists).astype(np.int32)
    pm, K0, nk = _matcher(gpu, refs, k0=8)
    on, st, fig = _three_ways(pm, _dev(torch, parts), nbr_off=off, nbr_ids=ids)
    assert st["rows"] == len(ids)
    assert N <= fig["low_pass_rows_in"] <= len(ids)
    for i in range(N):
        assert on[0][i] in lists[i]


def test_e_5d_search(gpu, gallery):
    """(e) Nine translations per particle: the rows of a particle span nine slots, each with its own norms and tails."""
    xa, ctx, torch = gpu
    refs, parts = gallery
    xo, yo = xa.search5d_offsets(3, 2)
    pm, K0, nk = _matcher(gpu, refs, k0=8, high_cap=11)
    on, st, fig = _three_ways(pm, _dev(torch, parts[:20]), shifts5d=(xo, yo))
    assert st["rows"] == 20 * NREFS * 9
    assert fig["low_pass_rows_in"] >= 20


def test_f_without_a_band_limit_the_path_does_not_engage(gpu, gallery):
    """(f) K0 = nk: the bank is contracted at every frequency, there is no low part to go by, and the figures read 0."""
    xa, ctx, torch = gpu
    refs, parts = gallery
    pm, K0, nk = _matcher(gpu, refs, k0=10 ** 6)
    assert K0 == nk
    dp = _dev(torch, parts)
    on, st1, fig1 = _run(pm, dp, 1)
    off, st0, fig0 = _run(pm, dp, 0)
    full, _, _ = _run(pm, dp, 1, prune=0)
    assert fig1 == fig0 == {k: 0 for k in FIGURES}
    for a, b, c in zip(on, off, full):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert st1 == st0 and st1["pruned_rows"] > 0


def test_low_pass_at_full_size(gpu):
    """256 px, 1000 references, 160 particles (the shape of test_full_size_matching_against_the_oracle) in the product
    configuration: low_pass 1 against low_pass 0, indices and re-scored rows."""
    xa, ctx, torch = gpu
    Df, nrefs, n = 256, 1000, 160
    vol = torch.from_numpy(synth.phantom(Df, seed=4, nblobs=20).astype(np.float32)).cuda()
    fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
    refs = fp.project(np.concatenate([synth.fibonacci_directions(nrefs), np.zeros((nrefs, 1))], 1))
    fp.close()
    refs = ((refs - refs.mean()) / refs.std()).contiguous()
    g = torch.Generator(device="cuda").manual_seed(23)
    idx = torch.randint(0, nrefs, (n,), generator=g, device="cuda")
    parts = (refs[idx] + np.sqrt(10.0) * torch.randn((n, Df, Df), generator=g, device="cuda")).contiguous()
    pm = xa.ProjectionMatcher(ctx, refs)
    K0, nk = pm.two_level_cut()
    assert K0 < nk
    on, st1, fig1 = _run(pm, parts, 1)
    off, st0, fig0 = _run(pm, parts, 0)
    print("full size: low pass on", st1, fig1, "off", st0, fig0, "K0", K0, "of", nk)
    for a, b in zip(on, off):
        assert np.array_equal(a, b)
    assert st1 == st0
    assert fig0 == {k: 0 for k in FIGURES}
    assert n <= fig1["low_pass_rows_out"] <= fig1["low_pass_rows_in"] == st1["rows"] - st1["pruned_rows"]
