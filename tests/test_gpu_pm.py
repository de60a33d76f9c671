"""GPU parity tests of the projection-matching path (C ABI -> HIP) against the CPU oracle.

The bar (BASELINE.json north_star): best-orientation indices (reference id, in-plane angle
index, mirror flag) bit-identical to the CPU path; shifts within 1e-3 px, maxCC within 1e-5.
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


def _library(D, nrefs, seed=1):
    vol = synth.phantom(D, seed=seed, nblobs=14)
    refs, dirs = synth.make_refs(vol, nrefs)
    return refs


@pytest.fixture(scope="module")
def lib64():
    D, nrefs = 64, 48
    refs = _library(D, nrefs)
    rng = np.random.default_rng(3)
    parts, truth = synth.make_particles(refs, 37, rng, snr=0.1, max_shift=2)
    return D, refs, parts, truth


def test_reference_library_fp64(gpu, oracle, lib64):
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    assert (pm.N, pm.ncoef) == (o.N, o.ncoef)
    for r in (0, 5, len(refs) - 1):
        c, s = pm.debug_ref(r)
        ce, se = o.ref_coefs(r), o.ref_sigma(r)
        assert abs(s - se) <= 1e-12 * se
        assert np.abs(c - ce).max() <= 1e-12 * np.abs(ce).max()


@pytest.mark.parametrize("precision,tol", [(64, 1e-12), (32, 5e-6)])
def test_particle_polar_fourier_transform(gpu, oracle, lib64, precision, tol):
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    c, s = pm.debug_prepare(torch.from_numpy(parts[:6]).cuda(), precision)
    for i in range(6):
        fP, fPm, sig = o.prepare_particle(parts[i])
        assert abs(s[i] - sig) <= tol * sig
        assert np.abs(c[i] - fP).max() <= tol * np.abs(fP).max()
        assert np.allclose(fPm, np.conj(fP))


def test_correlation_rows_and_fp32_margin(gpu, oracle, lib64):
    """fp64 re-scorer == oracle to rounding; fp32 coarse pass within the ambiguity margin."""
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    scale = sum(2 * np.pi * r for r in range(o.Ri, o.Ro + 1))
    worst32 = 0.0
    for i, r in ((0, 0), (1, 7), (2, 47), (3, 20)):
        exp = o.corr_rows(parts[i], r)
        p = torch.from_numpy(parts[i:i + 1]).cuda()
        got64 = pm.debug_corr_rows(p, r, 64)
        got32 = pm.debug_corr_rows(p, r, 32)
        assert np.abs(got64 - exp).max() <= 1e-10 * scale
        worst32 = max(worst32, np.abs(got32 - exp).max() / scale)
        assert np.argmax(got64) == np.argmax(exp)
    print("fp32 coarse-pass error / scale:", worst32)
    # the exactness of the indices needs the fp32 error of the winner and of the runner-up below tau / 2 each:
    # the library's own margin, with a factor 4 of headroom on top
    assert worst32 <= pm.get_option("tau_rel") / 8


@pytest.mark.parametrize("kind", ["phantom", "noise"])
def test_fp32_error_distribution_at_full_size_against_the_margin(gpu, kind):
    """The ambiguity margin tau_rel is not a worst-case bound (one for 127 rings x 400 frequencies x a 2048-point transform is
    two orders above what happens) but a multiple of the MEASURED error of the coarse pass, so the measurement is a test: at
    256 px, coarse (fp32) against re-score (fp64, equal to the oracle to 1e-10 S: test above) rows of 24 particles x 8
    references, 3e5 samples per gallery kind: the largest error stays below tau_rel / 4 -- half of the tau / 2 the argument
    needs -- and the standard deviation below tau_rel / 20 (the errors are sums of ~1e5 roundings: tau / 2 is ten of these
    bounds away)."""
    xa, ctx, torch = gpu
    D, nrefs, n = 256, 8, 24
    g = torch.Generator(device="cuda").manual_seed(5)
    if kind == "phantom":
        vol = torch.from_numpy(synth.phantom(D, seed=4, nblobs=20).astype(np.float32)).cuda()
        fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
        refs = fp.project(np.concatenate([synth.fibonacci_directions(nrefs), np.zeros((nrefs, 1))], 1))
        fp.close()
        refs = ((refs - refs.mean()) / refs.std()).contiguous()
    else:
        refs = torch.randn((nrefs, D, D), generator=g, device="cuda")
    idx = torch.randint(0, nrefs, (n,), generator=g, device="cuda")
    parts = (refs[idx] + np.sqrt(10.0) * torch.randn((n, D, D), generator=g, device="cuda")).contiguous()
    pm = xa.ProjectionMatcher(ctx, refs)
    scale = sum(2 * np.pi * r for r in range(1, D // 2))
    errs = []
    for i in range(n):
        for r in range(nrefs):
            p = parts[i:i + 1].contiguous()
            errs.append(pm.debug_corr_rows(p, r, 32) - pm.debug_corr_rows(p, r, 64))
    e = np.concatenate(errs) / scale
    tau = pm.get_option("tau_rel")
    print(kind, "fp32 - fp64 over", e.size, "samples: max", np.abs(e).max(), "std", e.std(), "tau_rel", tau)
    assert np.abs(e).max() <= tau / 4
    assert e.std() <= tau / 20


@pytest.mark.parametrize("parity", [0, 1])
def test_match_dense_indices_bit_identical(gpu, oracle, lib64, parity):
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    refno, psi, flip = pm.match(torch.from_numpy(parts).cuda(), parity=parity)
    er, ep, ef, ecc = o.match(parts, parity=parity)
    assert np.array_equal(refno.cpu().numpy(), er[:, 0])
    assert np.array_equal(psi.cpu().numpy(), ep[:, 0])
    assert np.array_equal(flip.cpu().numpy(), ef[:, 0])
    st = pm.last_stats()
    assert st["rows"] == len(parts) * len(refs)
    print("rescored particles:", st["rescored_particles"], "of", len(parts))


def test_match_with_neighbour_lists_and_chunking(gpu, oracle, lib64):
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    rng = np.random.default_rng(11)
    n, nrefs = len(parts), len(refs)
    lists = []
    for i in range(n):
        k = int(rng.integers(0, 12)) if i != 4 else 0     # particle 4 has no neighbours
        lists.append(rng.choice(nrefs, size=k, replace=False))
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    ids = np.concatenate(lists).astype(np.int32)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    pm.set_option("chunk_rows", 50)   # forces several chunks
    o = oracle.PM(refs)
    refno, psi, flip = pm.match(torch.from_numpy(parts).cuda(), off, ids, parity=1)
    er, ep, ef, ecc = o.match(parts, off, ids, parity=1)
    assert np.array_equal(refno.cpu().numpy(), er[:, 0])
    assert refno[4].item() == -1
    valid = er[:, 0] >= 0
    assert np.array_equal(psi.cpu().numpy()[valid], ep[valid, 0])
    assert np.array_equal(flip.cpu().numpy()[valid], ef[valid, 0])


def test_ascending_neighbour_lists_run_over_the_bank_with_a_mask(gpu, oracle, lib64):
    """A local search whose lists are non-empty and ascending (a sampling file's) goes through the matrix-core contraction
    of the whole bank, the off-list references dropped by the branch and bound: same answers as the oracle's list search
    and as the gather path, rows counted as listed; several chunks."""
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    rng = np.random.default_rng(12)
    n, nrefs = len(parts), len(refs)
    lists = [np.sort(rng.choice(nrefs, size=int(rng.integers(1, 12)), replace=False)) for _ in range(n)]
    lists[3] = np.array([7])      # a single neighbour
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    ids = np.concatenate(lists).astype(np.int32)
    dp = torch.from_numpy(parts).cuda()
    o = oracle.PM(refs)
    er, ep, ef, ecc = o.match(parts, off, ids, parity=1)
    for chunk_rows in (0, 3 * nrefs):
        pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
        if chunk_rows:
            pm.set_option("chunk_rows", chunk_rows)
        got = [t.cpu().numpy() for t in pm.match(dp, off, ids, parity=1)]
        st = pm.last_stats()
        assert st["rows"] == len(ids) and st["pruned_rows"] >= 0
        assert np.array_equal(got[0], er[:, 0]) and np.array_equal(got[1], ep[:, 0]) and np.array_equal(got[2], ef[:, 0])
        pm.set_option("mask_lists", 0)
        gather = [t.cpu().numpy() for t in pm.match(dp, off, ids, parity=1)]
        for a, b in zip(got, gather):
            assert np.array_equal(a, b)


def test_lists_that_name_every_reference_in_order_are_the_dense_search(gpu, oracle, lib64):
    """A global search written as neighbour lists (what the gallery's sampling file holds with --angular_distance -1)
    takes the dense MFMA path with its branch and bound; a single list in another order does not."""
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    n, nrefs = len(parts), len(refs)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    dp = torch.from_numpy(parts).cuda()
    dense = [t.cpu().numpy() for t in pm.match(dp, parity=1)]
    dense_pruned = pm.last_stats()["pruned_rows"]
    off = (np.arange(n + 1) * nrefs).astype(np.int32)
    ids = np.tile(np.arange(nrefs, dtype=np.int32), n)
    same = [t.cpu().numpy() for t in pm.match(dp, off, ids, parity=1)]
    assert pm.last_stats()["pruned_rows"] == dense_pruned > 0
    for a, b in zip(dense, same):
        assert np.array_equal(a, b)
    ids2 = ids.copy()
    ids2[:nrefs] = ids2[:nrefs][::-1]                  # particle 0 visits the bank backwards
    other = [t.cpu().numpy() for t in pm.match(dp, off, ids2, parity=1)]
    assert pm.last_stats()["pruned_rows"] == 0
    er, ep, ef, _ = oracle.PM(refs).match(parts, off, ids2, parity=1)
    for a, e in zip(other, (er[:, 0], ep[:, 0], ef[:, 0])):
        assert np.array_equal(a, e)


def test_match_any_box_size(gpu, oracle):
    """D=50: nothing on the rotational path needs a power of two (ring DFTs are direct, the length-N
    inverse DFT is Bluestein anyway); the CTF-filtered gallery uses a 75x75 Bluestein FFT (pad 1.5)."""
    xa, ctx, torch = gpu
    D, nrefs, n = 50, 20, 15
    refs = _library(D, nrefs, seed=6)
    rng = np.random.default_rng(12)
    parts, truth = synth.make_particles(refs, n, rng, snr=0.2, max_shift=2)
    paddim = 75
    fy = np.fft.fftfreq(paddim)[:, None]
    fx = np.fft.fftfreq(paddim)[None, :]
    Mctf = np.cos(40.0 * (fx * fx + fy * fy)) * np.exp(-6.0 * (fx * fx + fy * fy))
    for M, pd in ((None, 0), (Mctf, paddim)):
        pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda(), Mctf=M, paddim=pd)
        o = oracle.PM(refs, Mctf=M, paddim=pd)
        refno, psi, flip = pm.match(torch.from_numpy(parts).cuda())
        er, ep, ef, _ = o.match(parts)
        assert np.array_equal(refno.cpu().numpy(), er[:, 0])
        assert np.array_equal(psi.cpu().numpy(), ep[:, 0])
        assert np.array_equal(flip.cpu().numpy(), ef[:, 0])


def test_config2_shape_d128_many_references(gpu, oracle):
    """BASELINE config 2 in small: 128-px particles (N=394, Bluestein M=1024, MFMA contraction and ring DFT,
    register-blocked S6) against 300 references, all of them neighbours; SNR 0.1."""
    xa, ctx, torch = gpu
    D, nrefs, n = 128, 300, 40
    vol = synth.phantom(D, seed=3, nblobs=20)
    refs, dirs = synth.make_refs(vol, nrefs)
    rng = np.random.default_rng(17)
    parts, truth = synth.make_particles(refs, n, rng, snr=0.1, max_shift=3)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    assert pm.N == o.N == 394
    refno, psi, flip = pm.match(torch.from_numpy(parts).cuda(), parity=1)
    er, ep, ef, _ = o.match(parts, parity=1)
    assert np.array_equal(refno.cpu().numpy(), er[:, 0])
    assert np.array_equal(psi.cpu().numpy(), ep[:, 0])
    assert np.array_equal(flip.cpu().numpy(), ef[:, 0])
    sx, sy, cc = pm.translate(torch.from_numpy(parts).cuda(), refno, psi, flip, 10.0)
    ex, ey, ec = o.translate(parts, er[:, 0], ep[:, 0], ef[:, 0], 10.0)
    assert np.abs(sx.cpu().numpy() - ex).max() <= 1e-3 and np.abs(sy.cpu().numpy() - ey).max() <= 1e-3
    assert np.abs(cc.cpu().numpy() - ec).max() <= 1e-5


def test_config2_at_its_own_reference_count(gpu, oracle):
    """BASELINE config 2 at its own shape: 128-px particles against 1000 reference projections (the whole gallery as every
    particle's neighbourhood), 64 particles of the bench's kind (SNR 0.1, shifts up to 3 px); orientation indices bit for bit,
    shifts and maxCC as everywhere.  (VERDICT r05 test hole a: until round 6 this shape ran against 300 references only.)"""
    xa, ctx, torch = gpu
    D, nrefs, n = 128, 1000, 64
    vol = synth.phantom(D, seed=5, nblobs=20)
    # the gallery through the library's own projector (xmipp_angular_project_library's path; synth.make_refs takes minutes for 1000)
    dirs = synth.fibonacci_directions(nrefs)
    fpj = xa.FourierProjector(ctx, torch.from_numpy(vol.astype(np.float32)).cuda(), 2.0, 0.5, 3)
    refs = fpj.project(np.concatenate([dirs, np.zeros((nrefs, 1))], 1)).cpu().numpy()
    fpj.close()
    refs = ((refs - refs.mean()) / refs.std()).astype(np.float32)
    rng = np.random.default_rng(29)
    parts, truth = synth.make_particles(refs, n, rng, snr=0.1, max_shift=3)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    assert pm.N == o.N == 394
    dp = torch.from_numpy(parts).cuda()
    refno, psi, flip = pm.match(dp)
    er, ep, ef, _ = o.match(parts)
    assert np.array_equal(refno.cpu().numpy(), er[:, 0])
    assert np.array_equal(psi.cpu().numpy(), ep[:, 0])
    assert np.array_equal(flip.cpu().numpy(), ef[:, 0])
    sx, sy, cc = pm.translate(dp, refno, psi, flip, 10.0)
    ex, ey, ec = o.translate(parts, er[:, 0], ep[:, 0], ef[:, 0], 10.0)
    assert np.abs(sx.cpu().numpy() - ex).max() <= 1e-3 and np.abs(sy.cpu().numpy() - ey).max() <= 1e-3
    assert np.abs(cc.cpu().numpy() - ec).max() <= 1e-5
    # and with explicit lists of all 1000 references in stack order (what a _sampling.xmd of this configuration holds): same answer
    off = (np.arange(n + 1) * nrefs).astype(np.int32)
    ids = np.tile(np.arange(nrefs, dtype=np.int32), n)
    r2, p2, f2 = pm.match(dp, off, ids)
    assert torch.equal(r2, refno) and torch.equal(p2, psi) and torch.equal(f2, flip)


@pytest.mark.parametrize("kind", ["phantom", "noise", "flat", "pure_noise_particles"])
def test_branch_and_bound_of_the_row_transforms_changes_nothing(gpu, oracle, kind):
    """S3 skips rows whose coefficient moduli cannot reach the particle's best value minus two ambiguity margins
    (k_pm_prune_plan). Same indices with the pruning on and off, both equal to the oracle; how much is pruned depends
    on the data: references that look alike (phantom) or not at all (noise), particles without any signal."""
    xa, ctx, torch = gpu
    D, nrefs, n = 64, 96, 24
    rng = np.random.default_rng(5)
    if kind == "noise":
        refs = rng.standard_normal((nrefs, D, D))
        f = np.fft.fftfreq(D)
        lp = np.exp(-((f[:, None] ** 2 + f[None, :] ** 2) * (0.12 * D) ** 2))
        refs = np.fft.ifft2(np.fft.fft2(refs) * lp).real
        refs = (refs / refs.std()).astype(np.float32)
    else:
        refs, _ = synth.make_refs(synth.phantom(D, seed=2, nblobs=14), nrefs)
        if kind == "flat":
            refs = (refs + 10.0).astype(np.float32)        # a large constant: every row is dominated by its DC term
    if kind == "pure_noise_particles":
        parts = rng.standard_normal((n, D, D)).astype(np.float32)
    else:
        parts, _ = synth.make_particles(refs, n, rng, snr=0.1, max_shift=2)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    dp = torch.from_numpy(parts).cuda()
    on = [t.cpu().numpy() for t in pm.match(dp)]
    st = pm.last_stats()
    assert st["rows"] == n * nrefs and 0 <= st["pruned_rows"] < st["rows"]
    K0, nk = pm.two_level_cut()
    assert 8 <= K0 <= nk
    # the two-level contraction at other cuts (and switched off): same indices
    others = []
    pm.set_option("group_high", 0)          # the surviving rows finished one by one instead of particle by particle (k_pm_rows_high)
    others.append([t.cpu().numpy() for t in pm.match(dp)])
    pm.set_option("group_high", 1)
    pm.set_option("high_cap", 13)           # ... and with room for thirteen rows in the store: the rest take the other form in the same launch
    others.append([t.cpu().numpy() for t in pm.match(dp)])
    pm.set_option("high_cap", 0)
    for k0 in (8, 20, nk):
        pm.set_option("k0", k0)
        others.append([t.cpu().numpy() for t in pm.match(dp)])
    pm.set_option("k0", 0)
    assert pm.two_level_cut()[0] == K0
    pm.set_option("prune", 0)
    off = [t.cpu().numpy() for t in pm.match(dp)]
    assert pm.last_stats()["pruned_rows"] == 0
    for o_ in others:
        for a, b in zip(o_, off):
            assert np.array_equal(a, b)
    er, ep, ef, _ = oracle.PM(refs).match(parts)
    for a, b, e in zip(on, off, (er[:, 0], ep[:, 0], ef[:, 0])):
        assert np.array_equal(a, b) and np.array_equal(a, e)
    if kind == "noise":
        assert st["pruned_rows"] > 0.5 * st["rows"]        # unrelated references: almost nothing can reach the true match
    print(kind, "pruned", st["pruned_rows"], "of", st["rows"], "rescored rows", st["rescored_rows"], "K0", K0, "of", nk)


@pytest.mark.parametrize("kind", ["phantom", "noise"])
def test_branch_and_bound_at_full_size(gpu, kind):
    """BASELINE config 4 shape (256 px, 1000 references, 2048 particles at SNR 0.1): the pruned, two-level search and
    the exhaustive one give the same (reference, angle, mirror) for every particle, and so do other cuts K0."""
    xa, ctx, torch = gpu
    D, nrefs, n = 256, 1000, 2048
    g = torch.Generator(device="cuda").manual_seed(11)
    if kind == "phantom":
        vol = torch.from_numpy(synth.phantom(D, seed=4, nblobs=20).astype(np.float32)).cuda()
        fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
        dirs = synth.fibonacci_directions(nrefs)
        refs = fp.project(np.concatenate([dirs, np.zeros((nrefs, 1))], 1))
        fp.close()
        refs = ((refs - refs.mean()) / refs.std()).contiguous()
    else:
        x = torch.randn((nrefs, D, D), generator=g, device="cuda")
        f = torch.fft.rfft2(x)
        ky = torch.fft.fftfreq(D, device="cuda")[:, None]
        kx = torch.fft.rfftfreq(D, device="cuda")[None, :]
        refs = torch.fft.irfft2(f * torch.exp(-2 * (np.pi * 3.0) ** 2 * (kx * kx + ky * ky)), s=(D, D))
        refs = (refs / refs.std()).contiguous()
    idx = torch.randint(0, nrefs, (n,), generator=g, device="cuda")
    parts = (refs[idx] + np.sqrt(10.0) * torch.randn((n, D, D), generator=g, device="cuda")).contiguous()
    pm = xa.ProjectionMatcher(ctx, refs)
    on = [t.cpu().numpy() for t in pm.match(parts)]
    st = pm.last_stats()
    K0, nk = pm.two_level_cut()
    assert st["pruned_rows"] > 0.9 * st["rows"]
    pm.set_option("k0", 64 if K0 != 64 else 96)
    other = [t.cpu().numpy() for t in pm.match(parts)]
    pm.set_option("prune", 0)
    off = [t.cpu().numpy() for t in pm.match(parts)]
    for a, b, c in zip(on, other, off):
        assert np.array_equal(a, c) and np.array_equal(b, c)
    if kind == "noise":       # unrelated references: the true one wins (neighbouring phantom projections look alike)
        assert (on[0] == idx.cpu().numpy()).mean() > 0.95
    print(kind, "pruned", st["pruned_rows"] / st["rows"], "K0", K0, "of", nk, "rescored particles", st["rescored_particles"])


def test_many_surviving_rows_switch_the_next_chunk_to_the_full_contraction(gpu, oracle):
    """A gallery whose rows mostly survive the bounds (here: a large constant added to every reference) is cheaper contracted at
    every frequency with the coefficients kept than finished row by row (xh_pm.hip, adaptive_finish): the survivors of one chunk
    decide the form of the next.  Same indices in either form, equal to the oracle's; a friendly batch switches back."""
    xa, ctx, torch = gpu
    D, nrefs, n = 64, 96, 40
    rng = np.random.default_rng(15)
    refs, _ = synth.make_refs(synth.phantom(D, seed=2, nblobs=14), nrefs)
    flat = (refs + 10.0).astype(np.float32)
    parts, _ = synth.make_particles(flat, n, rng, snr=0.1, max_shift=2)
    er, ep, ef, _ = oracle.PM(flat).match(parts)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(flat).cuda())
    dp = torch.from_numpy(parts).cuda()
    pm.set_option("adaptive_finish", 0)
    base = [t.cpu().numpy() for t in pm.match(dp)]
    st = pm.last_stats()
    assert st["pruned_rows"] < 0.8 * st["rows"], st           # the premise: more than a fifth of the rows survive
    assert pm.get_option("dense_chunks") == 0
    pm.set_option("adaptive_finish", 1)
    pm.set_option("chunk_rows", 10 * nrefs)                    # four chunks of ten particles
    first = [t.cpu().numpy() for t in pm.match(dp)]
    assert pm.get_option("dense_chunks") == 3                  # the first chunk found out
    second = [t.cpu().numpy() for t in pm.match(dp)]
    assert pm.get_option("dense_chunks") == 4
    K0, nk = pm.two_level_cut()
    assert K0 < nk                                             # (the configured cut is what the handle reports, whatever the chunks ran with)
    for got in (first, second):
        for a, b, e in zip(got, base, (er[:, 0], ep[:, 0], ef[:, 0])):
            assert np.array_equal(a, b) and np.array_equal(a, e)
    # neighbour lists that run over the bank with a mask take the same switch
    k = 24
    ids = np.stack([np.sort(rng.choice(nrefs, k, replace=False)) for _ in range(n)]).astype(np.int32)
    off = (np.arange(n + 1) * k).astype(np.int32)
    lr, lp, lf, _ = oracle.PM(flat).match(parts, off, ids.ravel())
    got = [t.cpu().numpy() for t in pm.match(dp, off, ids.ravel())]
    for a, e in zip(got, (lr[:, 0], lp[:, 0], lf[:, 0])):
        assert np.array_equal(a, e)
    # ... and an ordinary gallery switches back after its first chunk
    pm2 = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    parts2, _ = synth.make_particles(refs, n, rng, snr=0.1, max_shift=2)
    dp2 = torch.from_numpy(parts2).cuda()
    pm2.set_option("adaptive_finish", 2)                       # start in the dense form
    pm2.set_option("chunk_rows", 10 * nrefs)
    g2 = [t.cpu().numpy() for t in pm2.match(dp2)]
    dense2 = pm2.get_option("dense_chunks")
    st2 = pm2.last_stats()
    r2, p2, f2, _ = oracle.PM(refs).match(parts2)
    for a, e in zip(g2, (r2[:, 0], p2[:, 0], f2[:, 0])):
        assert np.array_equal(a, e)
    if st2["pruned_rows"] > 0.95 * st2["rows"]:
        assert dense2 == 1, dense2
    print("flat gallery pruned", st["pruned_rows"], "of", st["rows"], "; ordinary gallery dense chunks", dense2, "pruned", st2["pruned_rows"], "of", st2["rows"])


def test_full_contraction_of_a_flat_peaked_map_at_full_size(gpu, oracle):
    """BASELINE config 4 shape with the compact phantom (every blob within 0.3 of the box radius: nearly rotation invariant) and particles
    that are rotated, mirrored and shifted: a large part of the rows survives the bounds.  The chunks contracted at every frequency with
    their coefficients kept (adaptive_finish 2: from the first chunk on) give the indices of the two-level form, and a sample of them the oracle's."""
    import math
    xa, ctx, torch = gpu
    D, nrefs, n = 256, 1000, 1536
    g = torch.Generator(device="cuda").manual_seed(21)
    vol = torch.from_numpy(synth.phantom(D, seed=9, nblobs=20).astype(np.float32)).cuda()
    fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
    dirs = synth.fibonacci_directions(nrefs)
    refs = fp.project(np.concatenate([dirs, np.zeros((nrefs, 1))], 1))
    fp.close()
    refs = ((refs - refs.mean()) / refs.std()).contiguous()
    idx = torch.randint(0, nrefs, (n,), generator=g, device="cuda")
    th = torch.rand((n,), generator=g, device="cuda") * (2 * math.pi)
    mir = (torch.rand((n,), generator=g, device="cuda") < 0.5).float() * 2 - 1
    rot = torch.zeros((n, 2, 3), device="cuda")
    rot[:, 0, 0] = torch.cos(th) * mir; rot[:, 0, 1] = -torch.sin(th); rot[:, 1, 0] = torch.sin(th) * mir; rot[:, 1, 1] = torch.cos(th)
    rot[:, :, 2] = torch.randint(-3, 4, (n, 2), generator=g, device="cuda").float() * (2.0 / D)
    parts = torch.empty((n, D, D), device="cuda")
    for b0 in range(0, n, 512):
        sl = slice(b0, b0 + 512)
        grid = torch.nn.functional.affine_grid(rot[sl], (rot[sl].shape[0], 1, D, D), align_corners=False)
        parts[sl] = torch.nn.functional.grid_sample(refs[idx[sl]][:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
    parts = (parts + math.sqrt(10.0) * torch.randn((n, D, D), generator=g, device="cuda")).contiguous()
    pm = xa.ProjectionMatcher(ctx, refs)
    pm.set_option("adaptive_finish", 0)
    two_level = [t.cpu().numpy() for t in pm.match(parts)]
    st = pm.last_stats()
    assert pm.get_option("dense_chunks") == 0
    pm.set_option("adaptive_finish", 2)
    full = [t.cpu().numpy() for t in pm.match(parts)]
    assert pm.get_option("dense_chunks") >= 1
    for a, b in zip(two_level, full):
        assert np.array_equal(a, b)
    m = 24
    er, ep, ef, _ = oracle.PM(refs.cpu().numpy()).match(parts[:m].cpu().numpy())
    for a, e in zip(full, (er[:, 0], ep[:, 0], ef[:, 0])):
        assert np.array_equal(a[:m], e)
    print("survived the bounds:", 1 - st["pruned_rows"] / st["rows"], "re-scored particles", st["rescored_particles"], "of", n,
          "; chunks contracted in full:", pm.get_option("dense_chunks"))


@pytest.mark.parametrize("D", [512, 24])
def test_match_extreme_box_sizes(gpu, oracle, D):
    """512 px: N=1602, Bluestein M=4096 (radix-2 LDS S3 kernel), 255 rings, nk=802; 24 px: M=256 (radix-2 too)."""
    xa, ctx, torch = gpu
    nrefs, n = (5, 3) if D == 512 else (16, 9)
    rng = np.random.default_rng(D)
    refs = rng.standard_normal((nrefs, D, D)).astype(np.float32)
    f = np.fft.fftfreq(D)
    lp = np.exp(-((f[:, None] ** 2 + f[None, :] ** 2) * (0.12 * D) ** 2))
    refs = np.fft.ifft2(np.fft.fft2(refs) * lp).real.astype(np.float32)
    parts = np.stack([refs[i % nrefs] + 0.5 * refs.std() * rng.standard_normal((D, D)) for i in range(n)]).astype(np.float32)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    assert pm.N == o.N
    refno, psi, flip = pm.match(torch.from_numpy(parts).cuda())
    er, ep, ef, _ = o.match(parts)
    assert np.array_equal(refno.cpu().numpy(), er[:, 0])
    assert np.array_equal(psi.cpu().numpy(), ep[:, 0])
    assert np.array_equal(flip.cpu().numpy(), ef[:, 0])
    sx, sy, cc = pm.translate(torch.from_numpy(parts).cuda(), refno, psi, flip, 5.0)
    ex, ey, ec = o.translate(parts, er[:, 0], ep[:, 0], ef[:, 0], 5.0)
    assert np.abs(sx.cpu().numpy() - ex).max() <= 1e-3 and np.abs(sy.cpu().numpy() - ey).max() <= 1e-3
    assert np.abs(cc.cpu().numpy() - ec).max() <= 1e-5


def test_exact_ties_follow_the_visiting_order(gpu, oracle, lib64):
    """Duplicated references give bit-equal correlations in the reference: the first visited
    wins, and the visiting order flips every image (APM:615-626,1112)."""
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    refs2 = np.concatenate([refs[:10], refs[3:4], refs[10:20], refs[3:4]])  # ref 3 also at 10 and 21
    rng = np.random.default_rng(21)
    pp = np.stack([refs2[3] + 0.3 * refs2[3].std() * rng.standard_normal((D, D)).astype(np.float32) for _ in range(6)])
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs2).cuda())
    o = oracle.PM(refs2)
    for parity in (0, 1):
        refno, psi, flip = pm.match(torch.from_numpy(pp).cuda(), parity=parity)
        er, ep, ef, _ = o.match(pp, parity=parity)
        assert set(er[:, 0]) <= {3, 10, 21}
        assert np.array_equal(refno.cpu().numpy(), er[:, 0])
        assert np.array_equal(psi.cpu().numpy(), ep[:, 0])
        assert np.array_equal(flip.cpu().numpy(), ef[:, 0])
    assert pm.last_stats()["rescored_particles"] == 6


@pytest.mark.parametrize("thr", [2, 3, 4])
def test_exact_ties_follow_the_worker_threads_of_thr(gpu, oracle, lib64, thr):
    """--thr n (APM:631,1018-1108): worker c of n takes the list positions i % n == c in the image's visiting order, the workers'
    results are merged, worker 0 first, strictly greater wins.  With duplicated references at list positions 3, 10 and 21 the winner
    is decided by (position % n, visiting order) -- 10 for n = 2 (3 % 2 = 1, 10 % 2 = 0, 21 % 2 = 1), 3 / 21 alternating for n = 3
    (all three positions are worker 0's), 3 / 10 ... -- and the device (option "threads") follows the oracle's restatement of it;
    lists in any order (gathered rows), ascending lists (they lose the whole-bank mode with threads > 1) and the running top-N too."""
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    refs2 = np.concatenate([refs[:10], refs[3:4], refs[10:20], refs[3:4]])  # ref 3 also at 10 and 21
    rng = np.random.default_rng(21)
    pp = np.stack([refs2[3] + 0.3 * refs2[3].std() * rng.standard_normal((D, D)).astype(np.float32) for _ in range(6)])
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs2).cuda())
    pm.set_option("threads", thr)
    o = oracle.PM(refs2)
    dp = torch.from_numpy(pp).cuda()
    seen = set()
    for parity in (0, 1):
        refno, psi, flip = pm.match(dp, parity=parity)
        er, ep, ef, _ = o.match(pp, parity=parity, ref_threads=thr)
        assert set(er[:, 0]) <= {3, 10, 21}
        assert np.array_equal(refno.cpu().numpy(), er[:, 0]) and np.array_equal(psi.cpu().numpy(), ep[:, 0]) and np.array_equal(flip.cpu().numpy(), ef[:, 0])
        seen |= set(er[:, 0])
        e1 = o.match(pp, parity=parity)[0]
        if thr == 2:
            assert (er[:, 0] == 10).all() and not np.array_equal(e1[:, 0], er[:, 0])       # the order of --thr 1 gives 3 / 21
    # neighbour lists: positions in the LIST decide (here the duplicates sit at list positions 0, 1, 2 of a shuffled / ascending list)
    for ascending in (False, True):
        lists = [np.array([21, 3, 10, 5, 7, 12][:5 + (i % 2)]) for i in range(6)]
        if ascending:
            lists = [np.sort(l) for l in lists]
        off = np.zeros(7, np.int32)
        off[1:] = np.cumsum([len(l) for l in lists])
        ids = np.concatenate(lists).astype(np.int32)
        refno, psi, flip = pm.match(dp, off, ids, parity=1)
        er, ep, ef, _ = o.match(pp, off, ids, parity=1, ref_threads=thr)
        assert np.array_equal(refno.cpu().numpy(), er[:, 0]) and np.array_equal(psi.cpu().numpy(), ep[:, 0]) and np.array_equal(flip.cpu().numpy(), ef[:, 0])
    # the running top-N of every worker and their merge
    refno, psi, flip = pm.match(dp, parity=0, n_orient=3)
    er, ep, ef, _ = o.match(pp, parity=0, n_orient=3, ref_threads=thr)
    assert np.array_equal(refno.cpu().numpy(), er)
    valid = er >= 0
    assert np.array_equal(psi.cpu().numpy()[valid], ep[valid]) and np.array_equal(flip.cpu().numpy()[valid], ef[valid])
    pm.set_option("threads", 1)
    refno, _, _ = pm.match(dp, parity=0)
    assert np.array_equal(refno.cpu().numpy(), o.match(pp, parity=0)[0][:, 0])


@pytest.mark.parametrize("mode", ["dense", "lists", "ascending_lists"])
def test_5d_search_indices_bit_identical(gpu, oracle, lib64, mode):
    """--search5d_shift 3 --search5d_step 2 (APM:321-348,575-589,676): 9 extra polar transforms per
    particle, every (reference, translation) pair competes; only (refno, psi, flip) are kept."""
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    xo, yo = xa.search5d_offsets(3, 2)
    assert len(xo) == 9 and (xo[4], yo[4]) == (0, 0)
    n = 21
    off = ids = None
    if mode != "dense":
        rng = np.random.default_rng(5)
        lists = [rng.choice(len(refs), size=int(rng.integers(1, 9)), replace=False) for _ in range(n)]
        if mode == "ascending_lists":         # the matrix-core path with the off-list references masked
            lists = [np.sort(l) for l in lists]
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(l) for l in lists])
        ids = np.concatenate(lists).astype(np.int32)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    if mode != "dense":
        pm.set_option("chunk_rows", 300 if mode == "lists" else 3 * 9 * len(refs))
    o = oracle.PM(refs)
    refno, psi, flip = pm.match(torch.from_numpy(parts[:n]).cuda(), off, ids, parity=1, shifts5d=(xo, yo))
    er, ep, ef, _ = o.match(parts[:n], off, ids, parity=1, xoff5d=xo, yoff5d=yo)
    assert np.array_equal(refno.cpu().numpy(), er[:, 0])
    assert np.array_equal(psi.cpu().numpy(), ep[:, 0])
    assert np.array_equal(flip.cpu().numpy(), ef[:, 0])
    # the search is not a no-op: some particles pick a different orientation than without it
    r0, p0, f0, _ = o.match(parts[:n], off, ids, parity=1)
    print("particles whose winner changed with the 5-D search:", int((r0[:, 0] != er[:, 0]).sum() + (p0[:, 0] != ep[:, 0]).sum()))
    assert pm.last_stats()["rows"] == (n * len(refs) * 9 if mode == "dense" else int(off[-1]) * 9)


@pytest.mark.parametrize("n_orient,shifts", [(3, None), (5, (1, 1))])
def test_number_orientations_running_top_n(gpu, oracle, lib64, n_orient, shifts):
    """--number_orientations > 1 reproduces the reference's running top-N (APM:714-735), including
    its quirks (ranks are not shifted down; rank n only accepts values below rank n-1)."""
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    n = 12
    sh = xa.search5d_offsets(*shifts) if shifts else None
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    for parity in (0, 1):
        refno, psi, flip = pm.match(torch.from_numpy(parts[:n]).cuda(), parity=parity, n_orient=n_orient, shifts5d=sh)
        kw = dict(xoff5d=sh[0], yoff5d=sh[1]) if sh else {}
        er, ep, ef, _ = o.match(parts[:n], parity=parity, n_orient=n_orient, **kw)
        assert refno.shape == (n, n_orient)
        assert np.array_equal(refno.cpu().numpy(), er)
        valid = er >= 0
        assert np.array_equal(psi.cpu().numpy()[valid], ep[valid])
        assert np.array_equal(flip.cpu().numpy()[valid], ef[valid])
        assert valid[:, 0].all()


def test_number_orientations_with_short_lists(gpu, oracle, lib64):
    """fewer candidates than ranks / empty lists leave refno = -1 (counterValidCorrs, APM:1068-1090)."""
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    n = 5
    lists = [[7], [], [3, 9], [1, 2, 3], [40]]
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    ids = np.concatenate([np.asarray(l, np.int32) for l in lists]).astype(np.int32)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    refno, psi, flip = pm.match(torch.from_numpy(parts[:n]).cuda(), off, ids, n_orient=4)
    er, ep, ef, _ = o.match(parts[:n], off, ids, n_orient=4)
    assert np.array_equal(refno.cpu().numpy(), er)
    assert (refno[1] == -1).all()
    valid = er >= 0
    assert np.array_equal(psi.cpu().numpy()[valid], ep[valid])
    assert np.array_equal(flip.cpu().numpy()[valid], ef[valid])


def test_translational_alignment(gpu, oracle, lib64):
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    er, ep, ef, _ = o.match(parts)
    er, ep, ef = er[:, 0].copy(), ep[:, 0].copy(), ef[:, 0].copy()
    er[5] = -1
    for max_shift in (-1.0, 1.5):
        sx, sy, cc = pm.translate(torch.from_numpy(parts).cuda(), torch.from_numpy(er).cuda(),
                                  torch.from_numpy(ep).cuda(), torch.from_numpy(ef).cuda(), max_shift)
        ex, ey, ec = o.translate(parts, er, ep, ef, max_shift)
        assert np.abs(sx.cpu().numpy() - ex).max() <= 1e-3
        assert np.abs(sy.cpu().numpy() - ey).max() <= 1e-3
        assert np.abs(cc.cpu().numpy() - ec).max() <= 1e-5


@pytest.mark.parametrize("D", [32, 128, 256, 50, 45])
def test_translational_alignment_other_sizes(gpu, oracle, D):
    """D = 64/128/256 take the register-blocked three-kernel path, other powers of two the radix-2 one,
    everything else (50, 45) the Bluestein line transforms of xh_plan.h."""
    xa, ctx, torch = gpu
    nrefs, n = 6, 7
    refs = _library(D, nrefs, seed=2)
    rng = np.random.default_rng(8)
    parts, truth = synth.make_particles(refs, n, rng, snr=0.5, max_shift=3)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    N = o.N
    er = rng.integers(0, nrefs, n).astype(np.int32)
    ep = rng.integers(0, N, n).astype(np.int32)
    ef = rng.integers(0, 2, n).astype(np.uint8)
    for i in range(n):      # half of them at the true orientation so that real peaks are tested too
        if i % 2 == 0:
            er[i] = truth[i][0]
    sx, sy, cc = pm.translate(torch.from_numpy(parts).cuda(), torch.from_numpy(er).cuda(), torch.from_numpy(ep).cuda(),
                              torch.from_numpy(ef).cuda(), 6.0)
    ex, ey, ec = o.translate(parts, er, ep, ef, 6.0)
    assert np.abs(sx.cpu().numpy() - ex).max() <= 1e-3
    assert np.abs(sy.cpu().numpy() - ey).max() <= 1e-3
    assert np.abs(cc.cpu().numpy() - ec).max() <= 1e-5


@pytest.mark.parametrize("pad", [1, 2])
def test_ctf_filtered_gallery(gpu, oracle, lib64, pad):
    """--ctf: the references are filtered (pad, FFT, x Mctf, IFFT, crop) before the polar transform (APM:457-481)."""
    xa, ctx, torch = gpu
    D, refs, parts, truth = lib64
    P = pad * D
    f = np.fft.fftfreq(P)
    r2 = f[:, None] ** 2 + f[None, :] ** 2
    Mctf = -np.sin(900.0 * r2 + 0.3) * np.exp(-8.0 * r2)          # even in both axes, like generateCTF
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda(), Mctf=Mctf, paddim=P)
    o = oracle.PM(refs, Mctf=Mctf, paddim=P)
    for r in (0, 11):
        c, s = pm.debug_ref(r)
        ce, se = o.ref_coefs(r), o.ref_sigma(r)
        assert abs(s - se) <= 1e-10 * se and np.abs(c - ce).max() <= 1e-10 * np.abs(ce).max()
    refno, psi, flip = pm.match(torch.from_numpy(parts).cuda())
    er, ep, ef, _ = o.match(parts)
    assert np.array_equal(refno.cpu().numpy(), er[:, 0]) and np.array_equal(psi.cpu().numpy(), ep[:, 0])
    sx, sy, cc = pm.translate(torch.from_numpy(parts).cuda(), refno, psi, flip)
    ex, ey, ec = o.translate(parts, er[:, 0], ep[:, 0], ef[:, 0])
    assert np.abs(sx.cpu().numpy() - ex).max() <= 1e-3 and np.abs(cc.cpu().numpy() - ec).max() <= 1e-5


def test_errors_are_loud(gpu):
    xa, ctx, torch = gpu
    refs = torch.zeros((2, 64, 64), device="cuda")
    with pytest.raises(xa.XhError):
        xa.ProjectionMatcher(ctx, refs, Ri=10, Ro=5)
    pm = xa.ProjectionMatcher(ctx, torch.rand((2, 64, 64), device="cuda"))
    with pytest.raises(xa.XhError):
        pm.match(torch.rand((1, 64, 64), device="cuda"), np.array([0, 1], np.int32), np.array([7], np.int32))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_translation_fp32_pass_with_double_precision_repeats(gpu, oracle, D):
    """xh_pm_translate runs its chain in fp32 and repeats in double precision every particle whose arg-max or window
    decision (filters.cpp:1659-1689) comes within 2e-5 |max| of flipping. Against the all-double chain on the same device:
    no discrete decision differs (shifts within 1e-4 px, far below a window step), maxCC within 1e-6; a sizeable fraction,
    but not all, of the particles stays fp32."""
    xa, ctx, torch = gpu
    nrefs, n = 12, 301
    refs = _library(D, nrefs, seed=4)
    rng = np.random.default_rng(D)
    parts, truth = synth.make_particles(refs, n, rng, snr=0.1, max_shift=3)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    dp = torch.from_numpy(parts).cuda()
    refno, psi, flip = pm.match(dp)
    fast = [t.cpu().numpy() for t in pm.translate(dp, refno, psi, flip)]
    rep = pm.translate_repeated()
    pm.set_option("s6_fp32", 0)
    full = [t.cpu().numpy() for t in pm.translate(dp, refno, psi, flip)]
    assert pm.translate_repeated() == 0
    assert np.abs(fast[0] - full[0]).max() <= 1e-4 and np.abs(fast[1] - full[1]).max() <= 1e-4
    assert np.abs(fast[2] - full[2]).max() <= 1e-6
    assert 0 <= rep < n // 2


def test_full_size_matching_against_the_oracle(gpu, oracle):
    """BASELINE config 2 / 4 at their own box: 256 px, 1000 references (projections of the 20-Gaussian phantom at
    Fibonacci-sphere directions, made by the library's projector), 160 particles at SNR 0.1 with in-plane rotation, mirror and
    shifts: reference, in-plane angle and mirror identical to the oracle for every particle, shifts 1e-3 px, maxCC 1e-5 --
    with the branch and bound, the two-level contraction and the fp32-first translational pass all in their default state."""
    xa, ctx, torch = gpu
    D, nrefs, n = 256, 1000, 160
    vol = torch.from_numpy(synth.phantom(D, seed=4, nblobs=20).astype(np.float32)).cuda()
    fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
    refs = fp.project(np.concatenate([synth.fibonacci_directions(nrefs), np.zeros((nrefs, 1))], 1))
    fp.close()
    refs = ((refs - refs.mean()) / refs.std()).contiguous()
    h_refs = refs.cpu().numpy()
    rng = np.random.default_rng(23)
    pick = rng.integers(0, nrefs, n)
    parts, truth = synth.make_particles(h_refs[pick], n, rng, snr=0.1, max_shift=3)
    pm = xa.ProjectionMatcher(ctx, refs)
    dp = torch.from_numpy(parts).cuda()
    refno, psi, flip = pm.match(dp, parity=1)
    st = pm.last_stats()
    o = oracle.PM(h_refs)
    er, ep, ef, _ = o.match(parts, parity=1)
    assert np.array_equal(refno.cpu().numpy(), er[:, 0])
    assert np.array_equal(psi.cpu().numpy(), ep[:, 0])
    assert np.array_equal(flip.cpu().numpy(), ef[:, 0])
    assert st["pruned_rows"] > 0          # the product configuration: rows were skipped and nothing changed
    sx, sy, cc = pm.translate(dp, refno, psi, flip, 10.0)
    ex, ey, ec = o.translate(parts, er[:, 0], ep[:, 0], ef[:, 0], 10.0)
    assert np.abs(sx.cpu().numpy() - ex).max() <= 1e-3 and np.abs(sy.cpu().numpy() - ey).max() <= 1e-3
    assert np.abs(cc.cpu().numpy() - ec).max() <= 1e-5
    print("rescored", st["rescored_particles"], "of", n, "pruned", st["pruned_rows"] / st["rows"], "S6 repeats", pm.translate_repeated())


def test_exact_indices_at_scale_against_a_fifty_times_wider_margin(gpu):
    """The arg-max is exact as long as no fp32 value is off by tau / 2, and tau is a multiple of a MEASURED error.  A
    check at a scale the oracle cannot reach: 8192 particles of the bench's kind (256 px, 1000 phantom references, SNR 0.1) matched
    with the product margin (tau_rel 2e-6: 13 % re-scored in fp64) and again with a margin fifty times wider (1e-4: every particle
    re-scored, every row within 1e-4 S of its best re-evaluated in double) give the same reference, in-plane index and mirror for
    every particle -- i.e. none of the 8192 decisions the product left to fp32 would have been different in double."""
    xa, ctx, torch = gpu
    D, nrefs, n = 256, 1000, 4096
    vol = torch.from_numpy(synth.phantom(D, seed=4, nblobs=20).astype(np.float32)).cuda()
    fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
    refs = fp.project(np.concatenate([synth.fibonacci_directions(nrefs), np.zeros((nrefs, 1))], 1))
    fp.close()
    refs = ((refs - refs.mean()) / refs.std()).contiguous()
    g = torch.Generator(device="cuda").manual_seed(77)
    pm = xa.ProjectionMatcher(ctx, refs)
    tau = pm.get_option("tau_rel")
    for batch in range(2):
        idx = torch.randint(0, nrefs, (n,), generator=g, device="cuda")
        th = torch.rand((n,), generator=g, device="cuda") * (2 * np.pi)
        rot = torch.zeros((n, 2, 3), device="cuda")
        rot[:, 0, 0] = torch.cos(th); rot[:, 0, 1] = -torch.sin(th); rot[:, 1, 0] = torch.sin(th); rot[:, 1, 1] = torch.cos(th)
        parts = torch.empty((n, D, D), device="cuda")
        for b0 in range(0, n, 512):
            sl = slice(b0, b0 + 512)
            grid = torch.nn.functional.affine_grid(rot[sl], (512, 1, D, D), align_corners=False)
            parts[sl] = torch.nn.functional.grid_sample(refs[idx[sl]][:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0]
        parts = (parts + np.sqrt(10.0) * torch.randn((n, D, D), generator=g, device="cuda")).contiguous()
        pm.set_option("tau_rel", tau)
        r1, p1, f1 = (t.clone() for t in pm.match(parts, parity=batch))
        few = pm.last_stats()["rescored_particles"]
        pm.set_option("tau_rel", 1e-4)
        r2, p2, f2 = pm.match(parts, parity=batch)
        many = pm.last_stats()["rescored_particles"]
        print("batch", batch, "re-scored", few, "->", many, "of", n)
        assert many >= 0.99 * n > few
        assert torch.equal(r1, r2) and torch.equal(p1, p2) and torch.equal(f1, f2)
    pm.set_option("tau_rel", tau)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_translation_fp32_map_error_against_the_margin(gpu, D):
    """The coarse pass of xh_pm_translate flags a particle when a discrete decision of bestShift comes within s6_eps |max| of
    flipping; that only protects the decisions if the fp32 correlation map itself is much closer than that to the double
    one: max |R32 - R64| <= s6_eps / 4 of the map's maximum, measured on the maps the two chains leave behind."""
    xa, ctx, torch = gpu
    nrefs, n = 8, 96
    refs = _library(D, nrefs, seed=6)
    rng = np.random.default_rng(D + 1)
    parts, truth = synth.make_particles(refs, n, rng, snr=0.1, max_shift=3)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    dp = torch.from_numpy(parts).cuda()
    refno, psi, flip = pm.match(dp)
    pm.set_option("s6_capture", 64)
    pm.translate(dp, refno, psi, flip)
    r64 = pm.debug_s6_maps(n)
    pm.set_option("s6_capture", 32)
    pm.translate(dp, refno, psi, flip)
    r32 = pm.debug_s6_maps(n)
    pm.set_option("s6_capture", 0)
    peak = np.abs(r64).reshape(n, -1).max(1)
    err = np.abs(r32 - r64).reshape(n, -1).max(1) / peak
    eps = pm.get_option("s6_eps")
    print("D", D, "max |R32 - R64| / |max|:", err.max(), "s6_eps", eps)
    assert peak.min() > 0 and err.max() <= eps / 4


def test_translation_fp32_map_error_on_the_bench_kind_of_data(gpu):
    """The same measurement where the product runs: 256 px, a gallery of 1000 projections of the phantom, particles at SNR 0.1 matched by
    the library itself.  s6_eps is twenty times what is measured here (and at least four times, as the test above asks)."""
    xa, ctx, torch = gpu
    D, nrefs, n = 256, 1000, 384
    g = torch.Generator(device="cuda").manual_seed(5)
    vol = torch.from_numpy(synth.phantom(D, seed=4, nblobs=20).astype(np.float32)).cuda()
    fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
    refs = fp.project(np.concatenate([synth.fibonacci_directions(nrefs), np.zeros((nrefs, 1))], 1))
    fp.close()
    refs = ((refs - refs.mean()) / refs.std()).contiguous()
    idx = torch.randint(0, nrefs, (n,), generator=g, device="cuda")
    parts = (torch.roll(refs[idx], shifts=(2, -3), dims=(1, 2)) + np.sqrt(10.0) * torch.randn((n, D, D), generator=g, device="cuda")).contiguous()
    pm = xa.ProjectionMatcher(ctx, refs)
    refno, psi, flip = pm.match(parts)
    pm.set_option("s6_capture", 64)
    pm.translate(parts, refno, psi, flip)
    r64 = pm.debug_s6_maps(n)
    pm.set_option("s6_capture", 32)
    pm.translate(parts, refno, psi, flip)
    r32 = pm.debug_s6_maps(n)
    pm.set_option("s6_capture", 0)
    peak = np.abs(r64).reshape(n, -1).max(1)
    err = np.abs(r32 - r64).reshape(n, -1).max(1) / peak
    eps = pm.get_option("s6_eps")
    print("max |R32 - R64| / |max| over", n, "particles:", err.max(), "median", np.median(err), "s6_eps", eps)
    assert peak.min() > 0 and err.max() <= eps / 8


def test_translation_fp32_first_against_the_oracle_at_full_size(gpu, oracle):
    """xh_pm_translate in its default state (fp32 pass, flagged particles repeated in double) against the ORACLE at 256 px on
    301 particles: shifts 1e-3 px, maxCC 1e-5; with --max_shift small enough that the rejection branch (APM:841-842) is taken
    for some of them."""
    xa, ctx, torch = gpu
    D, nrefs, n = 256, 12, 301
    refs = _library(D, nrefs, seed=4)
    rng = np.random.default_rng(D)
    parts, truth = synth.make_particles(refs, n, rng, snr=0.1, max_shift=3)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    o = oracle.PM(refs)
    dp = torch.from_numpy(parts).cuda()
    refno, psi, flip = pm.match(dp)
    for max_shift in (10.0, 2.5):
        sx, sy, cc = [t.cpu().numpy() for t in pm.translate(dp, refno, psi, flip, max_shift)]
        ex, ey, ec = o.translate(parts, refno.cpu().numpy(), psi.cpu().numpy(), flip.cpu().numpy(), max_shift)
        assert np.abs(sx - ex).max() <= 1e-3 and np.abs(sy - ey).max() <= 1e-3
        assert np.abs(cc - ec).max() <= 1e-5
        rejected = int(((ex == 0) & (ey == 0)).sum())
        print("max_shift", max_shift, "repeated", pm.translate_repeated(), "of", n, "; zero shifts", rejected)
    assert rejected > 0


def test_constant_particle_in_a_masked_list_search_stays_on_its_list(gpu):
    """A particle without variance has NaN bounds and a NaN pruning threshold; in the masked bank search (ascending neighbour
    lists) the references that are not on its list must still be excluded: the reference returned is on the list, as in the
    gather path."""
    xa, ctx, torch = gpu
    D, nrefs, n = 64, 40, 6
    refs = _library(D, nrefs, seed=9)
    rng = np.random.default_rng(3)
    parts = rng.standard_normal((n, D, D)).astype(np.float32)
    parts[2] = 1.0                                     # constant: sigma = 0
    lists = [np.sort(rng.choice(np.arange(5, nrefs), 7, replace=False)).astype(np.int32) for _ in range(n)]
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    ids = np.concatenate(lists).astype(np.int32)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    refno, psi, flip = pm.match(torch.from_numpy(parts).cuda(), off, ids)
    r = refno.cpu().numpy()
    for i in range(n):
        assert r[i] in lists[i], (i, r[i], lists[i])


# options of experiments that were measured and retired (docs/experiments.md): the matcher no longer knows them
RETIRED_PM_OPTIONS = ["use_mfma", "use_mfma64", "use_idft3", "contract_shape", "contract_dbg", "store_cut", "s6_pair",
                      "s6_coarse_kernel", "s6_debug", "early_exit", "tail_band", "mirror", "polar_cells", "use_fir", "use_fir64",
                      "fir64_fused", "tie_rel"]


def test_retired_options_are_rejected(gpu):
    xa, ctx, torch = gpu
    from xmipp3_amd._lib import lib
    refs = _library(32, 12)
    pm = xa.ProjectionMatcher(ctx, torch.from_numpy(refs).cuda())
    for name in RETIRED_PM_OPTIONS:
        assert lib().xh_pm_set_option(pm.h, name.encode(), 1.0) == -1, name      # XH_ERR_ARG
    assert lib().xh_pm_set_option(pm.h, b"tau_rel", pm.get_option("tau_rel")) == 0
