"""Throughput of xmipp_forward_art_zernike3d's sweep (xh_faz_sweep) at --size (default 128), one sigma, with degrees (3, 2) and without
deformation, on a synthetic volume (tests/synth.py's phantom). The particles are noisy filtered projections the device itself makes
(forward() against the phantom); the sweep then starts from a zero volume, as the program does without --ref.

images_per_s: one untimed sweep to warm up, then --reps sweeps of --images images, wall clock around each (a sweep ends in its one stream
wait). ms_per_stage: the same sweep with the library's event timing on, per image.

Next to every stage its own bound, computed here from the shapes (ball = the voxels with r <= RDef, N = D^3, px = D^2):
  splat       bytes: V (8 B) and maskF (4 B) per voxel of the listed bricks, the planes cleared and the tile entries added (16 B each);
              flop: the basis (ops_per_voxel of bench_volume_deform_sph.py, no sample), rotation and weights (30) per voxel of the ball.
              atomic bytes: 16 B per non-zero tile entry, counted exactly here from the first image's own positions (numpy).
  filter      bytes: 2 planes x px x (24 conversion + 4 line passes x 32 + 32 multiply).
  residual    bytes: px x (2 x 16 planes + 8 particle + 16 written).
  regulariser bytes: N x 4 (maskB) twice, ball x (8 + 32) for computeTV, ball x (32 + 8) for computeDTV.
  backward    bytes: N x 4 + ball x (16 V + 8 Reg); flop: as the splat's per voxel of the ball, plus 2 x 10 for the two bilinear reads.
bound_ms = max(bytes / 6.29 TB/s measured HBM copy rate, flop / 78.6 TFLOP/s fp64 vector peak). At D = 128 the six volumes (100 MB) fit
the Infinity Cache, so the byte bound is an HBM figure the caches can beat.
splat_atomic_bytes_per_s is set against 1.3 TB/s, the chip-wide rate of global float atomic adds. That figure was measured for f32
adds of 256 contiguous bytes; the rate of f64 adds is not known, and a tile row here is 48 doubles at most.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ATOMIC_BPS_F32 = 1.3e12


def tile_entries(D, RDef, R, coef, terms):
    """the non-zero (brick, pixel) pairs of one image: what the splat adds to the global planes"""
    from tests.test_volume_deform_sph_host import zsh_ref
    c = D // 2
    k, i, j = np.meshgrid(*(np.arange(D) - c,) * 3, indexing="ij")
    r2 = (k * k + i * i + j * j).astype(np.float64)
    inside = r2 <= RDef * RDef
    k, i, j = k[inside].astype(np.float64), i[inside].astype(np.float64), j[inside].astype(np.float64)
    rr = np.sqrt(r2[inside]) / RDef
    g = np.zeros((3, k.size))
    if coef is not None:
        vec = len(terms)
        for idx, (l1, n, l2, m) in enumerate(terms):
            z = np.where((rr > 0) | (l2 == 0), zsh_ref(l1, n, l2, m, j / RDef, i / RDef, k / RDef, rr), 0.0)
            for d in range(3):
                g[d] += coef[d * vec + idx] * z
    rx, ry, rz = j + g[0], i + g[1], k + g[2]
    x, y = R[0, 0] * rx + R[0, 1] * ry + R[0, 2] * rz, R[1, 0] * rx + R[1, 1] * ry + R[1, 2] * rz
    px, py = np.sign(x) * np.floor(np.abs(x) + 0.5), np.sign(y) * np.floor(np.abs(y) + 0.5)
    ok = (px >= -c) & (px <= D - 1 - c) & (py >= -c) & (py <= D - 1 - c)
    nb = (D + 15) // 16
    brick = (((k + c) // 16) * nb + (i + c) // 16) * nb + (j + c) // 16
    key = (brick[ok].astype(np.int64) * D + (py[ok] + c).astype(np.int64)) * D + (px[ok] + c).astype(np.int64)
    return int(np.unique(key).size), int(inside.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from bench_volume_deform_sph import FP64_FLOPS, HBM_BPS, ops_per_voxel
    from oracle import pyoracle
    from tests import synth
    from tests.test_volume_deform_sph_host import terms_ref
    assert torch.cuda.is_available(), "this benchmark needs the device"
    D, L1, L2, n = a.size, 3, 2, a.images
    ctx = xa.Context(0)
    phantom = synth.phantom(D, seed=11, nblobs=9).astype(np.float64)
    rng = np.random.default_rng(0)
    ang = synth.random_angles(n, rng)
    rows = [dict(rot=q[0], tilt=q[1], psi=q[2], shift_x=rng.uniform(-1, 1), shift_y=rng.uniform(-1, 1)) for q in ang]
    terms = terms_ref(L1, L2)
    vec = len(terms)
    coefs = 0.3 * rng.standard_normal((n, 3 * vec))
    cases = []
    for name, use in (("zernike_3_2", 1), ("no_deformation", 0)):
        co = coefs if use else None
        # the particles: the device's filtered projections of the phantom, with noise
        gen = xa.ForwardArtZernike3D(ctx, D, volume=phantom, l1=L1, l2=L2, use_zernike=use)
        gen.load(np.zeros((n, D, D), np.float32), rows, co)
        imgs = np.array([gen.forward(q)["P"][0].cpu().numpy() for q in range(n)])
        RDef = gen.RDef
        gen.close()
        imgs = (imgs + 0.1 * imgs.std() * rng.standard_normal(imgs.shape)).astype(np.float32)
        h = xa.ForwardArtZernike3D(ctx, D, l1=L1, l2=L2, use_zernike=use)
        h.load(imgs, rows, co)
        h.sweep()                                           # warm-up
        secs = []
        for _ in range(a.reps):
            h.set_volume(np.zeros((D, D, D)))
            t0 = time.perf_counter()
            err = h.sweep()
            secs.append(time.perf_counter() - t0)
        best = min(secs)
        h.set_timing(True)
        h.set_volume(np.zeros((D, D, D)))
        h.sweep()
        stage = {k: v / n for k, v in h.stage_ms().items()}
        nbricks = h.nbricks
        h.close()
        entries, ball = tile_entries(D, RDef, pyoracle.euler_matrix(*ang[0]), co[0] if use else None, terms)
        N, px = D ** 3, D * D
        basis = ops_per_voxel(L1, L2, 0) if use else 0
        byts = {"splat": 12.0 * nbricks * 4096 + 16.0 * px + 16.0 * entries, "filter": 2.0 * px * (24 + 4 * 32 + 32), "residual": px * (32 + 8 + 16.0),
                "regulariser": 8.0 * N + 80.0 * ball, "backward": 4.0 * N + 24.0 * ball}
        flop = {"splat": (basis + 30.0) * ball, "filter": 0.0, "residual": 0.0, "regulariser": 40.0 * ball, "backward": (basis + 50.0) * ball}
        stages = {}
        for k in stage:
            bound = max(byts[k] / HBM_BPS, flop[k] / FP64_FLOPS) * 1e3
            stages[k] = {"ms": round(stage[k], 5), "bytes": int(byts[k]), "flop": int(flop[k]), "bound_ms": round(bound, 5),
                         "bound_by": "bytes" if byts[k] / HBM_BPS > flop[k] / FP64_FLOPS else "flop", "time_over_bound": round(stage[k] / bound, 1)}
        atomic_bps = 16.0 * entries / (stage["splat"] * 1e-3)
        cases.append({"case": name, "images": n, "bricks": nbricks, "ball_voxels": ball, "seconds_per_sweep": [round(s, 5) for s in secs],
                      "images_per_s": round(n / best, 2), "ms_per_image": round(best / n * 1e3, 4), "ms_per_image_by_events": round(sum(stage.values()), 4),
                      "stages": stages, "splat_tile_entries": entries, "splat_atomic_bytes": int(16 * entries),
                      "splat_atomic_bytes_per_s": round(atomic_bps, 1), "splat_atomic_rate_over_f32_chip_rate": round(atomic_bps / ATOMIC_BPS_F32, 4),
                      "last_error": round(float(err[-1, 0]), 6)})
    out = {"bench": "forward_art_zernike3d", "size": D, "degrees": [L1, L2], "sigma": [2.0], "reps": a.reps, "f32_chip_atomic_bytes_per_s": ATOMIC_BPS_F32,
           "cases": cases}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
