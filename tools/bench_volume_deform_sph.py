"""Timing of xmipp_volume_deform_sph's cost evaluation (xh_vds_cost) and search on synthetic volumes (a few Gaussian blobs plus low
noise, seeded), degrees L1 = 3, L2 = 2: ms per evaluation at 128^3 and 256^3 with 1 and 3 pairs, at full-degree coefficients (the
(3, 2) kernel) and at stage-0 coefficients (the (3, 0) kernel a stage-0 search runs), and the evaluations and seconds of a full
staged search at 128^3 with 1 pair.

Next to every time, the evaluation's own bound, computed here from the shapes:
  bytes: over the box of the ball, every pair reads its reference voxel once (8 B) and the eight taps of its input volume; neighbouring
         voxels share taps, so the taps that miss are the input volume's own voxels once (8 B): 16 B per box voxel per pair.
  flop:  per voxel of the ball, the basis (the 2 h + 1 harmonics of every degree, the radial polynomials, 6 flop per term for the three
         coefficient FMAs plus 1 for R * S) and per pair the trilinear sample (7 lerps of 3 flop, 3 flop for the sums); counted by
         ops_per_voxel below.
bound_ms = max(bytes / 6.29 TB/s measured HBM copy rate, flop / 78.6 TFLOP/s fp64 vector peak); at these sizes (128^3 x 3 pairs is
100 MB, inside the 256 MiB Infinity Cache) the byte bound is an HBM figure the caches can beat. A time far above both bounds is
launch and readback latency: one evaluation is two launches, one 24-byte copy and one synchronise.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 6.29e12
FP64_FLOPS = 78.6e12


def ops_per_voxel(L1, L2, npairs):
    harm = {0: 0, 1: 3, 2: 14, 3: 34, 4: 62}          # multiplies and adds of the written-out harmonics of one degree
    radial = {(0, 0): 0, (1, 1): 1, (2, 0): 3, (2, 2): 1, (3, 1): 4, (3, 3): 2, (4, 0): 6, (4, 2): 4, (4, 4): 2, (5, 1): 7, (5, 3): 5, (5, 5): 3}
    flop = 12                                          # scaled coordinates, squares, r
    for h in range(L2 + 1):
        flop += harm[h]
        for l in range(h, L1 + 1, 2):
            flop += radial[(l, h)] + (2 * h + 1) * 7
    return flop + npairs * 24 + 6


def blobs(shape, seed, nblobs=8):
    """a smooth seeded volume: a few Gaussian blobs"""
    rng = np.random.default_rng(seed)
    k, i, j = np.meshgrid(*(np.arange(n) - n // 2 for n in shape), indexing="ij")
    v = np.zeros(shape)
    for _ in range(nblobs):
        c = rng.uniform(-0.25, 0.25, 3) * np.array(shape)
        s = rng.uniform(0.02, 0.05) * shape[0]
        v += rng.uniform(0.5, 1.0) * np.exp(-((k - c[0]) ** 2 + (i - c[1]) ** 2 + (j - c[2]) ** 2) / (2 * s * s))
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--search-size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "this benchmark needs the device"
    ctx = xa.Context(0)
    L1, L2 = 3, 2
    nt = xa.vds_num_terms(L1, L2)
    rng = np.random.default_rng(0)
    rows = []
    for n in a.sizes:
        shape = (n, n, n)
        VR = blobs(shape, seed=1)
        VI = np.roll(VR, 1, axis=2) + 0.02 * rng.standard_normal(shape)
        h = xa.VolumeDeformSph(ctx, shape, L1, L2)
        I = [xa.vds_normalize_robust(VI)] + [xa.vds_normalize_robust(h.gauss(VI, s)) for s in (1.0, 2.0)]
        R = [xa.vds_normalize_robust(VR)] + [xa.vds_normalize_robust(h.gauss(VR, s)) for s in (1.0, 2.0)]
        box = (2 * (math.ceil(h.Rmax) - 1) + 1) ** 3
        ball = 4.0 / 3.0 * math.pi * h.Rmax ** 3
        for npairs in (1, 3):
            h.set_pairs(np.array(I[:npairs]), np.array(R[:npairs]))
            full = 0.05 * rng.standard_normal(3 * nt)
            stage0 = np.zeros(3 * nt)
            stage0.reshape(3, nt)[:, :2] = 0.3
            for name, x, l2 in (("full", full, L2), ("stage0", stage0, 0)):
                for _ in range(10):
                    h.cost(x)
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    h.cost(x)                          # synchronous: each call ends in a stream synchronise
                ms = (time.perf_counter() - t0) * 1e3 / a.reps
                byts = 16.0 * box * npairs
                flop = ops_per_voxel(L1, l2, npairs) * ball
                bound = max(byts / HBM_BPS, flop / FP64_FLOPS) * 1e3
                rows.append({"size": n, "pairs": npairs, "coefficients": name, "ms_per_eval": round(ms, 4), "bytes": int(byts), "flop": int(flop),
                             "flop_per_voxel": ops_per_voxel(L1, l2, npairs), "bound_ms": round(bound, 5), "bound_by": "bytes" if byts / HBM_BPS > flop / FP64_FLOPS else "flop",
                             "time_over_bound": round(ms / bound, 1)})
        if n == a.search_size:
            h.set_pairs(np.array(I[:1]), np.array(R[:1]))
            h.refine_stage(0, np.zeros(3 * nt))            # warm-up
            t0 = time.perf_counter()
            x, cost, evals = h.refine()
            secs = time.perf_counter() - t0
            search = {"size": n, "pairs": 1, "evaluations": int(evals), "seconds": round(secs, 3), "cost_at_0": float(h.cost(np.zeros(3 * nt))[0]), "cost": float(cost),
                      "ms_per_eval": round(secs * 1e3 / max(1, evals), 4)}
    out = {"bench": "volume_deform_sph", "degrees": [L1, L2], "reps": a.reps, "cost": rows, "search": search if a.search_size in a.sizes else None}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
