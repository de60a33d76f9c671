"""Throughput of xmipp_angular_sph_alignment's device step (xh_asa_cost) and lockstep search (xh_asa_refine) against the batch capacity,
at --size (default 128), degrees (3, 2), on a synthetic volume (tests/synth.py's phantom). The particles are the device's own projections
of the volume at random orientations (one evaluation at zero variables, read back through last()), with noise; their input poses are
perturbed inside the default bounds (angles by up to 2 degrees, shifts by up to 1 px).

step:   one xh_asa_cost call of `capacity` rows with full-degree coefficients: upload, projection, two 2-D transforms with the filter
        between them, cost, readback, one stream wait. evaluations_per_s = capacity / step time; capacity 1 is one evaluation per device
        step, the shape of the reference's CUDA program, and is the baseline: speedup_vs_capacity_1 is the result.
search: one warm-up refine on a subset, then one timed refine with --optimizeDeformation --optimizeAlignment: particles_per_s.

Next to ms_per_eval, the evaluation's own bound, computed here from the shapes:
  bytes: over the ball r < RDef every voxel's eight taps of the volume (neighbouring voxels share them: the volume's own voxels once, 8 B)
         and its mask voxel (4 B); the plane: written once (8 B), converted (8 + 16 B), four line-transform passes and the filter
         (5 x 32 B), the cost kernel's read and the two planes it writes (16 + 16 B), and the particle (8 B) per pixel.
  flop:  per voxel of the ball the rotation (15), the basis and the trilinear sample (ops_per_voxel of bench_volume_deform_sph.py, one
         pair), the mask lookup's conversions not counted.
bound_ms = max(bytes / 6.29 TB/s measured HBM copy rate, flop / 78.6 TFLOP/s fp64 vector peak). Everything here fits the Infinity Cache,
so the byte bound is an HBM figure the caches can beat.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DEFAULT_CAPACITY = 64          # the program's (host/angular_sph_alignment.h) and the Python class's default


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--capacities", type=int, nargs="+", default=[1, DEFAULT_CAPACITY, 256])
    ap.add_argument("--reps", type=int, default=20, help="timed steps per capacity")
    ap.add_argument("--search-particles", type=int, default=8, help="particles of the timed refine (0: no search)")
    ap.add_argument("--search-capacities", type=int, nargs="+", default=[1, DEFAULT_CAPACITY])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from bench_volume_deform_sph import FP64_FLOPS, HBM_BPS, ops_per_voxel
    from tests import synth
    assert torch.cuda.is_available(), "this benchmark needs the device"
    D, L1, L2 = a.size, 3, 2
    ctx = xa.Context(0)
    vol = torch.from_numpy(synth.phantom(D, seed=11, nblobs=9).astype(np.float32)).cuda()
    rng = np.random.default_rng(0)
    npart = max(max(a.capacities), a.search_particles, 1)
    ang = synth.random_angles(npart, rng)
    # the particles: the device's own projections at the true poses
    gen = xa.AngularSphAlignment(ctx, vol, capacity=min(npart, 64), l1=L1, l2=L2)
    imgs = np.zeros((npart, D, D), np.float32)
    gen.load(imgs, [dict(rot=q[0], tilt=q[1], psi=q[2]) for q in ang])
    for i0 in range(0, npart, gen.capacity):
        m = min(gen.capacity, npart - i0)
        gen.cost(np.arange(i0, i0 + m), np.zeros((m, gen.nvars)))
        for r in range(m):
            imgs[i0 + r] = gen.last(r)[1].cpu().numpy()
    nvars, vec, RDef = gen.nvars, gen.vecSize, gen.RDef
    gen.close()
    imgs += 0.1 * imgs.std() * rng.standard_normal(imgs.shape).astype(np.float32)
    rows = [dict(rot=ang[i, 0] + rng.uniform(-2, 2), tilt=ang[i, 1] + rng.uniform(-2, 2), psi=ang[i, 2] + rng.uniform(-2, 2),
                 shift_x=rng.uniform(-1, 1), shift_y=rng.uniform(-1, 1)) for i in range(npart)]
    ball = 4.0 / 3.0 * math.pi * RDef ** 3
    byts = 12.0 * ball + (8 + 24 + 5 * 32 + 32 + 8) * D * D
    flop = (ops_per_voxel(L1, L2, 1) + 15) * ball
    bound = max(byts / HBM_BPS, flop / FP64_FLOPS) * 1e3
    steps, base = [], None
    for cap in a.capacities:
        h = xa.AngularSphAlignment(ctx, vol, capacity=cap, l1=L1, l2=L2)
        h.load(imgs[:cap], rows[:cap])
        X = np.zeros((cap, nvars))
        X[:, :3 * vec] = 0.05 * rng.standard_normal((cap, 3 * vec))
        X[:, 3 * vec:3 * vec + 5] = rng.uniform(-1, 1, (cap, 5))
        idx = np.arange(cap)
        for _ in range(3):
            h.cost(idx, X)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            h.cost(idx, X)                              # synchronous: each call ends in a stream synchronise
        ms = (time.perf_counter() - t0) * 1e3 / a.reps
        h.close()
        row = {"capacity": cap, "ms_per_step": round(ms, 4), "ms_per_eval": round(ms / cap, 5), "evaluations_per_s": round(cap / ms * 1e3, 1),
               "time_over_bound": round(ms / cap / bound, 1)}
        if cap == 1:
            base = cap / ms
        if base:
            row["speedup_vs_capacity_1"] = round((cap / ms) / base, 2)
        steps.append(row)
    search, sbase = [], None
    for cap in a.search_capacities if a.search_particles > 0 else []:
        n = a.search_particles
        h = xa.AngularSphAlignment(ctx, vol, capacity=cap, l1=L1, l2=L2, optimize_deformation=1, optimize_alignment=1)
        h.load(imgs[:1], rows[:1])
        h.refine()                                       # warm-up
        h.load(imgs[:n], rows[:n])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X, cost, en, de, it, ev = h.refine()
        secs = time.perf_counter() - t0
        st = h.stats()
        h.close()
        row = {"capacity": cap, "particles": n, "seconds": round(secs, 3), "particles_per_s": round(n / secs, 3), "evaluations": int(ev.sum()),
               "evaluations_per_s": round(int(ev.sum()) / secs, 1), "device_steps": st["steps"], "host_share": round(1.0 - st["device_s"] / st["total_s"], 4),
               "enabled": int((en == 1).sum()), "mean_cost": round(float(cost.mean()), 6)}
        if cap == 1:
            sbase = n / secs
        if sbase:
            row["speedup_vs_capacity_1"] = round((n / secs) / sbase, 2)
        search.append(row)
    out = {"bench": "angular_sph_alignment", "size": D, "degrees": [L1, L2], "reps": a.reps, "default_capacity": DEFAULT_CAPACITY,
           "bytes_per_eval": int(byts), "flop_per_eval": int(flop), "bound_ms": round(bound, 5), "bound_by": "bytes" if byts / HBM_BPS > flop / FP64_FLOPS else "flop",
           "step": steps, "search": search}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
