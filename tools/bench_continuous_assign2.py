"""Throughput of the continuous assignment's lockstep search (xh_ca2_refine) against the batch capacity: synthetic particles from
tests/synth.py's phantom at --size (projections at random orientations with noise), input poses perturbed inside the default bounds
(angles by up to 2 degrees, shifts by up to 1 px), searched with --optimizeShift --optimizeAngles ("pose") and the same plus
--optimizeDefocus ("pose+defocus", every particle with a CTF). Capacity 1 is one evaluation per device step, the shape of the reference's
CUDA program, and is the baseline; speedup_vs_capacity_1 is the result.
Per (search, capacity): one warm-up refine on a subset (code objects, scratch), then --repeats timed refines; the median and the
min..max spread are reported. host_share is the part of a refine's wall time spent outside device steps (the coroutines, the rows'
matrices, the scheduler), i.e. the time the device waits for the host. Prints one JSON line per (search, capacity)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--capacities", type=int, nargs="+", default=[1, 64, 1024, 4096])
    ap.add_argument("--particles", type=int, default=0, help="particles per refine (default: max(capacity, 256), 16 at capacity 1)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--searches", nargs="+", default=["pose", "pose+defocus"])
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from xmipp3_amd.api import ctf_params
    from tests import synth
    D = a.size
    ctx = xa.Context(0)
    vol = torch.from_numpy(synth.phantom(D, seed=11, nblobs=9).astype(np.float32)).cuda()
    nmax = a.particles or max(max(a.capacities), 256)
    rng = np.random.default_rng(0)
    ang = synth.random_angles(nmax, rng)
    fp = xa.FourierProjector(ctx, vol, 2.0, 0.5, 3)
    imgs = fp.project(ang).cpu().numpy()
    fp.close()
    imgs += 0.1 * imgs.std() * rng.standard_normal(imgs.shape).astype(np.float32)
    ctf = ctf_params(kV=300.0, Cs=2.7, Q0=0.07, DeltafU=15000.0, DeltafV=15400.0, azimuthal_angle=35.0)
    rows = [dict(rot=ang[i, 0] + rng.uniform(-2, 2), tilt=ang[i, 1] + rng.uniform(-2, 2), psi=ang[i, 2] + rng.uniform(-2, 2),
                 shift_x=rng.uniform(-1, 1), shift_y=rng.uniform(-1, 1)) for i in range(nmax)]
    base = {}
    for search in a.searches:
        defocus = search == "pose+defocus"
        for cap in a.capacities:
            n = a.particles or (16 if cap == 1 else max(cap, 256))
            n = min(n, nmax)
            h = xa.ContinuousAssign2(ctx, vol, capacity=cap, optimize_shift=1, optimize_angles=1, optimize_defocus=int(defocus))
            r = [dict(q, ctf=ctf) for q in rows[:n]] if defocus else rows[:n]
            w = min(n, max(cap, 16))
            h.load(imgs[:w], r[:w])
            h.refine()                                   # warm-up
            h.load(imgs[:n], r[:n])
            secs, stats, evals = [], [], 0
            for _ in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                X, cost, it, ev, en = h.refine()
                secs.append(time.perf_counter() - t0)
                stats.append(h.stats())
                evals = int(ev.sum())
            h.close()
            med = float(np.median(secs))
            k = int(np.argsort(secs)[len(secs) // 2])
            out = {"bench": "continuous_assign2", "size": D, "search": search, "capacity": cap, "particles": n, "repeats": a.repeats,
                   "seconds_median": round(med, 4), "seconds_min": round(min(secs), 4), "seconds_max": round(max(secs), 4),
                   "particles_per_s": round(n / med, 2), "evaluations_per_s": round(evals / med, 1),
                   "evaluations_per_particle": round(evals / n, 1), "device_rows": stats[k]["rows"], "device_steps": stats[k]["steps"],
                   "host_share": round(1.0 - stats[k]["device_s"] / stats[k]["total_s"], 4), "enabled": int((en == 1).sum())}
            if cap == 1:
                base[search] = n / med
            if search in base:
                out["speedup_vs_capacity_1"] = round((n / med) / base[search], 2)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
