"""xmipp_subtract_projection on the device (xh_sub) and its real-space ray projector (xh_rsp), at D = 128 and 256 (--sizes).

pipeline: the default path (Fourier projector, ROI mask, the 2-D disc) on --particles noisy projections of tests/synth.py's phantom, every
  other row with a CTF. particles_per_s: one untimed run to warm up, then --reps runs, wall clock around each, at capacity 1 (the
  reference's shape: one particle per step) and at --capacity. ms_per_stage: one more run with the library's event timing on, per
  particle. Next to every stage its bound, computed here from the shapes (px = D^2, Np = 2 (D - 1) + 1, c = 16 B):
    projection      bytes: the half-spectrum slice written and read (2 c px / 2), two line passes (2 x 2 c px), P written and the translation's
                    read and write (3 x 8 px); flop: 64 taps x 2 cubes x 2 per cell of the half spectrum, plus 10 per pixel.
    ctf             bytes: Np^2 x (pad 8 + c, 4 line passes x 2 c, multiply 2 c, crop c) + 8 px; flop: about 120 per cell of Np^2 (the CTF value).
    masks           the ROI's support projection: 4 rays x about 1.5 D steps per pixel, a bit per step; no byte bound worth the name.
                    flop: 10 per step.
    prepare_spectra bytes: px x (5 x 8 read, 2 x 8 + 4 c written) + 4 transforms x 4 passes x 2 c px.
    sums_fit        bytes: 2 c per fitted cell (about px / 2); models: 3 c per half-spectrum cell; output: px x (3 c + 2 c x 4 passes / 1 + 8 + 8 + c).
  bound_ms = max(bytes / 6.29 TB/s measured HBM copy rate, flop / 78.6 TFLOP/s fp64 vector peak). A chunk at these sizes fits the
  Infinity Cache, so the byte bound is an HBM figure the caches can beat; at capacity 1 every stage is launch-bound, which is the point.
rays: value mode against support mode on one binary mask: the measurement that justifies or retires support mode. steps: the voxel steps
  the rays walk (xh_rsp_steps), the full walk in value mode, up to the first hit on bits. ms: the library's event timer around one
  project() of --images orientations, best of --reps after a warm-up. A step reads 8 B (value) or one bit of a D^3 / 8 B table (support)
  and does about 10 fp64 operations; bound_steps_per_s = min(6.29 TB/s / 8 B, 78.6 TFLOP/s / 10) is printed for scale only: the walk is
  a dependent chain of loads and compares per lane.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 6.29e12
FP64_FLOPS = 78.6e12


def stage_bounds(D, fitted, steps_per_particle):
    px, c = float(D * D), 16.0
    Np = 2 * (D - 1) + 1
    half = D * (D // 2 + 1.0)
    byts = {"projection": c * half * 2 + 4 * c * half + 24 * px, "ctf": Np * Np * (8 + c + 8 * c + 2 * c + c) + 8 * px, "masks": steps_per_particle / 8.0,
            "prepare_spectra": px * (40 + 16 + 4 * c) + 4 * 4 * 2 * c * px, "sums_fit": 2 * c * fitted, "models": 3 * c * half,
            "output": px * (3 * c + 8 * c + 16 + c)}
    flop = {"projection": 256.0 * half + 10 * px, "ctf": 120.0 * Np * Np, "masks": 10.0 * steps_per_particle, "prepare_spectra": 10 * px, "sums_fit": 12.0 * fitted,
            "models": 20 * half, "output": 6 * px}
    return byts, flop


def pipeline(xa, ctx, D, n, capacity, reps):
    from tests import subtract_projection_ref as ref
    from tests import synth
    rng = np.random.default_rng(1)
    vol = (50.0 * synth.phantom(D, seed=11, nblobs=9)).astype(np.float32).astype(np.float64)
    roi = ref.blob_mask(D)
    ang = np.array(ref.generic_angles(n))
    import torch
    proj = xa.FourierProjector(ctx, torch.from_numpy(vol.astype(np.float32)).cuda(), 2.0, 0.5).project(ang).cpu().numpy()
    imgs = (1.3 * proj + 0.1 * proj.std() * rng.standard_normal(proj.shape)).astype(np.float32)
    from xmipp3_amd.api import ctf_params
    ctf = dict(kV=300.0, Cs=2.7, Ca=0.02, espr=1.0, Q0=0.07, DeltafU=15000.0, DeltafV=15400.0, azimuthal_angle=35.0, alpha=1e-4, DeltaF=20.0, DeltaR=0.3)
    rows = [dict(rot=a[0], tilt=a[1], psi=a[2], shift_x=float(rng.uniform(-2, 2)), shift_y=float(rng.uniform(-2, 2)),
                 ctf=ctf_params(**ctf) if k % 2 == 0 else None) for k, a in enumerate(ang)]
    rp = xa.RealSpaceProjector(ctx, torch.from_numpy(roi).cuda(), "support")
    steps = float(rp.steps(ang).sum(dtype=torch.int64).item()) / n
    rp.close()
    out = {"size": D, "particles": n, "roi_support_steps_per_particle": steps}
    first = None
    for cap in (1, capacity):
        h = xa.SubtractProjection(ctx, vol, roi, None, capacity=cap)
        h.load(imgs, rows)
        got, _ = h.run()                                    # warm-up
        first = got if first is None else first
        same = bool(got.tobytes() == first.tobytes())       # a particle does not depend on the capacity
        secs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            h.run()
            secs.append(time.perf_counter() - t0)
        h.set_timing(True)
        h.run()
        stage = {k: v / n for k, v in h.stage_ms().items()}
        fitted = float(((xa.sub_freq_map(D)[0] > 0) & (xa.sub_freq_map(D)[0] < h.maxwi)).sum())
        h.close()
        byts, flop = stage_bounds(D, fitted, steps)
        stages = {}
        for k in stage:
            bound = max(byts[k] / HBM_BPS, flop[k] / FP64_FLOPS) * 1e3
            stages[k] = {"ms": round(stage[k], 5), "bytes": int(byts[k]), "flop": int(flop[k]), "bound_ms": round(bound, 6),
                         "bound_by": "bytes" if byts[k] / HBM_BPS > flop[k] / FP64_FLOPS else "flop", "time_over_bound": round(stage[k] / bound, 1)}
        out[f"capacity_{cap}"] = {"capacity": cap, "seconds_per_run": [round(s, 5) for s in secs], "particles_per_s": round(n / min(secs), 1),
                                  "ms_per_particle_by_events": round(sum(stage.values()), 5), "stages": stages, "same_bits_as_capacity_1": same}
    out["speedup_over_capacity_1"] = round(out[f"capacity_{capacity}"]["particles_per_s"] / out["capacity_1"]["particles_per_s"], 2)
    return out


def rays(xa, ctx, D, images, reps):
    import torch
    from tests import subtract_projection_ref as ref
    rng = np.random.default_rng(0)
    ang = np.array(ref.generic_angles(images))
    off = rng.uniform(-3, 3, (images, 2))
    mask = torch.from_numpy(ref.blob_mask(D)).cuda()
    modes, planes = {}, {}
    for mode in ("value", "support"):
        rp = xa.RealSpaceProjector(ctx, mask, mode)
        steps = int(rp.steps(ang, off).sum(dtype=torch.int64).item())
        planes[mode] = rp.project(ang, off)                 # warm-up
        ctx.sync()
        ms = []
        t = ctx.timer()
        for _ in range(reps):
            t.start()
            rp.project(ang, off)
            t.stop()
            ms.append(t.elapsed_ms())
        best = min(ms)
        modes[mode] = {"packed": rp.packed, "steps": steps, "ms": [round(m, 4) for m in ms], "ms_per_image": round(best / images, 5),
                       "steps_per_s": round(steps / (best * 1e-3), 1), "images_per_s": round(images / (best * 1e-3), 1)}
        rp.close()
    agree = float(((planes["value"] > 0) == (planes["support"] > 0)).double().mean().item())
    modes["value"]["bound_steps_per_s"] = min(HBM_BPS / 8.0, FP64_FLOPS / 10.0)
    return {"size": D, "images": images, "mask_voxels": int(mask.sum().item()), "volume_bytes": 8 * D ** 3, "bits_bytes": D ** 3 // 8,
            "value": modes["value"], "support": modes["support"],
            "support_over_value_images_per_s": round(modes["support"]["images_per_s"] / modes["value"]["images_per_s"], 3),
            "support_equals_value_positive_fraction": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    assert torch.cuda.is_available(), "this benchmark needs the device"
    ctx = xa.Context(0)
    out = {"bench": "subtract_projection", "reps": a.reps, "pipeline": [pipeline(xa, ctx, D, a.particles, a.capacity, a.reps) for D in a.sizes],
           "rays": [rays(xa, ctx, D, a.images, a.reps) for D in a.sizes]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
