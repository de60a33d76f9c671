"""Measurements of xmipp_reconstruct_significant's device side (xh_rsig_*), written as one JSON document:
 - (image, direction) pairs/s of align at D = 64 and 128 against batch_chains, with the capacity of one pair (4 chains) as the baseline: the
   same pairs at every capacity, --repeats windows of at least --window seconds each, the median with the lowest and the highest;
 - seconds inside shift steps and inside rotation steps from events (a timed run), per chain-step, next to each step's HBM byte bound;
 - the share of chains still taking each step in rounds 2 and 3;
 - seconds of both weighting stages at N = 10^4 and 10^5 images with G = 10^3 directions.
Images are noisy rotated, shifted, possibly mirrored copies of the gallery's projections (tests/synth.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12          # achievable, not the 8 TB/s of the specification


def step_byte_bounds(D, ncoefs, nsamples, N, ln):
    """bytes every kernel of a step must move at least once, per chain (caches serve nothing, nothing is read twice)"""
    px = D * D
    shift = (8 + 16) * px                 # gather: image in, complex out
    shift += 2 * 2 * 32 * px              # two transforms of two line passes, each reading and writing the complex image
    shift += (16 + 16 + 16) * px          # correlate: projection spectrum and image spectrum in, product out
    shift += 16 * px                      # bestShift: the map once
    shift += (8 + 8) * px                 # the four candidates: projection and image once
    shift += (8 + 8) * px                 # applyGeometry: original in, current out
    rot = 8 * px + 8 * nsamples           # polar sampling
    rot += 3 * 8 * nsamples               # normalise: read, read, write
    rot += 8 * nsamples + 16 * ncoefs     # ring DFTs
    rot += 2 * 16 * ncoefs + 16 * N       # ring sum
    rot += 16 * N + 8 * ln + 8 * ln       # rotational correlation, first maximum
    rot += (8 + 8) * px                   # applyGeometry
    return shift, rot


def population(D, G, N, seed):
    from scipy import ndimage
    from tests import synth
    rng = np.random.default_rng(seed)
    base = synth.phantom(D, seed=1, nblobs=10)
    dirs = synth.fibonacci_directions(max(G, 2))[:G]
    few = np.stack([synth.project(base, r, t, 0.0) for r, t in dirs[:min(G, 4)]])
    gallery = np.stack([ndimage.rotate(few[g % len(few)], 360.0 * (g // len(few)) / max(1, G // len(few)), reshape=False, order=1) for g in range(G)])
    imgs = np.empty((N, D, D))
    for i in range(N):
        q = ndimage.rotate(gallery[int(rng.integers(G))], float(rng.uniform(0, 360)), reshape=False, order=1)
        if rng.integers(2):
            q = q[:, ::-1]
        q = ndimage.shift(q, rng.uniform(-5, 5, 2), order=1)
        imgs[i] = q + q.std() * rng.standard_normal(q.shape)
    return np.ascontiguousarray(gallery), imgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--gallery", type=int, default=64)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 256, 4096, 16384])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds every repeat is timed over, at least")
    ap.add_argument("--weight-images", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--weight-directions", type=int, default=1000)
    ap.add_argument("-o", default=os.path.join("profiles", "experiments", "reconstruct_significant_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    ctx = xa.Context(0)
    out = {"bench": "reconstruct_significant", "device": torch.cuda.get_device_name(0), "gallery": a.gallery, "images": a.images, "align": [], "weights": []}
    for D in a.sizes:
        gallery, imgs = population(D, a.gallery, a.images, 5)
        dg, di = torch.from_numpy(gallery).cuda(), torch.from_numpy(imgs).cuda()
        for batch in a.batches:
            n = a.images                                                    # every capacity aligns the same pairs
            h = xa.ReconstructSignificant(ctx, D, a.gallery, batch_chains=batch)
            h.load_gallery(dg)
            h.align(di[:1])                                                 # warm-up: code objects
            torch.cuda.synchronize()
            rates = []
            for _ in range(a.repeats):
                # a window of at least half a second: whole align calls until it is filled
                calls, t0 = 0, time.perf_counter()
                while True:
                    h.align(di[:n])
                    calls += 1
                    torch.cuda.synchronize()
                    t = time.perf_counter() - t0
                    if t >= a.window:
                        break
                rates.append(calls * n * a.gallery / t)
            s = h.stats()
            chains = 4 * n * a.gallery
            rec = {"size": D, "batch_chains": batch, "pairs": n * a.gallery, "repeats": a.repeats, "window_s": a.window, "pairs_per_s": round(float(np.median(rates)), 1),
                   "pairs_per_s_min": round(min(rates), 1), "pairs_per_s_max": round(max(rates), 1), "steps": int(s["steps"]),
                   "share_shift_round2": round(s["shift_round2"] / chains, 4), "share_shift_round3": round(s["shift_round3"] / chains, 4),
                   "share_rotation_round2": round(s["rotation_round2"] / chains, 4), "share_rotation_round3": round(s["rotation_round3"] / chains, 4)}
            if batch == max(a.batches):
                # a timed run: events around every step
                h.set_timing(True)
                h.align(di[:n])
                s = h.stats()
                nshift = s["shift_round1"] + s["shift_round2"] + s["shift_round3"]
                nrot = s["rotation_round1"] + s["rotation_round2"] + s["rotation_round3"]
                Ri, Ro = D // 5, D // 2
                nsam = [max(1, 2 * int(0.5 * 6.2831853071795864769 * r)) for r in range(Ri, Ro + 1)]
                bs, br = step_byte_bounds(D, sum(k // 2 + 1 for k in nsam), sum(nsam), nsam[-1], 2 * nsam[-1] - 1)
                rec.update({"shift_step_us_per_chain": round(1e6 * s["shift_steps_seconds"] / nshift, 3), "shift_step_hbm_bound_us_per_chain": round(1e6 * bs / HBM_BYTES_PER_S, 3),
                            "rotation_step_us_per_chain": round(1e6 * s["rotation_steps_seconds"] / nrot, 3),
                            "rotation_step_hbm_bound_us_per_chain": round(1e6 * br / HBM_BYTES_PER_S, 3),
                            "shift_steps_ms": round(1e3 * s["shift_steps_seconds"], 3), "rotation_steps_ms": round(1e3 * s["rotation_steps_seconds"], 3)})
            out["align"].append(rec)
            print(json.dumps(rec), flush=True)
            h.close()
        base = next(r for r in out["align"] if r["size"] == D and r["batch_chains"] == min(a.batches))
        for r in out["align"]:
            if r["size"] == D:
                r["speedup_over_one_pair_per_batch"] = round(r["pairs_per_s"] / base["pairs_per_s"], 2)
        del dg, di
    # both weighting stages on synthetic correlations
    G = a.weight_directions
    from tests import synth
    dirs = np.asarray(synth.fibonacci_directions(G))
    h = xa.ReconstructSignificant(ctx, 64, 1, batch_chains=4)
    for N in a.weight_images:
        gen = torch.Generator(device="cuda").manual_seed(1)
        cc = torch.rand((N, G), dtype=torch.float64, device="cuda", generator=gen)
        imed = torch.rand((N, G), dtype=torch.float64, device="cuda", generator=gen) + 0.5
        M = torch.eye(3, dtype=torch.float64, device="cuda").repeat(N, G, 1, 1).contiguous()
        h.weights(M[:16], cc[:16].clone(), imed[:16].clone(), 1, dirs[:, 0], dirs[:, 1], 10.0, 0.95)       # warm-up
        h.weights(M, cc, imed, 1, dirs[:, 0], dirs[:, 1], 10.0, 0.95, use_imed=True, max_shift=3.0)
        s = h.stats()
        rec = {"images": N, "directions": G, "image_stage_s": round(s["image_weights_seconds"], 4), "direction_stage_s": round(s["direction_weights_seconds"], 4),
               "neighbour_count_host_s": round(s["neighbour_count_host_seconds"], 4)}
        out["weights"].append(rec)
        print(json.dumps(rec), flush=True)
        del cc, imed, M
    h.close()
    os.makedirs(os.path.dirname(a.o), exist_ok=True)
    with open(a.o, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
