"""Timing of xmipp_resolution_monogenic_signal's device side (xh_mono_*, MonoRes) on synthetic maps of size^3, a single map and two half
maps: seconds of a full sweep (after a warm-up run), ms per frequency, and with per-stage events the split of a frequency into split /
filter, the batched inverse line passes, the amplitude row pass, smoothing, statistics, select and assign, each next to the time its
HBM bytes take at 8 TB/s (the bound of a stage that only moves data). The select is compared with one torch.sort of the same keys, what
the reference does per frequency. Prints one JSON line per (size, mode); --out appends them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8e12


def stage_bytes(n, halves):
    """HBM bytes of one frequency's stages, each array read or written once per kernel that touches it"""
    N, NF = n ** 3, n * n * (n // 2 + 1)
    maps = 2 if halves else 1
    c, d, i = 16, 8, 4
    return {
        "split": maps * (NF * c + 4 * NF * c),                      # read F, write the four spectra
        "inverse": maps * 2 * (2 * 4 * NF * c),                     # y and z passes, each reads and writes the four spectra
        "rows": maps * (4 * NF * c + N * d),                        # read the four spectra, write the amplitude
        "smooth": maps * ((N * d + NF * c) + 4 * NF * c + 2 * NF * c + 4 * NF * c + (NF * c + N * d)),   # r2c rows, y z, the tail, y z, c2r rows
        "stats": N * (i + d) * (2 if halves else 1) - (N * i if halves else 0),
        "select": 6 * N * (d + i),                                  # six digit passes over values and mask
        "assign": N * i,                                            # the mask read; only voxels still at 1 or 2 touch the other arrays
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from tests import monores_ref as R
    ctx = xa.Context(0)
    lines = []
    for n in a.sizes:
        shape = (n, n, n)
        rp, rn = int(n * 0.28), int(n * 0.44)
        rng = np.random.default_rng(0)
        sig = R.synth_map(shape, 1)
        sig[R.r2_map(shape) > rp * rp] = 0.0
        out_sphere = R.r2_map(shape) >= rn * rn
        noise = [rng.standard_normal(shape) * 0.2 for _ in range(2)]
        for z in noise:
            z[out_sphere] = 0.0
        mask = torch.from_numpy(R.protein_mask(shape, rp)).cuda()
        m = xa.MonoRes(ctx, shape)
        for halves in (False, True):
            v1 = torch.from_numpy(sig + noise[0]).cuda()
            v2 = torch.from_numpy(sig + noise[1]).cuda() if halves else None
            kw = dict(vol2=v2, sampling=1.0, max_res=12.0, step=0.25)

            def sweep():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = m.run(v1, mask, **kw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, r
            sweep()                                     # warm-up: code objects
            t_full, r = sweep()
            nfreq = len(r["steps"])
            m.set_timing(True)
            t_timed, _ = sweep()
            m.set_timing(False)
            ms = m.stage_ms()
            by = stage_bytes(n, halves)
            per = {k: round(v / nfreq, 4) for k, v in ms.items()}
            bound = {k: round(by[k] / HBM * 1e3, 4) for k in ms}
            # the select alone against one full sort of the same keys
            amp = m.amplitude(v1, 0.25, 0.23, 0.27, True).view(-1)
            reps = 10
            rank = int(amp.numel() * 0.95)
            m.select(amp, rank)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                m.select(amp, rank)
            t_sel = (time.perf_counter() - t0) / reps * 1e3
            torch.sort(amp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                torch.sort(amp)
            torch.cuda.synchronize()
            t_sort = (time.perf_counter() - t0) / reps * 1e3
            line = {"bench": "resolution_monogenic_signal", "size": n, "half_maps": halves, "frequencies": nfreq, "stop": r["stop"],
                    "sweep_s": round(t_full, 4), "sweep_timed_s": round(t_timed, 4), "ms_per_frequency": round(sum(ms.values()) / nfreq, 4),
                    "stage_ms_per_frequency": per, "stage_hbm_bound_ms": bound, "select_ms": round(t_sel, 4), "torch_sort_ms": round(t_sort, 4)}
            print(json.dumps(line), flush=True)
            lines.append(line)
        m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
