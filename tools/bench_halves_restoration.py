"""Timing of xmipp_volume_halves_restoration's device stages (xh_halves_*) on synthetic half maps of size^3: --denoising 2,
--deconvolution 2, --filterBank 0.01 0.5 1 3, --difference 2, each stage timed alone after a warm-up run. The filter bank is run once more
with per-band events, which splits a band into its two inverse transforms (with the band filters), the CDF (200 order statistics by radix
select) and the weights. cdf_* compares one CDF with reading its N doubles once (N 8 B over its time, as a fraction of 8 TB/s);
torch_sort_ms is one full sort of the same keys by torch.sort (the device's library radix sort), what the reference does per band.
Prints one JSON line."""
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
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import xmipp3_amd as xa
    from tests.test_gpu_halves_restoration import halves
    n = a.size
    shape = (n, n, n)
    V1, V2 = halves(shape, 0)
    d1, d2 = torch.from_numpy(V1).cuda(), torch.from_numpy(V2).cuda()
    ctx = xa.Context(0)
    h = xa.HalvesRestoration(ctx, shape)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    stages = [("denoise", lambda: h.denoise(2)), ("deconvolve", lambda: h.deconvolve(2, 0.2, 0.001)),
              ("filter_bank", lambda: h.filter_bank(0.01, 0.5, 1, 3)), ("difference", lambda: h.difference(2, 1.5))]
    h.load(d1, d2)
    for _, f in stages:                      # warm-up: code objects
        f()
    h.load(d1, d2)
    ms = {}
    for name, f in stages:
        ms[name], _ = timed(f)
    total = sum(ms.values())
    # the filter bank again, with events per band
    h.load(d1, d2)
    h.set_timing(True)
    t_fb_timed, _ = timed(lambda: h.filter_bank(0.01, 0.5, 1, 3))
    h.set_timing(False)
    bands, band_ms = h.band_timing()
    # one CDF alone, keys 0.5 (a - b)^2 as the filter bank's
    h.cdf(d1, d2, mult=0.5)
    reps = 10
    t_cdf, _ = timed(lambda: [h.cdf(d1, d2, mult=0.5) for _ in range(reps)])
    t_cdf /= reps
    N = n ** 3
    keys = 0.5 * (d1 - d2) * (d1 - d2)
    torch.sort(keys.view(-1))
    t_sort, _ = timed(lambda: [torch.sort(keys.view(-1)) for _ in range(reps)])
    t_sort /= reps
    print(json.dumps({"bench": "volume_halves_restoration", "size": n, "stage_ms": {k: round(v, 2) for k, v in ms.items()}, "total_ms": round(total, 2),
                      "filter_bank_bands": bands, "filter_bank_timed_ms": round(t_fb_timed, 2),
                      "per_band_ms": {"transforms": round(band_ms[0] / bands, 4), "cdf": round(band_ms[1] / bands, 4), "weights": round(band_ms[2] / bands, 4)},
                      "cdf_ms": round(t_cdf, 4), "cdf_read_once_gbps": round(N * 8 / (t_cdf * 1e-3) / 1e9, 1),
                      "cdf_fraction_of_8tbps": round(N * 8 / (t_cdf * 1e-3) / 8e12, 4), "torch_sort_ms": round(t_sort, 4)}))


if __name__ == "__main__":
    main()
