#!/usr/bin/env python3
"""CPU model of k_rf_grid's schedule: how long a launch takes, relative to a perfect split of its work over the waves, for a given
order of the tile list. No GPU; numpy only.

    python3 tools/sim_grid_schedule.py [--mv 512] [--radius 1.9] [--n 4096] [--cus 256] [--orders morton,0.05] [--cache FILE.npz]

1. Work per unit (8 x 8 x 4 voxels) for a set of orientations (--n projections on --dirs Fibonacci directions with random in-plane
   angles, the bench's shape; --dirs 0: random directions): visits, from the kernel's own cull test per (unit, projection), and
   batches of 64 voxels, from the voxels of the unit inside the projection's slab, counted on 32 sample points per unit.
   cost = --visit-cost x visits + batches.
2. The tile order, read from tools/tile_order_dump.cpp (built here with the host compiler), which includes the library's own
   xh_rf_tiles.h: "morton" is the order without heads, a number is the heavy fraction (XG_HEAVY_FRAC), "default" the library's.
3. An event simulation of the ring as the kernel runs it: one workgroup of 12 waves per CU, 64 streams (class c, sub-stream j:
   entries j, j + 8, ... of the class), home stream (b & 7) * 8 + ((b >> 3) & 7), hopping to the next stream when one is empty, a tile
   grabbed two ahead, eight tickets per tile drawn by whichever wave of the workgroup is free. A wave runs faster when fewer waves
   share its CU: speed (12 / n) ^ --speed-exp, at most --speed-cap.
Prints per order: makespan / ideal (ideal = total cost / waves) and mean occupancy (busy wave time / (makespan x waves))."""
import argparse
import heapq
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NW, NSUB = 12, 8


def euler_matrix(rot, tilt, psi):
    a, b, g = np.radians([rot, tilt, psi])
    ca, cb, cg, sa, sb, sg = np.cos(a), np.cos(b), np.cos(g), np.sin(a), np.sin(b), np.sin(g)
    cc, cs, sc, ss = cb * ca, cb * sa, sb * ca, sb * sa
    return np.array([[cg * cc - sg * sa, cg * cs + sg * ca, -cg * sb], [-sg * cc - cg * sa, -sg * cs + cg * ca, sg * sb], [sc, ss, cb]])


def orientations(n, ndirs, seed):
    rng = np.random.default_rng(seed)
    if ndirs > 0:
        i = np.arange(ndirs) + 0.5
        tilt = np.degrees(np.arccos(1 - 2 * i / ndirs))
        rot = np.degrees((np.pi * (1 + 5 ** 0.5) * i) % (2 * np.pi))
        k = rng.integers(ndirs, size=n)
        rot, tilt = rot[k], tilt[k]
    else:
        rot, tilt = rng.uniform(0, 360, n), np.degrees(np.arccos(rng.uniform(-1, 1, n)))
    return np.stack([rot, tilt, rng.uniform(0, 360, n)], 1)


def build_dump(workdir):
    exe = os.path.join(workdir, "tile_order_dump")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-I", os.path.join(ROOT, "xmipp3_amd", "csrc"),
                           os.path.join(ROOT, "tools", "tile_order_dump.cpp"), "-o", exe])
    return exe


def tile_order(exe, mv, radius, waves, order):
    cmd = [exe, str(mv), repr(radius), str(waves)] + ([] if order == "default" else [order])
    lines = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.split("\n")
    off = [int(v) for v in lines[1].split()[1:]]
    head = [int(v) for v in lines[2].split()[1:]]
    tiles = np.array([[int(v) for v in l.split()[:3]] for l in lines[3:] if l], dtype=np.int64)
    return tiles, off, head


def unit_work(tiles, mv, radius, ang):
    """visits and batches per (tile, unit) for the tiles in the given (canonical) order"""
    sizeX = mv // 2
    sub = np.arange(8)
    x0 = tiles[:, None, 0] * 16 + (sub & 1) * 8
    y0 = tiles[:, None, 1] * 16 + ((sub >> 1) & 1) * 8
    z0 = tiles[:, None, 2] * 8 + (sub >> 2) * 4
    uc = np.stack([x0 + 3.5 - sizeX, y0 + 3.5 - sizeX, z0 + 1.5 - sizeX], -1).reshape(-1, 3).astype(np.float32)
    # 32 sample points per unit: every second voxel
    gx, gy, gz = np.meshgrid(np.arange(0.5, 8, 2) - 3.5, np.arange(0.5, 8, 2) - 3.5, np.arange(0.5, 4, 2) - 1.5, indexing="ij")
    offs = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1).astype(np.float32)
    visits = np.zeros(len(uc), np.int64)
    batches = np.zeros(len(uc), np.int64)
    items = 0
    r = np.float32(radius)
    lim2 = (sizeX + radius) ** 2
    orig = uc + sizeX                       # voxel index of the unit's centre; samples outside the volume [0, mv] do not count
    for a in ang:
        A = euler_matrix(*a).astype(np.float32)
        n, xv = A[2], A[0]
        dn, dx = uc @ n, uc @ xv
        hn = min(5.2, 3.5 * (abs(n[0]) + abs(n[1])) + 1.5 * abs(n[2]) + 0.02)
        hx = min(5.2, 3.5 * (abs(xv[0]) + abs(xv[1])) + 1.5 * abs(xv[2]) + 0.02)
        keep = np.nonzero((np.abs(dn) <= r + hn) & (dx >= -(r + hx)) & (dx <= sizeX + r + hx))[0]
        visits[keep] += 1
        p = uc[keep, None, :] + offs[None]
        inside = (np.abs(p @ n) <= r) & (p @ xv >= -r) & ((p * p).sum(-1) <= lim2) & ((orig[keep, None, :] + offs[None]).max(-1) <= mv)
        it = inside.sum(1) * 8
        items += int(it.sum())
        batches[keep] += (it + 63) // 64
    return visits.reshape(-1, 8), batches.reshape(-1, 8), items


def simulate(order_rows, off, cost, cus, speed_exp, speed_cap):
    """order_rows: row of `cost` per list entry. Returns makespan, busy wave time."""
    nblocks = 8 * max(1, cus // 8)
    nstreams = 8 * NSUB
    counter = [0] * nstreams
    stream_len = []
    for st in range(nstreams):
        c, j = divmod(st, NSUB)
        nt = off[c + 1] - off[c]
        stream_len.append((nt - j + NSUB - 1) // NSUB if nt > j else 0)
    speed = [0.0] + [min(speed_cap, (NW / n) ** speed_exp) for n in range(1, NW + 1)]

    class WG:
        pass
    wgs = []
    for b in range(nblocks):
        w = WG()
        w.home = (b & 7) * NSUB + ((b >> 3) & (NSUB - 1))
        w.hop, w.ticket, w.ring, w.v, w.t, w.n, w.heap = 0, 0, {}, 0.0, 0.0, NW, []
        wgs.append(w)

    def produce(w, q):
        tile = -1
        while w.hop < nstreams:
            st = (w.home + w.hop) % nstreams
            k = counter[st]
            counter[st] += 1
            if k < stream_len[st]:
                tile = order_rows[off[st // NSUB] + st % NSUB + k * NSUB]
                break
            w.hop += 1
        w.ring[q] = tile

    def draw(w):
        """the free wave of w takes tickets until one has work; False: the ring is empty, the wave leaves"""
        while True:
            t = w.ticket
            w.ticket += 1
            q = t >> 3
            if (t & 7) == 0:
                produce(w, q + 2)
            tile = w.ring[q]
            if tile < 0:
                return False
            c = cost[tile][t & 7]
            if c > 0:
                heapq.heappush(w.heap, w.v + c)
                return True

    for w in wgs:
        produce(w, 0)
        produce(w, 1)
    events = []
    busy = 0.0
    for b, w in enumerate(wgs):
        for _ in range(NW):
            if not draw(w):
                w.n -= 1
        if w.heap:
            heapq.heappush(events, (w.heap[0] / speed[w.n], b))
    makespan = 0.0
    while events:
        t, b = heapq.heappop(events)
        w = wgs[b]
        w.v, w.t = heapq.heappop(w.heap), t
        makespan = max(makespan, t)
        if not draw(w):
            w.n -= 1
            busy += t
        if w.heap:
            heapq.heappush(events, (w.t + (w.heap[0] - w.v) / speed[w.n], b))
    return makespan, busy, nblocks * NW


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mv", type=int, default=512)
    ap.add_argument("--radius", type=float, default=1.9)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--dirs", type=int, default=1000)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--orders", default="morton,default")
    ap.add_argument("--visit-cost", type=float, default=1.3)
    ap.add_argument("--speed-exp", type=float, default=0.75)
    ap.add_argument("--speed-cap", default="2.2", help="comma-separated: one simulation each")
    ap.add_argument("--cache", default=None, help="npz file for the per-unit work (computed when missing)")
    args = ap.parse_args()
    waves = args.cus * NW
    with tempfile.TemporaryDirectory() as wd:
        exe = build_dump(wd)
        orders = {o: tile_order(exe, args.mv, args.radius, waves, o) for o in args.orders.split(",")}
    canon = next(iter(orders.values()))[0]
    canon = canon[np.lexsort((canon[:, 0], canon[:, 1], canon[:, 2]))]
    row = {tuple(t): i for i, t in enumerate(canon.tolist())}
    if args.cache and os.path.exists(args.cache):
        z = np.load(args.cache)
        visits, batches, items = z["visits"], z["batches"], int(z["items"])
        assert visits.shape == (len(canon), 8), "the cache is of another tile set"
    else:
        visits, batches, items = unit_work(canon, args.mv, args.radius, orientations(args.n, args.dirs, args.seed))
        if args.cache:
            np.savez_compressed(args.cache, visits=visits, batches=batches, items=items)
    cost = (args.visit_cost * visits + batches).tolist()
    total = float(args.visit_cost * visits.sum() + batches.sum())
    print(f"mv {args.mv} radius {args.radius} n {args.n} dirs {args.dirs} waves {waves} tiles {len(canon)}")
    print(f"visits {visits.sum() / 1e6:.2f} M  batches {batches.sum() / 1e6:.2f} M  items per visit {items / max(1, visits.sum()):.1f}")
    print(f"heaviest unit: {visits.max()} visits, {(args.visit_cost * visits + batches).max() / (total / waves):.2f} of the mean load of a wave")
    for cap in [float(c) for c in args.speed_cap.split(",")]:
        for name, (tiles, off, head) in orders.items():
            rows = [row[tuple(t)] for t in tiles.tolist()]
            mk, busy, nw = simulate(rows, off, cost, args.cus, args.speed_exp, cap)
            print(f"order {name:8s} heads {sum(head):5d}  speed cap {cap:.1f}  makespan / ideal {mk / (total / nw):.3f}  mean occupancy {busy / (mk * nw):.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
