"""The gridding kernel's tile list (xmipp3_amd/csrc/xh_rf_tiles.h) through tools/tile_order_dump.cpp, a stand-alone host program
built here with the address and undefined-behaviour sanitizers: the set of tiles, the equal-work classes, and in every class a head
of heavy tiles (heaviest first) followed by the rest in Morton order."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES = 256 * 12           # MI355X: 256 CUs, XgCfg::NW waves on each
CASES = [(64, 1.9), (80, 1.9), (100, 1.9), (512, 1.9), (64, 2.5)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("tile_order") / "tile_order_dump")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "xmipp3_amd", "csrc"), os.path.join(ROOT, "tools", "tile_order_dump.cpp"), "-o", exe])
    cache = {}

    def run(mv, radius):
        if (mv, radius) not in cache:
            cache[(mv, radius)] = subprocess.run([exe, str(mv), repr(radius), str(WAVES)], check=True, capture_output=True).stdout
        return cache[(mv, radius)]
    run.exe = exe
    return run


def _parse(raw):
    lines = raw.decode().split("\n")
    off = [int(v) for v in lines[1].split()[1:]]
    head = [int(v) for v in lines[2].split()[1:]]
    tiles, est = [], []
    for l in lines[3:]:
        if l:
            f = l.split()
            tiles.append((int(f[0]), int(f[1]), int(f[2])))
            est.append(float(f[3]))
    assert lines[0].split()[-1] == str(len(tiles))
    return off, head, tiles, est


def _spread(v):
    x = 0
    for b in range(10):
        x |= ((v >> b) & 1) << (3 * b)
    return x


def _morton(t):
    # on (x, y, z / 2), the low bit of z last
    return ((_spread(t[0]) | _spread(t[1]) << 1 | _spread(t[2] >> 1) << 2) << 1) | (t[2] & 1)


def _expected(mv, radius):
    """The tiles within reach, in raster order (z, y, x), and the equal-work split of that order into eight classes."""
    tpx, tpz = (mv + 1 + 15) // 16, (mv + 1 + 7) // 8
    R = mv // 2 + radius + math.sqrt(2 * 7.5 * 7.5 + 3.5 * 3.5) + 1.0
    tiles, wsum, acc = [], [], 0.0
    for tz in range(tpz):
        for ty in range(tpx):
            for tx in range(tpx):
                d = math.sqrt((tx * 16 + 7.5 - mv // 2) ** 2 + (ty * 16 + 7.5 - mv // 2) ** 2 + (tz * 8 + 3.5 - mv // 2) ** 2)
                if d <= R:
                    tiles.append((tx, ty, tz))
                    acc += 1.0 / max(d, 8.0)
                    wsum.append(acc)
    off = [0]
    for c in range(1, 8):
        target = acc * c / 8.0
        off.append(next(i for i, w in enumerate(wsum) if w >= target))
    off.append(len(tiles))
    return tiles, off


def _near_origin(t, mv):
    """does the tile hold a voxel less than 8 from the origin (voxel mv / 2 on every axis)? At mv 512 these are the eight tiles that
    share the origin as a corner (the ninth at exactly 8, (16, 16, 33), touches it with one voxel only)."""
    d2 = 0
    for lo, n in ((t[0] * 16, 16), (t[1] * 16, 16), (t[2] * 8, 8)):
        c = mv // 2
        d = max(lo - c, 0, c - (lo + n - 1))
        d2 += d * d
    return d2 < 64


@pytest.mark.parametrize("mv,radius", CASES)
def test_tile_list(dump, mv, radius):
    off, head, tiles, est = _parse(dump(mv, radius))
    exp_tiles, exp_off = _expected(mv, radius)
    # exactly the tiles within reach, each once
    assert len(tiles) == len(set(tiles)) and set(tiles) == set(exp_tiles)
    # the classes: contiguous pieces of the raster order, cut at equal estimated work
    assert off == exp_off
    for c in range(8):
        assert set(tiles[off[c]:off[c + 1]]) == set(exp_tiles[off[c]:off[c + 1]])
    heads = set()
    for c in range(8):
        n, h = off[c + 1] - off[c], head[c]
        assert 0 <= h <= n
        he, hk = est[off[c]:off[c] + h], [_morton(t) for t in tiles[off[c]:off[c] + h]]
        # head: non-increasing estimate, ties by Morton key
        assert all(a > b or (a == b and ka < kb) for a, b, ka, kb in zip(he, he[1:], hk, hk[1:]))
        rk = [_morton(t) for t in tiles[off[c] + h:off[c + 1]]]
        assert all(a < b for a, b in zip(rk, rk[1:]))
        # nothing in the remainder is heavier than the lightest tile of the head
        if h and h < n:
            assert max(est[off[c] + h:off[c + 1]]) <= min(he)
        heads.update(tiles[off[c]:off[c] + h])
    near = [t for t in tiles if _near_origin(t, mv)]
    assert near and all(t in heads for t in near)
    if mv == 512:
        # the origin sits at the seam of classes 3 and 4, on a corner shared by eight tiles: four open each of the two classes
        assert len(near) == 8
        assert sorted(tiles[off[3]:off[3] + 4] + tiles[off[4]:off[4] + 4]) == sorted(near)
        assert 8 < sum(head) < 2048


def test_two_runs_print_the_same_bytes(dump):
    for mv, radius in CASES:
        again = subprocess.run([dump.exe, str(mv), repr(radius), str(WAVES)], check=True, capture_output=True).stdout
        assert again == dump(mv, radius) and len(again) > 0


def test_morton_argument_gives_no_heads(dump):
    """"morton" is the order before the heads (the schedule model's baseline): same tiles and classes, every class in Morton order"""
    raw = subprocess.run([dump.exe, "100", "1.9", str(WAVES), "morton"], check=True, capture_output=True).stdout
    off, head, tiles, _ = _parse(raw)
    off2, _, tiles2, _ = _parse(dump(100, 1.9))
    assert head == [0] * 8 and off == off2
    for c in range(8):
        k = [_morton(t) for t in tiles[off[c]:off[c + 1]]]
        assert k == sorted(k) and set(tiles[off[c]:off[c + 1]]) == set(tiles2[off[c]:off[c + 1]])
