"""The launch geometry of the line kernels (stardis_amd/csrc/sdx_line_geom.h) on the host, no GPU: the two decode functions the kernels
call — narrow_unit(block, wave) and wide_unit(block) — and line_launch_make, which the host's launch code calls, run in a stand-alone
program (tests/line_geom_probe.cpp, built here with the host compiler) over EVERY block index and wave of each launch below, and are
compared with plain integer arithmetic written from the formulas the kernels had before the header existed (64-bit divisions per wave,
the tile-prefix loop, the `roles` word).  The division helper is checked at the edges of its stated range, 0 <= n < 2^31, 1 <= d < 2^31.

Launches: nu_begin in {0, 1, 255, 257, 12301} x nu_count in {1, 7, 64, 257, 7634, 120398} x depths in {1, 56, 64, 65, 129} x F in {1, 2, 4}
x n_split in {2, 4, 8}, the subsets kernels' narrow role (F = 4) beside the plain one, the three narrow orders; wide role: 1, 7, 8, 9, 471
and 4703 tiles x wide_group in {0, 1, 2}, with and without a far role's workgroups in front; one role switched off; the range refusal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NU_BEGIN = (0, 1, 255, 257, 12301)
NU_COUNT = (1, 7, 64, 257, 7634, 120398)
DEPTHS = (1, 56, 64, 65, 129)
TILE = 256


class Probe:
    def __init__(self, exe):
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE)

    def read(self, dtype, count):
        data = self.p.stdout.read(np.dtype(dtype).itemsize * count)
        assert len(data) == np.dtype(dtype).itemsize * count, "the probe ended early"
        return np.frombuffer(data, dtype=dtype)

    def launch(self, nu_begin, nu_count, n_depth, n_split, narrow_f, subsets, wide_group=0, order=0, mask=3, far_blocks=0, tile=TILE):
        self.p.stdin.write(f"G {nu_begin} {nu_count} {n_depth} {n_split} {tile} {narrow_f} {int(subsets)} {wide_group} {order} {mask} {far_blocks}\n".encode())
        self.p.stdin.flush()
        ok, blocks, wide_first, narrow_first = (int(v) for v in self.read(np.int64, 4))
        if not ok:
            return None
        wide = self.read(np.int32, 3 * (narrow_first - wide_first)).reshape(-1, 3)
        narrow = self.read(np.int32, 3 * (blocks - narrow_first) * n_split).reshape(-1, n_split, 3)
        return blocks, wide_first, narrow_first, wide, narrow

    def div(self, d, ns):
        self.p.stdin.write((f"D {d} {len(ns)} " + " ".join(str(n) for n in ns) + "\n").encode())
        self.p.stdin.flush()
        return self.read(np.int64, len(ns))

    def close(self):
        self.p.stdin.close()
        assert self.p.wait(timeout=60) == 0


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("line_geom") / "line_geom_probe")
    proc = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "line_geom_probe.cpp")], capture_output=True,
                          text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    p = Probe(exe)
    yield p
    p.close()


def narrow_reference(nu_begin, nu_count, n_depth, n_split, F, subsets, order, on=True):
    """the narrow role of line_all_body as it stood: (blocks, i0 [blocks][n_split], chunk, live), and the number of units"""
    g0 = nu_begin // F
    n_grp = (nu_begin + nu_count + F - 1) // F - g0
    n_narrow = n_grp * ((n_depth + 63) // 64)
    n_nb = n_narrow if subsets else (n_narrow + n_split - 1) // n_split
    group = 16 if subsets else 4
    blocks = (n_nb + 8 * group - 1) // (8 * group) * (8 * group)  # (the host: whole rounds of the XCD-aware order)
    p = np.arange(blocks, dtype=np.int64)
    j = p >> 3
    wg = ((j // group) * 8 + (p & 7)) * group + j % group
    if order == 1:
        wg = p
    if order == 2:
        wg = (p & 7) * ((n_nb + 7) // 8) + j
    dead = wg >= n_nb
    if order == 2:
        dead |= j >= (n_nb + 7) // 8
    wave = np.arange(n_split, dtype=np.int64)
    c = np.repeat(wg[:, None], n_split, axis=1) if subsets else wg[:, None] * n_split + wave[None, :]
    live = ~dead[:, None] & (c < n_narrow) & on
    return blocks, (g0 + c % n_grp) * F, c // n_grp, live, n_narrow


def wide_reference(nu_begin, nu_count, n_depth, wide_group, on=True, tile_points=TILE):
    """the wide role of line_all_body as it stood: (n_wide, tile [n_wide], depth, live)"""
    tiles = (nu_begin + nu_count + tile_points - 1) // tile_points - nu_begin // tile_points
    wg = wide_group
    tiles_pad = (tiles + 8 * wg - 1) // (8 * wg) * (8 * wg) if wg else tiles
    b = np.arange(tiles_pad * n_depth, dtype=np.int64)
    if wg == 0:
        p, d = b % tiles, b // tiles
        tile = p >> 3
        for f in range(7):
            tile = tile + np.where(f < (p & 7), (tiles - f + 7) >> 3, 0)
    else:
        p, d = b % tiles_pad, b // tiles_pad
        j = p >> 3
        tile = ((j // wg) * 8 + (p & 7)) * wg + j % wg
    return b.size, tile, d, (tile < tiles) & on, tiles


def check_narrow(probe, nu_begin, nu_count, n_depth, n_split, F, subsets, order=0, mask=3, far_blocks=0):
    got = probe.launch(nu_begin, nu_count, n_depth, n_split, F, subsets, order=order, mask=mask, far_blocks=far_blocks)
    assert got is not None
    blocks, wide_first, narrow_first, _, narrow = got
    ref_blocks, i0, chunk, live, n_narrow = narrow_reference(nu_begin, nu_count, n_depth, n_split, F, subsets, order, on=bool(mask & 2))
    what = (nu_begin, nu_count, n_depth, n_split, F, subsets, order, mask)
    assert wide_first == far_blocks and blocks - narrow_first == ref_blocks, what
    assert np.array_equal(narrow[:, :, 2] != 0, live), what
    assert np.array_equal(narrow[:, :, 0][live], i0[live]) and np.array_equal(narrow[:, :, 1][live], chunk[live]), what
    if mask & 2:  # every unit exactly once (subsets: once per wave of its workgroup)
        units = (narrow[:, :, 1][live].astype(np.int64) << 32) | narrow[:, :, 0][live]
        assert np.unique(units).size == n_narrow and units.size == n_narrow * (n_split if subsets else 1), what
        assert narrow[:, :, 0][live].max() < nu_begin + nu_count and narrow[:, :, 0][live].min() > nu_begin - F, what
        assert narrow[:, :, 1][live].max() * 64 < n_depth, what


def check_wide(probe, nu_begin, nu_count, n_depth, wide_group, mask=3, far_blocks=0, tile_points=TILE):
    got = probe.launch(nu_begin, nu_count, n_depth, 2, 1, False, wide_group=wide_group, mask=mask, far_blocks=far_blocks, tile=tile_points)
    assert got is not None
    _, wide_first, narrow_first, wide, _ = got
    n_wide, tile, depth, live, tiles = wide_reference(nu_begin, nu_count, n_depth, wide_group, on=bool(mask & 1), tile_points=tile_points)
    what = (nu_begin, nu_count, n_depth, wide_group, mask, far_blocks, tiles)
    assert wide_first == far_blocks and narrow_first - wide_first == n_wide, what
    assert np.array_equal(wide[:, 2] != 0, live), what
    assert np.array_equal(wide[:, 0][live], tile[live]) and np.array_equal(wide[:, 1][live], depth[live]), what
    if mask & 1:  # every (tile, depth) exactly once
        assert np.unique(wide[:, 1][live].astype(np.int64) * tiles + wide[:, 0][live]).size == tiles * n_depth == int(live.sum()), what
    return tiles


def test_narrow_units_of_every_block_and_wave(probe):
    for nu_begin in NU_BEGIN:
        for nu_count in NU_COUNT:
            for n_depth in DEPTHS:
                for n_split in (2, 4, 8):
                    for F in (1, 2, 4):
                        check_narrow(probe, nu_begin, nu_count, n_depth, n_split, F, False)
                    check_narrow(probe, nu_begin, nu_count, n_depth, n_split, 4, True)  # (the subsets kernels: R = F = 4)


def test_narrow_orders_switched_off_role_and_far_blocks_in_front(probe):
    for nu_begin in NU_BEGIN:
        for nu_count in NU_COUNT[:5]:
            for n_depth in DEPTHS:
                for order in (1, 2):
                    for F in (1, 4):
                        check_narrow(probe, nu_begin, nu_count, n_depth, 2, F, False, order=order)
                    check_narrow(probe, nu_begin, nu_count, n_depth, 4, 4, True, order=order)
                check_narrow(probe, nu_begin, nu_count, n_depth, 4, 2, False, mask=1)
                check_narrow(probe, nu_begin, nu_count, n_depth, 4, 4, False, far_blocks=3 * n_depth)


def test_wide_units_of_every_block(probe):
    seen = set()
    for tiles in (1, 7, 8, 9, 471, 4703):
        for nu_begin, nu_count in ((0, tiles * TILE), (257, (tiles - 1) * TILE - 5 if tiles > 1 else 3), (255, (tiles - 1) * TILE + 1)):
            for n_depth in DEPTHS:
                for wide_group in (0, 1, 2):
                    seen.add(check_wide(probe, nu_begin, nu_count, n_depth, wide_group))
                    seen.add(check_wide(probe, nu_begin, nu_count, n_depth, wide_group, far_blocks=5 * n_depth))
                check_wide(probe, nu_begin, nu_count, n_depth, 0, mask=2)
    assert seen >= {1, 7, 8, 9, 471, 4703}, seen
    # the listed shards too, 512-point tiles (which no kernel runs any more: the header takes any tile) and a wide group that is no power of two
    for nu_begin in NU_BEGIN:
        for nu_count in NU_COUNT:
            check_wide(probe, nu_begin, nu_count, 56, 0)
            check_wide(probe, nu_begin, nu_count, 65, 2, tile_points=512)
            check_wide(probe, nu_begin, nu_count, 7, 3)


def test_division_helper_at_the_edges_of_its_range(probe):
    top = 2**31 - 1
    rng = np.random.default_rng(7)
    divisors = [1, 2, 3, 5, 7, 30, 255, 256, 257, 471, 3817, 7634, 65535, 65536, 65537, 120398, 263000, 2**30 - 1, 2**30, 2**30 + 1, top - 512, top - 1, top]
    divisors += [int(d) for d in rng.integers(1, top, 40)]
    for d in divisors:
        ns = {0, 1, top, top - 1, top - 2}
        for k in (1, 2, 3, top // d - 1, top // d):
            for e in (-1, 0, 1):
                ns.add(k * d + e)
        ns |= {int(n) for n in rng.integers(0, top, 200)}
        ns = sorted(n for n in ns if 0 <= n <= top)
        assert np.array_equal(probe.div(d, ns), np.array(ns, dtype=np.int64) // d), d


def test_a_launch_beyond_the_stated_range_is_refused(probe):
    assert probe.launch(0, 2**31, 56, 2, 1, False) is None            # frequency indices
    assert probe.launch(0, 2**31 - 600, 129, 2, 1, False) is None     # narrow units (three depth chunks)
    assert probe.launch(0, 2**28, 129, 2, 1, False, far_blocks=2**31 - 2**27) is None  # workgroups
    assert probe.launch(0, 7634, 56, 2, 3, False) is None             # F is 1, 2 or 4
    assert probe.launch(0, 7634, 56, 2, 1, False) is not None
