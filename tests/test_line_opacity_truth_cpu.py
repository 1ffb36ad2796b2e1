"""The reference alone meets the conditions tests/test_gpu_line_opacity_truth.py rests on (tests/line_opacity_truth.py): every probe
item of every hostile class has exactly the half-width, centre and window edges its class claims, every class reaches the decision it
is named for — recomputed here from the documented constants of the line path —, every term of a probe line is visible in the sum, few
terms hug a Humlicek boundary, and the fp64 oracle stays within 1e-12 of the extended-precision truth.  No GPU."""
import numpy as np
import pytest

import line_opacity_truth as T
import oracle

pytestmark = pytest.mark.skipif(not T.EXTENDED, reason="no extended-precision long double on this host")

SMALL = T.NAMES


def expected_window(c, l, d):
    hw, centre = int(c.hw[l, d]), int(c.centre[l])
    if centre < 0:
        centre = int(T.centre_index(c.nus, c.line_nus[l]))
    return max(centre - hw, 0), min(centre + hw, c.n_nu)


@pytest.mark.parametrize("name", SMALL + T.WALKS)
def test_probe_items_have_the_windows_their_class_claims(name):
    c = T.case(name)
    assert c.probe.any() and np.all(np.diff(c.line_nus) >= 0)
    r = c.reference()
    t = r["t"]
    d_nu = T.d_nu_of(c.nus)
    assert d_nu == T.D
    for l in np.flatnonzero(c.probe):
        if c.centre[l] >= 0:
            assert T.centre_index(c.nus, c.line_nus[l]) == c.centre[l], l
        for d in range(c.n_depth):
            g = c.gammas[l, d if c.gammas.shape[1] > 1 else 0]
            assert T.half_width_of(g, c.dw[l, d], c.alphas[l, d], d_nu, c.n_nu) == c.hw[l, d], (l, d)
            want = expected_window(c, l, d)
            assert oracle.window(c.nus, c.line_nus[l], g, c.dw[l, d], c.alphas[l, d]) == want, (l, d)
            assert (t.lo[l, d], t.hi[l, d]) == want
    # ... and the oracle's evaluation count is the sum of the windows
    assert r["evals"] == int(np.maximum(t.hi - t.lo, 0).sum()) == t.n_terms


@pytest.mark.parametrize("name", SMALL + T.WALKS)
def test_visibility_excluded_share_and_the_oracle_against_the_truth(name):
    c = T.case(name)
    r = c.reference()
    t = r["t"]
    # every term of a probe line: at least VISIBLE of the truth at its point, or exactly zero
    with np.errstate(all="ignore"):
        share = np.where(t.plane[None] > 0, t.probe_terms / t.plane[None], T.L(0))
    inside = np.zeros(t.probe_terms.shape, dtype=bool)
    for k, l in enumerate(t.probe_index):
        for d in range(c.n_depth):
            inside[k, d, t.lo[l, d]:t.hi[l, d]] = True
    assert np.all(t.probe_terms[~inside] == 0)
    visible = (share >= T.VISIBLE) | (t.probe_terms == 0)
    assert visible[inside].all(), float(share[inside & ~visible].min())
    if name not in ("class_edges", "profiles"):  # (their alpha = 0 / underflowing items are the exactly-zero terms)
        assert np.all(t.probe_terms[inside] > 0)
    assert t.n_near <= T.NEAR_SHARE * t.n_terms, (t.n_near, t.n_terms)
    assert t.n_near32 <= T.NEAR_SHARE * t.n_terms or c.cls == "profiles", (t.n_near32, t.n_terms)  # (the mixed mode's own margin)
    assert np.array_equal(r["oracle"] == 0, t.plane == 0)
    if c.cls != "profiles":
        assert r["oracle_distance"] < 1e-12
    # the probe terms and the filler's plane make up the whole
    assert T.distance(r["filler"] + t.probe_terms.sum(axis=0), t.plane) < 1e-15  # (two orders of one extended-precision sum)
    if name in ("on_points", "far_edges"):  # ... and the filler's plane is the truth of the list without its probe lines
        assert T.distance(r["filler"], T.truth(*c.args(~c.probe)).plane) < 1e-18


def test_every_class_has_its_cases():
    assert {T.case(n).cls for n in T.NAMES} == set(T.CLASSES)


def test_grid_ends_and_on_points_reach_their_ties():
    c = T.case("grid_ends")
    n, nus = c.n_nu, c.nus
    p = c.line_nus[c.probe]
    for v in (nus[0], nus[-1]):
        assert (p == v).any() and (p == np.nextafter(v, np.inf)).any() and (p == np.nextafter(v, 0.0)).any()
    beyond = sorted({round(float(v - nus[0]) / T.D, 3) for v in p if v > nus[0] + 1.0})
    assert beyond == [0.5, 9.5, 10.5, 63.0, 200.0, 5000.0]
    below = sorted({round(float(nus[-1] - v) / T.D, 3) for v in p if v < nus[-1] - 1.0})
    assert below == beyond
    # the searchsorted-left tie: a line on grid frequency i has centre i + 1, as the line an ulp below it; an ulp above it, centre i
    assert T.centre_index(nus, nus[-1]) == n and T.centre_index(nus, np.nextafter(nus[-1], np.inf)) == n - 1
    assert T.centre_index(nus, nus[0]) == 1 and T.centre_index(nus, np.nextafter(nus[0], np.inf)) == 0
    # each position with a floor, a medium, a > MEDIUM_HALF_WIDTH and a whole-grid window
    for v in np.unique(p):
        hws = set(c.hw[c.probe & (c.line_nus == v)][:, 0])
        assert hws == {10, 300, 4500, n} and 4500 > T.MEDIUM_HALF_WIDTH
    lg = T.case("grid_ends_long")  # the grid on which a shard of an indexed list is culled: every window class beyond both ends
    assert lg.n_nu > 16384
    for out in (lg.probe & (lg.line_nus > lg.nus[0]), lg.probe & (lg.line_nus < lg.nus[-1])):
        assert set(lg.hw[out][:, 0]) == {10, 300, 4500, lg.n_nu}
    assert {T.MEDIUM_HALF_WIDTH, T.MEDIUM_HALF_WIDTH + 1} <= set(lg.hw[lg.probe][:, 0])
    # beyond the blue end the window is [0, hw), beyond the red end [N - hw, N)
    t = c.reference()["t"]
    out_blue, out_red = c.probe & (c.line_nus > nus[0]), c.probe & (c.line_nus < nus[-1])
    assert np.all(t.lo[out_blue] == 0) and np.all(t.hi[out_blue] == c.hw[out_blue])
    assert np.all(t.hi[out_red] == n) and np.all(t.lo[out_red] == n - c.hw[out_red])
    c = T.case("on_points")
    for i in (255, 256, 257, 2047, 2048, c.n_nu - 1):
        on = c.probe & (c.line_nus == c.nus[i])
        assert on.any() and np.all(c.centre[on] == i + 1)
        assert np.all(c.centre[c.probe & (c.line_nus == np.nextafter(c.nus[i], 0.0))] == i + 1)
        assert np.all(c.centre[c.probe & (c.line_nus == np.nextafter(c.nus[i], np.inf))] == i)
    assert 255 % T.TILE == T.TILE - 1 and 2048 % (T.TILE * T.FAR_UNIT_TILES) == 0


def test_class_edges_sit_on_the_class_bounds():
    c = T.case("class_edges")
    hws = set(np.unique(c.hw[c.probe]))
    n = c.n_nu
    assert {10, 11, T.NARROW_HALF_WIDTH, T.NARROW_HALF_WIDTH + 1, T.NARROW_REACH, T.NARROW_REACH + 1, T.MEDIUM_HALF_WIDTH,
            T.MEDIUM_HALF_WIDTH + 1, n - 1, n} == hws
    px = T.pixels_of(c.gammas, c.dw, c.alphas, c.d_nu)[c.probe]
    assert (px == 10.0).sum() == c.n_depth  # the tie of `pixels > 10`
    assert ((px < 10.0) & (px > 9.99)).sum() == c.n_depth and ((px > 10.0) & (px < 10.01)).sum() == c.n_depth
    assert (px >= 2.0 ** 31).sum() == c.n_depth and (px == 0.0).sum() == c.n_depth
    # a half-width of MEDIUM_HALF_WIDTH + 1 that the grid does not clip
    t = c.reference()["t"]
    sel = c.probe[:, None] & (c.hw == T.MEDIUM_HALF_WIDTH + 1)
    assert sel.any() and np.all((t.hi - t.lo)[sel] == 2 * (T.MEDIUM_HALF_WIDTH + 1))


@pytest.mark.parametrize("n_depth", [65, 129])
def test_depth_varying_changes_class_between_the_depth_chunks(n_depth):
    c = T.case(f"depth_varying_{n_depth}")
    assert c.gammas.shape == (c.n_lines, 1)
    cls = np.where(c.hw > T.MEDIUM_HALF_WIDTH, 2, np.where(c.hw > T.NARROW_HALF_WIDTH, 1, 0))[c.probe]
    sat = (c.hw == c.n_nu)[c.probe]
    first, second = cls[:, :64], cls[:, 64:128]
    assert any(np.all(a[0] == a) and np.all(b[0] == b) and a[0] != b[0] for a, b in zip(first, second))
    if n_depth > 128:
        assert any(a[0] != b[-1] and sat[k, 128:].any() for k, (a, b) in enumerate(zip(first, cls[:, 128:])))
    assert any((row > T.NARROW_HALF_WIDTH).sum() == 1 for row in c.hw[c.probe])  # a line that is wide at exactly one depth
    assert any(len(set(row)) == 3 for row in c.hw[c.probe][:, :3].tolist())  # narrow, medium and saturated at neighbouring depths


@pytest.mark.parametrize("K,start", list(zip(T.COINCIDENT_K, T.COINCIDENT_START)))
@pytest.mark.parametrize("wide", [0, 1])
def test_coincident_lines_add_up(K, start, wide):
    c = T.case(f"coincident_{K}_{'wide' if wide else 'narrow'}")
    idx = np.flatnonzero(c.probe)
    assert idx.size == K and idx[0] == start and np.all(np.diff(idx) == 1)
    for a in (c.line_nus, c.dw, c.gammas, c.alphas):
        assert np.all(a[idx] == a[idx[0]])
    assert np.all((c.hw[idx] > T.NARROW_HALF_WIDTH) == bool(wide))
    t = c.reference()["t"]
    one = T.truth(*c.args(idx[:1]))
    assert T.distance(t.probe_terms.sum(axis=0), K * one.plane) < 4e-19 * K
    assert np.array_equal(t.probe_terms.sum(axis=0) == 0, one.plane == 0)


def test_coincident_runs_start_on_and_off_the_stretches():
    s = np.array(T.COINCIDENT_START)
    assert ((s % 256) == 0).any() and (((s % 64) == 0) & ((s % 256) != 0)).any() and ((s % 64) != 0).any()


@pytest.mark.parametrize("wide", [0, 1])
def test_pile_up_puts_every_centre_on_a_grid_end(wide):
    c = T.case("pile_up_wide" if wide else "pile_up_narrow")
    centre = T.centre_index(c.nus, c.line_nus)
    assert (centre == 0).sum() == 3000 and (centre == c.n_nu).sum() == 3000
    t = c.reference()["t"]
    hw = np.maximum(t.hi - t.lo, 0)
    out = (centre == 0) | (centre == c.n_nu)
    assert np.any(hw[out] > T.NARROW_HALF_WIDTH) == bool(wide)
    assert c.probe.sum() >= 60


def test_profiles_reach_their_extremes():
    c = T.case("profiles")
    assert not (~c.probe).any()
    y = (c.gammas / (T.SQRT_PI * T.PI)) / c.dw
    assert (c.gammas == 0).any() and (y == 1e-30).any() and ((c.gammas > 0) & (c.gammas < 2.3e-308)).any()
    assert np.isclose(y, 15.0).any() and np.isclose(y, 1e6).any()
    x_edge = 9 * T.D / c.dw
    assert (x_edge >= 1e8).any() and (10 * T.D / c.dw < 1e-6 * 600).any()
    t = c.reference()["t"]
    big = T.case("profiles_big").reference()["t"].plane
    assert float(big.max()) > 1e270 and 0 < float(t.plane[t.plane > 0].min()) < 1e-290
    for d in range(c.n_depth):  # whole windows with |x| < 1e-6
        for l in range(c.n_lines):
            if c.dw[l, d] > 1e16:
                assert np.abs(c.nus[t.lo[l, d]:t.hi[l, d]] - c.line_nus[l]).max() / c.dw[l, d] < 1e-6


@pytest.mark.parametrize("jump", [0, 1])
def test_far_edges_sit_on_the_far_ranges(jump):
    c = T.case("far_edges_jump" if jump else "far_edges")
    assert c.n_nu >= 8 * T.TILE and c.n_nu % T.TILE
    fr = T.far_ranges(c.nus)
    near_points = int(T.FAR_RATIO * (T.TILE // 2)) + T.TILE // 2  # sdx_far_field_rule
    if not jump:  # on a uniform grid c -+ 6 h lies 5 h = 2.5 (TILE - 1) points beyond the tile's ends (the kernel's own first guess)
        reach = (5 * (T.TILE - 1)) // 2
        for tile, (a, b) in enumerate(fr):
            assert a == max(tile * T.TILE - reach, 0) and b == min(tile * T.TILE + T.TILE + reach, c.n_nu)
            assert tile * T.TILE + T.TILE // 2 - a < near_points  # (no point the rule promises to evaluate in place is far)
    centres = set(T.centre_index(c.nus, c.line_nus[c.probe]).tolist())
    hit = 0
    for tile in ((3, 4) if jump else (3, 5)):
        for r in fr[tile]:
            for idx in (r - 1, r, r + 1):
                if 0 < idx < c.n_nu:
                    assert idx in centres
                    hit += 1
    assert hit >= 9
    t = c.reference()["t"]
    lo, hi = t.lo[c.probe], t.hi[c.probe]
    # such a line's window holds a whole tile that is far from it: the far role has work
    far_tiles = 0
    for l in range(lo.shape[0]):
        ci = T.centre_index(c.nus, c.line_nus[c.probe][l])
        for tile, (a, b) in enumerate(fr):
            far_tiles += int((ci < a or ci > b) and lo[l, 0] <= tile * T.TILE and hi[l, 0] >= (tile + 1) * T.TILE)
    assert far_tiles > 20
    # window edges on a tile's first / last point, one beside, and inside a tile
    assert {256, 257, 255, 384} <= set(lo.reshape(-1).tolist()) and {1792, 1793, 1791, 1664} <= set(hi.reshape(-1).tolist())
    if jump:  # the sixteen probes around the smooth-grid guess miss the bound: lane 0 searches
        for tile in (3, 4):
            guess = tile * T.TILE - (5 * (T.TILE - 1)) // 2
            assert not (guess - 8 <= fr[tile][0] - 1 < guess + 8)


@pytest.mark.parametrize("kind,n", [(1, 1), (63, 63), (64, 64), (65, 65)])
def test_sparse_lists_have_their_lengths(kind, n):
    assert T.case(f"sparse_{kind}").n_lines == n


def test_sparse_lists_leave_tiles_empty():
    c = T.case("sparse_one_tile")
    assert set((T.centre_index(c.nus, c.line_nus) // T.TILE).tolist()) == {4}
    c = T.case("sparse_alternate_tiles")
    plane = c.reference()["t"].plane
    for tile in range(8):
        assert np.any(plane[:, tile * T.TILE:(tile + 1) * T.TILE] != 0) == (tile % 2 == 0)


@pytest.mark.parametrize("name", T.WALKS)
def test_walk_shapes_meet_the_rule_of_the_launch(name):
    """line_partials (stardis_hip.hip): F = 2 from 16384 points and F = 4 from 32768 where 2 n_lines >= n_nu; the subsets form where
    2 n_lines >= 8 n_nu on an indexed list (>= 8192 lines) with four line subsets (choose_splits: from 640 (tile, depth) pairs on)"""
    c = T.case(name)
    dense = 2 * c.n_lines >= c.n_nu
    tiles = -(-c.n_nu // T.TILE)
    splits = min(max(4, -(-2560 // (tiles * c.n_depth))), -(-c.n_lines // 64), 8)
    sub = 2 * c.n_lines >= 8 * c.n_nu and splits == 4
    f = 4 if sub else ((4 if c.n_nu >= 32768 else 2 if c.n_nu >= 16384 else 1) if dense else 1)
    assert (f, sub) == dict(walk_f2=(2, False), walk_f4=(4, False), walk_sub=(4, True))[name]
    assert c.n_lines >= 8192  # the default of indexed_min_lines
    idx = np.flatnonzero(c.probe)
    for j, hw in c.notes["where"]:
        assert c.probe[j] and np.all(c.hw[j] == hw)
    run = np.arange(c.notes["run_at"], c.notes["run_at"] + c.notes["K"])
    assert c.probe[run[0]] and np.all(c.line_nus[run] == c.line_nus[run[0]]) and idx.size == len(c.notes["where"]) + c.probe[run].sum()
    assert (run[0] // 64) != (run[-1] // 64)  # the run crosses a 64-line stretch


@pytest.mark.parametrize("name", ["class_edges", "grid_ends", "far_edges", "coincident_64_wide", "pile_up_wide"])
def test_the_judgement_notices_one_missing_or_doubled_term(name):
    """judge() passes the oracle's own plane, and fails it with the weakest term of a probe line taken out, or added twice, at one point"""
    c = T.case(name)
    r = c.reference()
    t = r["t"]
    T.judge(c, r["oracle"], False)
    with np.errstate(all="ignore"):
        share = np.where((t.probe_terms > 0) & r["tight"][None], t.probe_terms / t.plane[None], np.inf)
    p, d, i = np.unravel_index(np.argmin(share), share.shape)
    assert T.VISIBLE <= share[p, d, i] < np.inf
    for sign in (-1.0, 1.0):
        bad = r["oracle"].copy()
        bad[d, i] = float(bad[d, i] + sign * t.probe_terms[p, d, i])
        with pytest.raises(AssertionError):
            T.judge(c, bad, True)
