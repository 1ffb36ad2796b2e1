// sdx_line_geom.h — how a block index of the line launch (k_line_all, k_line_listed, k_line_all_mixed; sdx_kernels.h) becomes a unit
// of work, stated ONCE: the host (stardis_hip.hip) forms a LineGeom per launch from the shard and the grid, the kernels
// decode their block index with the two functions below, and the host-side test runs the same functions over every block index.
// (The kernels with a far field keep decoding the host's four words themselves — LineWords, sdx_kernels.h, which says why — on the same
// grid: line_launch_make counts their far workgroups, which come first.)
// Free of HIP: plain C++17, constexpr on host and device, so that a stand-alone host program can include it.
//
// Everything a wave derived per launch constant — four 64-bit divisions in the narrow role, two emulated 32-bit ones and the tile-prefix
// loop in the wide role, the decode of the `roles` word — is formed here on the host.  What is left per wave is one multiply-high division
// in the wide role (block -> depth, position) and one in the narrow role, and that only with more than one depth chunk (n_depth > 64).
//
// RANGE.  Every index is a non-negative int: line_launch_make() refuses (ok = false) a launch whose grid, narrow units or last frequency
// index do not stay below 2^31 - 512 (the surplus workgroups of the last round form indices past the last unit before they are
// compared), and line_div is exact for every dividend 0 <= n < 2^31 and every divisor 1 <= d < 2^31.
//
// SIZE.  The struct is 18 dwords of kernel arguments (and four of holes), each read where its role begins and nowhere else: a line kernel starts with
// more scalar arguments than it has scalar registers, and every further word that stays live is a spill lane.  Hence no word that a
// wave can form with one instruction (tiles / 8, tiles % 8), and no role mask: a role that is
// switched off has no live unit (tiles = 0, n_narrow = 0) while its workgroups stay in the grid.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SDX_GEOM_FN __host__ __device__ __forceinline__ constexpr
#else
#define SDX_GEOM_FN inline constexpr
#endif

// n / d by one 32 x 32 -> 64 bit multiplication and a shift: mul = ceil(2^shift / d), shift = 31 + ceil(log2 d).  With
// mul d = 2^shift + e, 0 <= e < d <= 2^(shift - 31): n mul / 2^shift = n / d + n e / (d 2^shift), and n e < 2^31 2^(shift - 31) = 2^shift
// keeps the excess below 1 / d — the floor is that of n / d for every 0 <= n < 2^31.  mul < 2^32 because d > 2^(shift - 32).
struct LineDiv {
    uint32_t mul;
    int32_t shift;
};
constexpr int64_t kLineIndexBound = ((int64_t)1 << 31) - 512;  // grids, units and frequency indices of a launch stay below this
SDX_GEOM_FN LineDiv line_div_make(int d)
{
    int l = 0;
    while (((int64_t)1 << l) < (int64_t)d) ++l;
    return LineDiv{(uint32_t)((((uint64_t)1 << (31 + l)) + (uint64_t)d - 1) / (uint64_t)d), 31 + l};
}
SDX_GEOM_FN int line_div(int n, LineDiv v) { return (int)(((uint64_t)(uint32_t)n * v.mul) >> v.shift); }

constexpr int kLineRoleWide = 1, kLineRoleNarrow = 2;  // line_launch_make's mask (one at a time: split-launch profiling, SDX_SPLIT_LAUNCHES)
constexpr int kNarrowGroupPlain = 4, kNarrowGroupSubsets = 16;  // consecutive narrow workgroups' worth of frequencies that share an XCD

// The grid: [0, wide_first) the far role's workgroups, if any; [wide_first, narrow_first) wide role; [narrow_first, ...) narrow role.
// (The holes keep the words of one role from being loaded, and spilled, together with another's.)
struct LineGeom {
    int narrow_first;
    int hole0_[3];
    // wide role: block - wide_first = depth * tiles_pad + p; p -> tile by the XCD-aware order.  wide_group 0: XCD x = p % 8 takes the
    // contiguous tiles [prefix(x), prefix(x + 1)), prefix(x) = x (tiles / 8) + min(x, tiles % 8) — the closed form of
    // sum_{f < x} ceil((tiles - f) / 8).  wide_group g > 0: groups of g tiles going round the XCDs, tiles_pad = the tiles rounded up to
    // whole rounds of 8 g (surplus workgroups are not live).  tiles = 0: the role is switched off.
    int wide_first, tiles, tiles_pad, wide_group;
    LineDiv by_tiles_pad, by_wide_group;
    int hole_;
    // narrow role: unit c = chunk * n_grp + r is the group of F = 1 << f_shift frequencies from (g0 + r) F on, depth chunk `chunk` (64
    // depths each); n_narrow units (0: the role is switched off), n_split waves of a workgroup with a unit each, or — subsets — one unit
    // per workgroup; n_nb8: workgroups per XCD of order 2
    int f_shift, g0, n_grp, n_narrow, n_split, order, n_nb8;
    LineDiv by_grp;
};

struct LineLaunch {
    LineGeom g;
    int64_t blocks;  // workgroups of the launch
    bool ok;         // false: beyond the range stated above — nothing is launched
};

// nu_begin, nu_count: the shard's columns; tile_points: 64 R; narrow_f in {1, 2, 4}; subsets: the narrow role of the SUBSETS kernels;
// wide_group 0 .. 15; order 0 grouped, 1 plain, 2 one block per XCD (the host passes 0 for both: the other orders were measured and lost,
// and stay only because the kernels spill more scalar registers without them — LineWords, sdx_kernels.h); far_blocks: the workgroups of
// the far role, first in the grid.
SDX_GEOM_FN LineLaunch line_launch_make(int64_t nu_begin, int64_t nu_count, int n_depth, int n_split, int tile_points, int narrow_f, bool subsets,
                                        int wide_group, int order, int mask, int64_t far_blocks)
{
    LineLaunch L{};
    LineGeom& g = L.g;
    const int64_t nu_end = nu_begin + nu_count;
    const int64_t tiles = (nu_end + tile_points - 1) / tile_points - nu_begin / tile_points;
    const int64_t round = wide_group ? 8 * (int64_t)wide_group : 1;
    const int64_t tiles_pad = (tiles + round - 1) / round * round;
    const int64_t n_wide = tiles_pad * n_depth;
    const int64_t g0 = nu_begin / narrow_f, n_grp = (nu_end + narrow_f - 1) / narrow_f - g0;
    const int64_t n_chunks = (n_depth + 63) / 64;
    const int64_t n_narrow = n_grp * n_chunks;
    const int64_t n_nb = subsets ? n_narrow : (n_narrow + n_split - 1) / n_split;
    // whole rounds of the XCD-aware order: 8 XCDs x groups of 4 workgroups, 16 in the subsets kernel (surplus workgroups are not live)
    const int64_t narrow_round = 8 * (subsets ? kNarrowGroupSubsets : kNarrowGroupPlain);
    const int64_t narrow_blocks = (n_nb + narrow_round - 1) / narrow_round * narrow_round;
    const int64_t n_far = far_blocks;
    L.blocks = n_far + n_wide + narrow_blocks;
    L.ok = nu_begin >= 0 && nu_count >= 0 && n_depth > 0 && n_split > 0 && n_split <= 8 && (narrow_f == 1 || narrow_f == 2 || narrow_f == 4) && tiles_pad >= 1 &&
           n_grp >= 1 && far_blocks >= 0 && nu_end < kLineIndexBound && n_narrow < kLineIndexBound && L.blocks < kLineIndexBound;
    if (!L.ok) return L;
    g.wide_first = (int)n_far;
    g.narrow_first = (int)(n_far + n_wide), g.tiles = (mask & kLineRoleWide) ? (int)tiles : 0, g.tiles_pad = (int)tiles_pad;
    g.wide_group = wide_group;
    g.by_tiles_pad = line_div_make((int)tiles_pad), g.by_wide_group = line_div_make(wide_group ? wide_group : 1);
    g.f_shift = narrow_f == 4 ? 2 : (narrow_f == 2 ? 1 : 0);
    g.g0 = (int)g0, g.n_grp = (int)n_grp, g.n_narrow = (mask & kLineRoleNarrow) ? (int)n_narrow : 0, g.n_nb8 = (int)((n_nb + 7) / 8);
    g.n_split = n_split, g.order = order;
    g.by_grp = line_div_make((int)n_grp);
    return L;
}

struct WideUnit {
    int tile, depth;
    bool live;
};
struct NarrowUnit {
    int i0, chunk;  // first frequency (global index) of the wave's group, depth chunk
    bool live;
};

// g.wide_first <= block < g.narrow_first
SDX_GEOM_FN WideUnit wide_unit(const LineGeom& g, int block)
{
    const int b = block - g.wide_first;
    const int d = line_div(b, g.by_tiles_pad), p = b - d * g.tiles_pad;
    const int x = p & 7, j = p >> 3;
    int tile = 0;
    if (g.wide_group == 0) {
        const int q = g.tiles >> 3, r = g.tiles & 7;
        tile = j + x * q + (x < r ? x : r);
    } else {
        const int jq = line_div(j, g.by_wide_group);
        tile = (jq * 8 + x) * g.wide_group + (j - jq * g.wide_group);
    }
    return WideUnit{tile, d, tile < g.tiles};
}

// g.narrow_first <= block; wave < g.n_split.  Only a unit past the first depth chunk (n_depth > 64) executes a division.
template <bool SUBSETS>
SDX_GEOM_FN NarrowUnit narrow_unit(const LineGeom& g, int block, int wave)
{
    constexpr int G = SUBSETS ? kNarrowGroupSubsets : kNarrowGroupPlain;
    const int p = block - g.narrow_first, j = p >> 3;
    // (workgroups p, p + 8, ... share an XCD: they take groups of G consecutive workgroups' worth of frequencies, the groups going round the XCDs)
    int wg = ((j / G) * 8 + (p & 7)) * G + j % G;
    if (g.order == 1) wg = p;
    if (g.order == 2) wg = j < g.n_nb8 ? (p & 7) * g.n_nb8 + j : g.n_narrow;
    // (a workgroup past the last one forms c >= n_narrow: the workgroups hold ceil(n_narrow / n_split) n_split >= n_narrow units)
    const int c = SUBSETS ? wg : wg * g.n_split + wave;
    if (c >= g.n_narrow) return NarrowUnit{0, 0, false};  // (subsets: the whole workgroup)
    int chunk = 0, r = c;
    if (c >= g.n_grp) {
        chunk = line_div(c, g.by_grp);
        r = c - chunk * g.n_grp;
    }
    return NarrowUnit{(g.g0 + r) << g.f_shift, chunk, true};
}

// ---- what the kernels rely on, at the edges of the stated range and at a few launches ---------------------------------------------
namespace line_geom_checks {
constexpr bool div_ok(int n, int d) { return line_div(n, line_div_make(d)) == n / d; }
constexpr int kMax = 2147483647;
static_assert(div_ok(0, 1) && div_ok(kMax, 1) && div_ok(kMax, 2) && div_ok(kMax, 3) && div_ok(kMax, kMax) && div_ok(kMax - 1, kMax), "line_div");
static_assert(div_ok(kMax, 65535) && div_ok(kMax, 65537) && div_ok(kMax, 1 << 30) && div_ok(kMax, (1 << 30) + 1) && div_ok(kMax - 6, 7), "line_div");
static_assert(div_ok(3 * 715827882 - 1, 715827882) && div_ok(3 * 715827882, 715827882), "line_div");
// S-c2 (7634 frequencies, 56 depths, two subsets): 30 tiles a depth, 3817 narrow workgroups in 3840, no division in the narrow role
constexpr LineLaunch kSc2 = line_launch_make(0, 7634, 56, 2, 256, 1, false, 0, 0, 3, 0);
static_assert(kSc2.ok && kSc2.g.narrow_first == 30 * 56 && kSc2.blocks == 30 * 56 + 3840 && kSc2.g.n_narrow == kSc2.g.n_grp, "S-c2");
static_assert(wide_unit(kSc2.g, 0).tile == 0 && wide_unit(kSc2.g, 1).tile == 4 && wide_unit(kSc2.g, 8).tile == 1 && wide_unit(kSc2.g, 31).depth == 1, "S-c2");
static_assert(narrow_unit<false>(kSc2.g, 30 * 56 + 1, 1).i0 == 9 && !narrow_unit<false>(kSc2.g, 30 * 56 + 3839, 0).live, "S-c2");
static_assert(!line_launch_make(0, (int64_t)1 << 31, 56, 2, 256, 1, false, 0, 0, 3, 0).ok, "range");
}  // namespace line_geom_checks
