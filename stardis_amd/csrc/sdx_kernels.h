// sdx_kernels.h — HIP kernels of the STARDIS hot path for gfx950.  Included once by stardis_hip.hip.
//
// Data layout in HBM (DESIGN.md section 3 has the table)
//   inputs   reference layout: line arrays [N_l][N_d] (doppler, alpha, gamma[N_l][N_d|1]), grid nus[N_nu] descending.
//   pre-pass WIDE items (half-width > 64 points) depth-major [N_d][N_l], split by use: scan words 16 B, records 48 B, slow part
//            16 B (+ 32 B fp32 records in the mixed mode); NARROW items line-major [N_l][N_d]: a one-byte half-width and three
//            f64 (1 / doppler, y, amplitude) — struct LineWork below.
//   outputs  [N_d][ld] with the frequency index contiguous.
#pragma once
#include <type_traits>

#include "sdx_math.h"
#include "sdx_broadening.h"
#include "sdx_cheb.h"
#include "sdx_rt_layout.h"
#include "sdx_line_geom.h"

namespace sdx {

constexpr int kBlock = 256;

__device__ __forceinline__ void wave_sync()
{
    // LDS hand-over between lanes of ONE wave: the LDS unit executes a wave's instructions in order, so only the
    // compiler has to be kept from moving accesses across this point
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}


// ------------------------------------------------------------------------------------------------
// d_nu = -max(diff(nus))  (opacities_solvers/base.py:524-526): partial maxima, finished by consumers.
constexpr int kDnuPartials = 256;
// ... and, 4096 bytes behind the partial maxima, a SAMPLE of the grid: kGridSample frequencies at a stride of ceil(N_nu / kGridSample)
// points, written by the launch that computes the partial maxima and read — 16 contiguous KB — by every pre-pass block that
// looks for line centres (a block sampling the grid itself touches one 64-byte line per sample)
constexpr int kGridSample = 2048;
constexpr int kGridSampleOffset = 512;  // doubles
__device__ __forceinline__ void grid_sample_block(const int bid, const int n_blocks, int64_t n_nu, const double* __restrict__ nus, double* __restrict__ sample)
{
    const int64_t cstride = (n_nu + kGridSample - 1) / kGridSample;
    for (int q = bid * (int)blockDim.x + (int)threadIdx.x; q < kGridSample; q += n_blocks * (int)blockDim.x) {
        const int64_t j = (int64_t)q * cstride;
        sample[q] = j < n_nu ? nus[j] : -INFINITY;
    }
}

__device__ __forceinline__ void shard_range(int64_t n_nu, const double* __restrict__ nus, int64_t n_lines, const double* __restrict__ line_nus,
                                            int64_t nu_begin, int64_t nu_count, int* __restrict__ sel);

// ---- far field of the line opacity: the per-tile index ranges (the commentary is at far_eligible, below) ------------------------
constexpr double kFarRatio = 6.0;
constexpr int kFarTile = 256;  // the far field lives on the 256-point tiles of the fp64 line kernel (R = 4)
struct FarReq {
    int* range;            // [2 T], [2 T + 1] per GLOBAL tile T
    int64_t first, count;  // the tiles wanted (count = 0: none)
};
// centre and half-width of a tile from its end frequencies (exact halvings of one rounded sum / difference each)
__device__ __forceinline__ void far_tile_geometry(double nu_a, double nu_b, double& c, double& h)
{
    c = mul_rn(0.5, add_rn(nu_a, nu_b));
    h = mul_rn(0.5, sub_rn(nu_a, nu_b));
}
// first i in [lo, hi] with nus[i] < v (hi if none) on the descending grid
__device__ __forceinline__ int64_t first_below(const double* __restrict__ nus, int64_t lo, int64_t hi, double v)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (nus[mid] >= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// Sixteen lanes per (tile, bound).  On a smooth grid the bound lies 2.5 tile widths beyond the tile's end, at an offset the tile's own
// mean spacing predicts to a few points: the lanes probe the sixteen grid points around that guess — ONE round trip behind the two
// loads of the tile's ends — and the count of frequencies >= the bound follows from their ballot.  Where the crossing is not among
// them (the spacing jumps), lane 0 searches: a bracket of eight tiles on that side first, then the rest of the grid.
__device__ __forceinline__ void far_ranges_block(const int bid, const int n_blocks, int64_t n_nu, const double* __restrict__ nus, const FarReq& fr)
{
    const int lane = threadIdx.x & 63, sub = lane & 15, grp_shift = lane & 48;
    const int64_t groups = (int64_t)n_blocks * (blockDim.x >> 4);
    for (int64_t k0 = (int64_t)bid * (blockDim.x >> 4); k0 < 2 * fr.count; k0 += groups) {  // (uniform trip count per block)
        const int64_t k = k0 + (threadIdx.x >> 4);
        const bool live = k < 2 * fr.count;
        const int64_t T = fr.first + (live ? k >> 1 : 0), i0 = T * kFarTile;
        const bool upper = (k & 1) == 0;
        int out = upper ? 0 : 0x7FFFFFFF;
        bool search = false;
        double v = 0.0;
        int64_t guess = 0;
        if (live && i0 + kFarTile <= n_nu) {
            double c, h;
            far_tile_geometry(nus[i0], nus[i0 + kFarTile - 1], c, h);
            if (h > 0.0) {
                search = true;
                v = upper ? add_rn(c, mul_rn(kFarRatio, h)) : sub_rn(c, mul_rn(kFarRatio, h));
                // (c +- 6 h lies 5 h beyond the tile's end: 5 / 2 * (kFarTile - 1) points at the tile's mean spacing)
                guess = upper ? i0 - (5 * (kFarTile - 1)) / 2 : i0 + kFarTile - 1 + (5 * (kFarTile - 1)) / 2;
            }
        }
        // the probes: grid points guess - 8 + sub (outside the grid: +inf above, -inf below, so that the ballot stays monotone)
        const int64_t pi = guess - 8 + sub;
        const double pv = !search ? 0.0 : (pi < 0 ? INFINITY : (pi >= n_nu ? -INFINITY : nus[pi]));
        const unsigned long long ge = __ballot(search && pv >= v);
        const unsigned m16 = (unsigned)(ge >> grp_shift) & 0xFFFFu;  // this group's sixteen answers (bit j: probe j >= v)
        if (search) {
            if ((m16 & 1u) && !(m16 & 0x8000u)) {
                out = (int)(guess - 8 + __popc(m16));  // = #{i : nus[i] >= v}: every point before the window is >= v as well
            } else if (sub == 0) {
                if (upper) {
                    const int64_t b0 = max(i0 - 8 * kFarTile, (int64_t)0);
                    out = (int)((b0 == 0 || nus[b0 - 1] >= v) ? first_below(nus, b0, i0, v) : first_below(nus, 0, b0 - 1, v));
                } else {
                    const int64_t b1 = min(i0 + 9 * kFarTile, n_nu);
                    out = (int)((b1 == n_nu || nus[b1] < v) ? first_below(nus, i0 + kFarTile, b1, v) : first_below(nus, b1 + 1, n_nu, v));
                }
            }
        }
        if (live && sub == 0) fr.range[2 * T + (upper ? 0 : 1)] = out;
    }
}
__global__ __launch_bounds__(kBlock) void k_far_ranges(int64_t n_nu, const double* __restrict__ nus, FarReq fr)
{
    far_ranges_block(blockIdx.x, gridDim.x, n_nu, nus, fr);
}


__global__ __launch_bounds__(kBlock) void k_dnu_partial(int64_t n_nu, const double* __restrict__ nus,
                                                        double* __restrict__ partial, int* __restrict__ zero, int64_t n_zero, FarReq far)
{
    far_ranges_block(blockIdx.x, gridDim.x, n_nu, nus, far);
    // (culled pre-pass: the per-line maxima the classification pass accumulates into are cleared here, not by a memset node)
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n_zero; k += (int64_t)gridDim.x * kBlock) zero[k] = 0;
    grid_sample_block(blockIdx.x, gridDim.x, n_nu, nus, partial + kGridSampleOffset);
    double m = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i + 1 < n_nu; i += (int64_t)gridDim.x * kBlock)
        m = fmax(m, nus[i + 1] - nus[i]);
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    __shared__ double s[kBlock / 64];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) m = fmax(m, s[w]);
        partial[blockIdx.x] = m;
    }
}

__device__ __forceinline__ double block_dnu(const double* __restrict__ partial, int n_partial, double* s_red)
{
    double m = -INFINITY;
    for (int i = threadIdx.x; i < n_partial; i += blockDim.x) m = fmax(m, partial[i]);
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s_red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, s_red[w]);
    __syncthreads();
    return -m;
}

// this thread's share of max(diff(nus)) — eight independent loads in flight per thread: the scan is latency-, not
// bandwidth-bound (the grid sits in L2).  Issued EARLY by the pre-pass so that it overlaps the centre search.
__device__ __forceinline__ double dnu_scan_local(const double* __restrict__ nus, int64_t n_nu)
{
    double m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
    const int64_t step = blockDim.x;
    int64_t i = threadIdx.x;
    for (; i + 3 * step + 1 < n_nu; i += 4 * step) {
        const double a0 = nus[i], b0 = nus[i + 1], a1 = nus[i + step], b1 = nus[i + step + 1];
        const double a2 = nus[i + 2 * step], b2 = nus[i + 2 * step + 1], a3 = nus[i + 3 * step], b3 = nus[i + 3 * step + 1];
        m0 = fmax(m0, b0 - a0);
        m1 = fmax(m1, b1 - a1);
        m2 = fmax(m2, b2 - a2);
        m3 = fmax(m3, b3 - a3);
    }
    for (; i + 1 < n_nu; i += step) m0 = fmax(m0, nus[i + 1] - nus[i]);
    return fmax(fmax(m0, m1), fmax(m2, m3));
}
__device__ __forceinline__ double block_max_to_dnu(double m, double* s_red)
{
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s_red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, s_red[w]);
    __syncthreads();
    return -m;
}
__device__ __forceinline__ double block_dnu_scan(const double* __restrict__ nus, int64_t n_nu, double* s_red)
{
    return block_max_to_dnu(dnu_scan_local(nus, n_nu), s_red);
}

// index of the first grid frequency strictly below line_nu in the DESCENDING grid
//   = N_nu - searchsorted(nus[::-1], line_nu)   (base.py:556-558)
__device__ __forceinline__ double recip_guarded(double d)
{
    // Newton-refined hardware reciprocal for ordinary magnitudes, IEEE division otherwise (0, inf, NaN, subnormal)
    return (d > 1e-290 && d < 1e290) ? recip(d) : 1.0 / d;
}
constexpr double kInvSqrtPiPi = 0x1.6fcb5f827b97fp-3;  // 1 / (sqrt(pi) pi), correctly rounded
// 1 / dw, y and the amplitude of a (line, depth) item from its doppler width, gamma and alpha (voigt.py:148-149, base.py:627) — what the
// pre-pass stores in a narrow record, and what the narrow role forms itself when it reads the raw inputs (LineWork::narrow_raw)
__device__ __forceinline__ void narrow_params(double dw, double g, double a, double& inv, double& y, double& amp)
{
    inv = recip_guarded(dw);
    y = mul_rn(mul_rn(g, kInvSqrtPiPi), inv);
    amp = mul_rn(mul_rn(a, kInvSqrtPi), inv);
}
__device__ __forceinline__ int64_t closest_index(const double* __restrict__ nus, int64_t n_nu, double line_nu)
{
    int64_t lo = 0, hi = n_nu;  // first i with nus[i] < line_nu
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (nus[mid] >= line_nu) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// window rule base.py:561-575, bit-for-bit (each operation rounds once, same order)
// (the quotient by d_nu — one divisor for every item — through div_by: the correctly rounded quotient from 1 / d_nu, computed once)
__device__ __forceinline__ int64_t window_rule(int64_t c, int64_t n_nu, double d_nu, double r_dnu, double gamma, double dw, double alpha,
                                               int& lo, int& hi)
{
    const double pixels = mul_rn(div_by(mul_rn(add_rn(gamma, dw), alpha), d_nu, r_dnu), 20.0);
    const double forced = pixels > 10.0 ? pixels : 10.0;  // max(10, x); NaN keeps 10
    const int64_t hw = forced >= (double)n_nu ? n_nu : (int64_t)forced;  // int() truncates; saturating is equivalent
    const int64_t l = c - hw, h = c + hw;
    lo = (int)(l < 0 ? 0 : l);
    hi = (int)(h > n_nu ? n_nu : h);
    return hw;
}

// ------------------------------------------------------------------------------------------------
// Pre-pass: one block = kPreLines lines x up to 64 depths, 1024 threads, the (line, depth) items in registers (prepass_block).
// lines per pre-pass block — a template parameter: 16 (one item per thread) for short lists whose blocks all fit the chip at once,
// 32 (two items per thread: the block's latency chain is paid once for twice the items) for long ones, 48 / 54 (three) for the
// culled pre-pass of a frequency shard, whose blocks then fit ONE round of the chip
constexpr int kPreDepths = 64;
constexpr int kPreBlock = 1024;  // threads per pre-pass block: one (line, depth) item per thread, 16 waves to hide latency

constexpr int kNarrowHalfWidth = 64;    // windows with half-width <= this go to the narrow-window kernel
constexpr int kNarrowReach = 128;       // ... which looks for its lines within this many points of a frequency: line CORES up to this
                                        // half-width are delegated to it (lane <-> depth: one Faddeeva region per wave, where a
                                        // 64-point block of the wide role holds all four)
constexpr int kMediumHalfWidth = 4096;  // class bound of the indexed wide path: medium lines are found by centre range
constexpr int kMaxTile = 512;           // the widest tile of the wide role (64 R points, R <= 8)

// What the pre-pass leaves for the line kernels.  WIDE (line, depth) items (half-width > kNarrowHalfWidth) are depth-major
// [N_d][N_l] — a (depth, line-range) read is contiguous — and split by use:
//   wscan   16 B, read by every candidate test: window [lo, hi) and the CORE range [clo, chi), a superset of the grid points
//           where the Faddeeva region is not I (|x| + y <= 15); lo = hi = 0 for narrow / empty items
//   wrec    48 B, read once per (item, tile) that overlaps: line frequency, 1 / doppler and the region-I constants
//   wslow   16 B, read only by tiles that touch a window edge or the core: y and the amplitude (regions II-IV)
//   wrec32  32 B, the fp32 twin of wrec for the mixed-precision mode (line frequency as a hi + lo pair)
#ifdef SDX_WALK_STATS  // analysis build (scripts/r4/walk_stats.sh): what the waves of the line kernel spend their time on
constexpr int kWalkStatSlots = 1 << 19;  // lower half: wide waves by (depth < 64, tile < 512, subset < 8); upper half: narrow waves by frequency
__device__ unsigned long long g_walk_stats[(size_t)kWalkStatSlots * 8];
#endif
#ifdef SDX_PRE_STATS  // analysis build (scripts/r5/pre_stats.sh): when the phases of a pre-pass block begin (100 MHz device clock)
constexpr int kPreStatSlots = 1 << 14;
__device__ unsigned long long g_pre_stats[(size_t)kPreStatSlots * 8];
#define SDX_PRE_STAMP(n) do { if (tid == 0) pst[n] = wall_clock64(); } while (0)
#else
#define SDX_PRE_STAMP(n) do { } while (0)
#endif
struct alignas(16) WideScan {
    int lo, hi, clo, chi;
};
struct alignas(16) WideRec {
    double lnu, inv, yk, cv, cd, spare;
};
struct alignas(16) WideSlow {
    double y, amp;
};
struct alignas(32) WideRec32 {  // one s_load_dwordx8
    // ncl = -(lnu - nuh) * inv: the low part of the line frequency, already scaled.  Operands that meet in one instruction
    // share an aligned 8-byte pair (a VALU instruction reads one scalar register pair): (inv, ncl), (cv, cd), yk twice
    float nuh, yk, inv, ncl, cv, cd, pad0, pad1;
};
struct LineWork {
    WideScan* wscan;
    WideRec* wrec;
    WideSlow* wslow;
    WideRec32* wrec32;  // nullptr unless the mixed-precision mode is on
    // NARROW items (half-width <= kNarrowHalfWidth) and the delegated cores of wide items, LINE-major [N_l][N_d] so that
    // lane <-> depth reads coalesce.  Separate arrays: one 32-byte record per item was measured 45 % slower in the narrow
    // role (a wave's load then touches 28 cache lines three times over instead of 4 + 4 + 7 + 7 + 7)
    // half-width h of the narrow role's window [max(c - h, 0), min(c + h, N_nu)) around the line's centre c — a narrow item's
    // own half-width (<= kNarrowHalfWidth) or the delegated core's (<= kNarrowReach); 0: nothing to do for this (line, depth).
    // One byte instead of the two clamped bounds: the clamp is implied by the frequency index being a grid index.
    unsigned char* nhw;
    int skip_unlisted_scan;  // long lists, one depth block per line: wscan is written only for lines with a wide window somewhere
    double* n_inv;   // 1 / doppler
    double* n_y;
    double* n_amp;
    // narrow_raw != 0 (long dense lists, fp64; round 6): NO narrow records — n_inv / n_y / n_amp point at the CALLER'S doppler widths,
    // gammas and alphas (the same line-major layout; narrow_raw = the gammas' columns, 1 or N_d) and the narrow role forms 1 / dw, y and
    // the amplitude itself for the items it evaluates (narrow_params: the pre-pass's own three operations, hence the same bits): the
    // pre-pass writes one byte per narrow item instead of 25 — 1.35 of its 1.67 GB at 1e6 lines
    int narrow_raw;
    // mixed-precision mode: the narrow role evaluates in fp32 — the same three arrays as floats, and the line frequencies
    // as hi + lo float pairs [N_l]
    float* n_inv32;
    float* n_y32;
    float* n_amp32;
    float2v* lnu32;
    int* cnt_ge;     // [N_nu + 2]: number of lines whose centre index is >= p (lines are a prefix: centres descend)
    int* centre;     // [N_l] centre index of each line
    int* nhw_max;    // [N_l] largest NARROW half-width of the line over all depths (0: no narrow item)
    int* whw_max;    // [N_l] largest WIDE half-width of the line over all depths (0: no wide item)
    // long line lists: ascending indices of the lines whose widest window exceeds kMediumHalfWidth (they may reach any tile and
    // are scanned completely; all other lines are found by centre range).  nullptr for short lists (every line is scanned, or — n_csplit, below — every line with a wide window somewhere).
    int* hlist;
    int* hcount;     // [0] entries of hlist, [1] entries of wlist, [2] entries of xlist
    // frequency shards of long lists: the lines with a wide window whose centre lies within kMediumHalfWidth of the shard's
    // columns but outside the blocks of consecutive lines the shard prepares anyway (centres within 2 kNarrowReach) — with
    // hlist the lines the gather blocks of a culled pre-pass prepare.  nullptr otherwise.
    int* xlist;
    // ... and the other lines with a wide window (kNarrowHalfWidth < widest window <= kMediumHalfWidth), ascending, with
    // wrank[l] = number of wlist entries below line l ([N_l + 1]): the lines centred near a tile are a contiguous range of
    // line indices (cnt_ge), hence a contiguous range [wrank[la], wrank[lb]) of wlist
    int* wlist;
    int* wrank;
    WideScan* hscan;  // [N_d][N_l] rows, entry k of row d = wscan[d][hlist[k]]: the huge lines' scan words, contiguous
    // (list-ordered copies of the huge lines' RECORDS and of the wlist scan words as well were measured in round 3: the wide
    // role fetches 0.36 GB per launch at 1e6 lines either way — its 16 GB were the narrow role's — and the copies cost more
    // than the walk gained; removed)
    // frequency-sharded runs of long lists: the pre-pass only has to prepare the lines this shard can touch.  sel (device
    // memory, written on the side of k_dnu_partial; nullptr: every line): [0..1] = the index range [la, lb) of the lines whose
    // centre lies within kMediumHalfWidth of the shard's columns — the only ones a medium window can reach it from;
    // [2..3] = [na, nb), those within 2 kNarrowReach — every line there may touch the shard (narrow windows, delegated
    // cores) and is prepared by the range blocks; outside [na, nb) only lines with a wide window matter: hlist (any distance)
    // and xlist (within [la, lb)), prepared by the gather blocks
    const int* sel;
    int n_pix;      // pixel blocks (cnt_ge) behind the line blocks of the pre-pass grid
    int gather;     // gather blocks behind those: block g prepares hlist[g kPreLines ...] (0: none)
    int64_t shard_begin, shard_end;  // the shard's columns (culled runs only need cnt_ge near them)
    unsigned long long* evals;
    int* ticket;  // culled runs: the pre-pass launch's work counter, one per depth block (zeroed by k_hlist_count), or nullptr
    int front;    // culled runs: the blocks with work are the FIRST blocks of the pre-pass grid (k_line_prepass maps its block index)
    // SHORT lists (no hlist), full pre-pass, n_csplit > 0: the lines with a wide window at any depth (whw_max > 0), ascending, one
    // list per line subset s < n_csplit of the wide role (chunk q of 64 consecutive line indices belongs to subset q % n_csplit) — the
    // set and the order in which subset s meets its possible hits when it scans every line.  The lists lie one behind the other where
    // long lists keep hlist (wide_list_of), their entries and offsets where the list launches keep their block counts
    // (wide_list_counts: [s] entries, [8 + s] offset).  Written by the LAST line block of the pre-pass launch to finish
    // (compact_wide_lines); `ticket` then counts the finished line blocks and is left at zero.  0: the wide role scans the whole list.
    // (no pointers of their own: a larger LineWork made every launch that takes one slower, list or no list)
    int n_csplit;
    // far field (line_far_body): the (line, depth, tile) triples that far_eligible() accepts are left to the far role — the wide role
    // skips them — and their sum reaches the grid through the tile's 16 Chebyshev nodes (a third plane).
    // far_range[2 T], [2 T + 1] (k_far_ranges): a line is far from global tile T when its centre index is < the first or > the second
    // (0 and INT_MAX: tile T has no far field); nullptr = no far field in this launch
    const int* far_range;
};

__device__ __forceinline__ int* wide_list_of(const LineWork& w, int64_t n_lines) { return w.whw_max + n_lines; }
__device__ __forceinline__ int* wide_list_counts(const LineWork& w) { return w.hcount + 16; }

// k / d for 0 <= k < 65536 and 1 <= d < 65536 with the divisor's reciprocal m = small_div_magic(d) = ceil(2^32 / d): one multiply-high
// instead of the ~30 instructions of a 32-bit division by a run-time value (the pre-pass indexes its (line, depth) items six times)
__host__ __device__ __forceinline__ unsigned small_div_magic(int d) { return d > 1 ? 0xFFFFFFFFu / (unsigned)d + 1u : 0u; }
__device__ __forceinline__ int small_div(int k, unsigned magic) { return magic ? (int)__umulhi((unsigned)k, magic) : k; }

// Short lists: the wide role's candidates, compacted per line subset (LineWork::n_csplit).  Run by ONE block, the last line block of
// the pre-pass launch to finish, behind the agent-scope acquire of its ticket: whw_max is complete.  Chunk q (the 64 lines a wave
// reads with one load) belongs to subset q % n_split; its wide lines go, in ascending order, behind those of the subset's earlier
// chunks.  The masks of all chunks meet in LDS (the grid sample's 16 KB, free by now): one load per line, two barriers.
constexpr int kListMaxChunks = kGridSample - 8;  // 64-bit masks in the sample's array, the subset totals behind them
__device__ __forceinline__ void compact_wide_lines(const LineWork& w, const int64_t n_lines, unsigned long long* __restrict__ s_mask, const int tid)
{
    const int n_split = w.n_csplit;
    const int n_chunks = (int)((n_lines + 63) >> 6);
    const int wave = tid >> 6, lane = tid & 63;
    int* const s_tot = reinterpret_cast<int*>(s_mask + kListMaxChunks);
    int* const clist = wide_list_of(w, n_lines);
    int* const ccount = wide_list_counts(w);
    for (int q = wave; q < n_chunks; q += kPreBlock / 64) {
        const int64_t l = (int64_t)q * 64 + lane;
        const unsigned long long m = __ballot(l < n_lines && w.whw_max[l] > 0);
        if (lane == 0) s_mask[q] = m;
    }
    __syncthreads();
    // wide lines of subset s in the chunks below q (lanes share the subset's earlier chunks)
    auto below = [&](int s, int q) {
        int c = 0;
        for (int j = lane; s + j * n_split < q; j += 64) c += __popcll(s_mask[s + j * n_split]);
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
        return c;
    };
    if (wave < n_split) {
        const int t = below(wave, n_chunks);
        if (lane == 0) s_tot[wave] = t;
    }
    __syncthreads();
    for (int q = wave; q < n_chunks; q += kPreBlock / 64) {
        const int s = q % n_split;
        int base = below(s, q);
        for (int k = 0; k < s; ++k) base += s_tot[k];
        const unsigned long long m = s_mask[q];
        if ((m >> lane) & 1)
            clist[base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = q * 64 + lane;
    }
    if (tid < n_split) {
        int off = 0;
        for (int k = 0; k < tid; ++k) off += s_tot[k];
        ccount[tid] = s_tot[tid];
        ccount[8 + tid] = off;
    }
}

// PLANNED (sdx_grid_plan, include/stardis_hip.h): what depends on the grid and the line frequencies alone was formed once, by
// k_grid_plan_build — a planned line block stages no grid sample, searches no centre and scans no spacing: `dnu_partial` is then the
// plan's array of doubles ([0] = d_nu, [1] = 1 / d_nu), w.centre and w.cnt_ge point into the plan, the launch has no pixel blocks, and
// the block's chain is ONE round trip (centres, the two scalars, the dense inputs) and one barrier in front of the arithmetic.
constexpr int kPlanFreqOffset = 8;  // doubles: the per-frequency planes of a plan lie behind its scalars
template <bool GEN, int kPreLines, bool LIST = true, bool PLANNED = false>
__device__ __forceinline__ void prepass_block(const int bx, const int by, const int gy, int n_depth, int64_t n_nu, const double* __restrict__ nus,
                                                         const double* __restrict__ dnu_partial, int n_partial,
                                                         int64_t n_lines, const double* __restrict__ line_nus,
                                                         const double* __restrict__ doppler,
                                                         const double* __restrict__ gammas, int gamma_cols,
                                                         const double* __restrict__ alphas, LineWork w,
                                                         int* __restrict__ out_lo_ref, int* __restrict__ out_hi_ref,
                                                         int n_line_blocks, const LineParams& lp, const int tid = threadIdx.x)
{
    int gbx = -1;  // >= 0: a gather block
    if (bx >= n_line_blocks) {
        if (bx >= n_line_blocks + w.n_pix) {
            if (!w.gather) return;
            gbx = bx - n_line_blocks - w.n_pix;
        } else {
            // pixel blocks: cnt_ge[p] = #{l : centre_l >= p} = #{l : line_nu_l <= nus[p-1]}  (centre_l = #{i : nus[i] >= line_nu_l})
            if (by == 0 && w.cnt_ge) {
                const int64_t pidx = (int64_t)(bx - n_line_blocks) * blockDim.x + tid;
                // a shard only reads cnt_ge within kMediumHalfWidth (+ a narrow window) of the TILES that hold its columns: tiles
                // are aligned to the global grid, so the first and last one reach up to kMaxTile - 1 points beyond the shard
                const bool needed = !w.sel || (pidx >= w.shard_begin - kMediumHalfWidth - 2 * kNarrowReach - kMaxTile &&
                                               pidx <= w.shard_end + kMediumHalfWidth + 2 * kNarrowReach + kMaxTile);
                if (pidx <= n_nu + 1 && needed) {
                    int64_t cnt;
                    if (pidx == 0) cnt = n_lines;
                    else if (pidx == n_nu + 1) cnt = 0;
                    else {
                        const double v = nus[pidx - 1];
                        int64_t lo = 0, hi = n_lines;  // first l with line_nus[l] > v
                        while (lo < hi) {
                            const int64_t mid = lo + ((hi - lo) >> 1);
                            if (line_nus[mid] <= v) lo = mid + 1; else hi = mid;
                        }
                        cnt = lo;
                    }
                    w.cnt_ge[pidx] = (int)cnt;
                }
            }
            return;
        }
    }
    // Round 5: every thread keeps its (line, depth) items in REGISTERS, depth fastest — the order of the reference layout it reads
    // and of the line-major narrow arrays it writes: loads and narrow stores coalesce as they are, and nothing is staged through
    // LDS (rounds 1 - 4 transposed the block through 70 KB of it so that the depth-major wide records were written line-fastest:
    // three arrays written, read transposed, the derived constants written back and read again by a second pass, two more barriers).
    // The depth-major records of WIDE items — a few per cent of a list — and the scan words go out as scattered 16 / 48-byte stores;
    // the lines of a block are neighbours in those rows, so the pieces of a 64-byte sector meet in the L2 of the XCD the block runs
    // on before it is written back.  3 KB of LDS per block instead of 70: the size of a block is its threads and registers alone.
    // (54 lines per block: models of at most 56 depth points — every MARCS model has 56 — where 54 x 56 items are three per thread)
    constexpr int kItemDepths = kPreLines == 54 ? 56 : kPreDepths;
    constexpr int kPreItems = (kPreLines * kItemDepths + kPreBlock - 1) / kPreBlock;  // items per thread
    static_assert(kPreLines <= 64, "lines per pre-pass block");
    static_assert(!(PLANNED && GEN), "the generating pre-pass takes no grid plan");
#ifdef SDX_PRE_STATS
    unsigned long long pst[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    SDX_PRE_STAMP(0);
    constexpr int kMaxWaves = kPreBlock / 64;
    __shared__ int64_t s_c[kPreLines];
    __shared__ double s_red[kMaxWaves];
    __shared__ unsigned long long s_ev[kMaxWaves];
    __shared__ int s_hwmax[kPreLines], s_whwmax[kPreLines];
    __shared__ double s_lnu[kPreLines];

    const int nthreads = blockDim.x;
    const bool gather = gbx >= 0;
    const int64_t l0 = (int64_t)(gather ? gbx : bx) * kPreLines;
    const int d0 = by * kPreDepths;
    // which lines this block prepares: kPreLines consecutive ones, or — gather blocks — kPreLines consecutive entries of hlist
    __shared__ int s_l[kPreLines];
    int nl = (int)min((int64_t)kPreLines, n_lines - l0);
    int n_h = 0;
    if (gather) {
        // the gather list: hlist, then xlist
        n_h = w.hcount[0];
        const int n_g = n_h + (w.xlist ? w.hcount[2] : 0);
        if (l0 >= n_g) return;  // block-uniform
        nl = min(kPreLines, n_g - (int)l0);
        if (tid < kPreLines) {
            const int k = (int)l0 + tid;
            s_l[tid] = tid < nl ? (k < n_h ? w.hlist[k] : w.xlist[k - n_h]) : 0;
        }
        __syncthreads();
    } else {
        if (w.sel && (l0 + kPreLines <= w.sel[2] || l0 >= w.sel[3])) return;  // not a block of the shard's own line range
        if (tid < kPreLines) s_l[tid] = (int)(l0 + tid);
        // (no barrier needed: the non-gather path indexes with l0 + ll directly)
    }
#define SDX_LINE_OF(ll) (gather ? (int64_t)s_l[ll] : l0 + (ll))
    const int nd = min(kPreDepths, n_depth - d0);
    const unsigned nd_magic = small_div_magic(nd);  // (items k < kPreLines kPreDepths = 4096)
    // line centres first: a sample of the grid in LDS brackets the answer — 128 points read from the grid itself where the block
    // also scans the grid spacing (<= 16384 points), otherwise the 2048 points the grid-spacing launch left (kGridSample): a
    // bracket of at most 64 points up to 131 072 grid points, i.e. no dependent global load before the one that resolves it
    // (rounds 1 - 4 sampled 128 points whatever the grid, and at 120 398 points a block spent 5.9 of its 26 us on four bisection
    // steps in global memory — device time stamps, scripts/r5/pre_stats.sh)
    __shared__ double s_coarse[kGridSample];
    const int n_samp = dnu_partial ? kGridSample : 128;  // (the launch that left the partial maxima also left the sample)
    [[maybe_unused]] const int64_t cstride = (n_nu + n_samp - 1) / n_samp;
    if constexpr (PLANNED) {
        // (s_coarse stays: the block that lists the wide lines keeps its masks there)
        if (tid < kPreLines) s_c[tid] = tid < nl ? (int64_t)w.centre[SDX_LINE_OF(tid)] : 0;
    } else if (dnu_partial) {
        for (int q = tid; q < kGridSample; q += kPreBlock) s_coarse[q] = dnu_partial[kGridSampleOffset + q];
    } else if (tid < 128) {
        const int64_t j = (int64_t)tid * cstride;
        s_coarse[tid] = j < n_nu ? nus[j] : -INFINITY;
    }
    if (tid >= kPreBlock - kPreLines) {
        const int ll = tid - (kPreBlock - kPreLines);
        s_lnu[ll] = ll < nl ? line_nus[SDX_LINE_OF(ll)] : 0.0;
    }

    // this thread's share of max(diff(nus)), requested now — its loads travel while the centres are searched: one of the partial
    // maxima a launch before this one left (long grids: n_partial <= kDnuPartials < the block's threads), or its part of the scan
    [[maybe_unused]] double dnu_local = 0.0, plan_dnu = 0.0, plan_rdnu = 0.0;
    if constexpr (PLANNED) {
        plan_dnu = dnu_partial[0], plan_rdnu = dnu_partial[1];  // (requested with the centres above and the dense inputs below)
    } else {
        dnu_local = dnu_partial ? (tid < n_partial ? dnu_partial[tid] : -INFINITY) : dnu_scan_local(nus, n_nu);
        __syncthreads();
    }
    SDX_PRE_STAMP(1);  // the grid sample and the line frequencies are in LDS
    // The block's dense inputs are requested now (kPreItems per thread): their latency hides behind the centre search below —
    // whose one global load they precede in the queue — instead of following it; requested before the barrier above they only
    // held eighteen registers through the sample's hand-over.
    [[maybe_unused]] double r_dw[kPreItems], r_a[kPreItems], r_g[kPreItems];
    if constexpr (!GEN) {
#pragma unroll
        for (int it = 0; it < kPreItems; ++it) {
            const int k = tid + it * kPreBlock;
            r_dw[it] = r_a[it] = r_g[it] = 0.0;
            if (k < nl * nd) {
                const int ll = small_div(k, nd_magic), dd = k - ll * nd;
                const int64_t l = SDX_LINE_OF(ll);
                const int d = d0 + dd;
                r_dw[it] = doppler[l * n_depth + d];
                r_a[it] = alphas[l * n_depth + d];
                r_g[it] = gamma_cols > 1 ? gammas[l * gamma_cols + d] : gammas[l * gamma_cols];
            }
        }
    }
    // wave ll narrows the bracket of line ll to 64 points by bisection (none needed when the grid has <= 8192 points) and resolves
    // it with ONE coalesced load and a ballot — a chain of one or two dependent global loads instead of log2(N_nu / 128)
    if constexpr (!PLANNED)
    for (int ll = tid >> 6; ll < nl; ll += kPreBlock / 64) {
        const int lane = tid & 63;
        {
            const double v = s_lnu[ll];
            int a = 0, b = n_samp;  // first sample strictly below v
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (s_coarse[mid] >= v) a = mid + 1; else b = mid;
            }
            // the answer lies in ((a-1)*cstride, a*cstride]
            int64_t lo = a > 0 ? (int64_t)(a - 1) * cstride + 1 : 0;
            int64_t hi = min((int64_t)a * cstride, n_nu);
            while (hi - lo > 64) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (nus[mid] >= v) lo = mid + 1; else hi = mid;
            }
            const int64_t idx = lo + lane;
            const bool below = idx < hi && nus[idx] < v;
            const unsigned long long m = __ballot(below);
            if (lane == 0) s_c[ll] = m ? lo + __builtin_ctzll(m) : hi;
        }
    }
    if (tid < kPreLines) s_hwmax[tid] = 0, s_whwmax[tid] = 0;
    SDX_PRE_STAMP(2);  // this wave's centres are found
    // d_nu (:524-526): from the partial maxima of k_dnu_partial, or — small grids — scanned here directly
    // (its barriers also publish the centres and the cleared maxima)
    // (block-uniform: both live in scalar registers — three items per thread leave the 64-VGPR budget no room for them)
    double d_nu_v, r_dnu_v;
    if constexpr (PLANNED) {
        d_nu_v = plan_dnu, r_dnu_v = plan_rdnu;
        __syncthreads();  // the line frequencies, the centres and the cleared maxima are in LDS
    } else {
        d_nu_v = block_max_to_dnu(dnu_local, s_red);
        r_dnu_v = 1.0 / d_nu_v;
    }
    const double d_nu = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(d_nu_v)), __builtin_amdgcn_readfirstlane(__double2loint(d_nu_v)));
    const double r_dnu = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(r_dnu_v)), __builtin_amdgcn_readfirstlane(__double2loint(r_dnu_v)));
    SDX_PRE_STAMP(3);  // grid spacing known

    [[maybe_unused]] __shared__ GenDepth s_gd[GEN ? kPreDepths : 1];
    [[maybe_unused]] __shared__ GenLine s_gl[GEN ? kPreLines : 1];
    if constexpr (GEN) {
        // line parameters from per-line scalars and per-depth state (f1): nothing dense to read.  The per-depth and the
        // per-line factors (every pow / tgamma / n_eff) are evaluated once per block column / row and shared through LDS.
        if (tid < nd) s_gd[tid] = gen_depth(lp, d0 + tid);
        else if (tid >= 64 && tid < 64 + nl) s_gl[tid - 64] = gen_line(lp, line_nus[SDX_LINE_OF(tid - 64)], SDX_LINE_OF(tid - 64));
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kPreItems; ++it) {
            const int k = tid + it * kPreBlock;
            r_dw[it] = r_a[it] = r_g[it] = 0.0;
            if (k < nl * nd) {
                const int ll = small_div(k, nd_magic), dd = k - ll * nd;
                const GenDepth& D = s_gd[dd];  // fields are read from LDS where they are used: copies would cost ~40 VGPRs
                const GenLine& L = s_gl[ll];
                r_dw[it] = gen_doppler(lp, L, D);
                r_a[it] = gen_alpha(lp, L, D, d0 + dd, n_depth);
                r_g[it] = gen_gamma(lp, L, D);
            }
        }
    }

    // ONE arithmetic pass, depth fastest; every output of an item leaves from its thread
    constexpr bool kCountEvals = kPreLines < 48;  // (48 lines per block: culled shards only, which never count — two registers the block needs)
    [[maybe_unused]] unsigned long long ev = 0;
    // what the scan word of an item is rebuilt from after the barrier (two registers per item instead of the word's four: three
    // items per thread have to fit 64 VGPRs — two resident blocks per CU): the half-width of a WIDE window (0: the word is empty) and
    // the core's half-width, negative when the core is delegated to the narrow role
    int keep_hw[kPreItems], keep_chw[kPreItems];
#pragma unroll
    for (int it = 0; it < kPreItems; ++it) {
        const int k = tid + it * kPreBlock;
        keep_hw[it] = 0, keep_chw[it] = 0;
        if (k >= nl * nd) continue;
        const int ll = small_div(k, nd_magic), dd = k - ll * nd;
        const int64_t l = SDX_LINE_OF(ll);
        const double dw = r_dw[it], g = r_g[it], a = r_a[it];
        const int64_t c = s_c[ll];
        int lo, hi;
        const int64_t hw = window_rule(c, n_nu, d_nu, r_dnu, g, dw, a, lo, hi);
        const bool narrow = hw <= kNarrowHalfWidth;
        // 1 / dw once (the refined hardware reciprocal: the correctly rounded value but for ~1 in 1e8 arguments), y and the amplitude
        // as products with it — within 2 ulp of the reference's quotients (voigt.py:148-149), which the kernels multiply into x = dnu (1 / dw)
        // and the profile anyway; three divisions (~25 instructions each) fewer per item (round 6)
        double inv, yy, amp;
        narrow_params(dw, g, a, inv, yy, amp);
        int core_hw = 0;
        bool delegated = false;
        if (w.wscan) {
            const size_t o = (size_t)(d0 + dd) * n_lines + l;  // depth-major (wide kernel)
            WideScan sc = {0, 0, 0, 0};
            if (!narrow && hi > lo) {
                // core: grid points with |x| + y <= 15 lie within (15 - y) doppler widths of the line, i.e. within
                // floor(that / d_nu) + 1 points of the centre (d_nu is the SMALLEST spacing of the grid, :524-526).  A margin
                // (15.001, + 2 points) covers the rounding of x = delta_nu * (1 / dw); a superset costs nothing but speed.
                const double reach = mul_rn(mul_rn(15.001 - yy, dw), r_dnu);
                const int64_t chw = yy < 15.001 ? (reach >= (double)n_nu ? n_nu : (int64_t)reach + 2) : 0;
                keep_chw[it] = (int)min(chw, (int64_t)2147483647);
                sc.lo = lo;
                sc.hi = hi;
                sc.clo = max((int)max(c - chw, (int64_t)0), lo);
                sc.chi = chw > 0 ? min((int)min(c + chw, n_nu), hi) : sc.clo;
                // A core no wider than a narrow window is DELEGATED to the narrow role (lanes <-> depth: all depths of a line
                // sit in the same Faddeeva regions at one frequency, where a 64-point tile holds a few core points of one
                // depth): the narrow arrays below get the core's half-width as this item's window and the wide role leaves
                // those points out.
                delegated = chw > 0 && chw <= kNarrowReach && sc.chi > sc.clo;
                core_hw = (int)min(chw, hw);  // the core is clipped by the window (64 < hw < chw happens)
                if (delegated) {
                    atomicMax(&s_hwmax[ll], (int)chw);
                    sc.clo = -sc.clo - 1;  // the sign marks the delegation
                }
                const RegionI k1 = region1_setup(yy, amp);
                const double lnu = s_lnu[ll];
                w.wrec[o] = WideRec{lnu, inv, k1.yk, k1.cv, k1.cd, 0.0};
                w.wslow[o] = WideSlow{yy, amp};
                if (w.wrec32) {
                    const float nuh = (float)lnu;
                    w.wrec32[o] = WideRec32{nuh, (float)k1.yk, (float)inv, -((float)(lnu - (double)nuh) * (float)inv), (float)k1.cv, (float)k1.cd, 0.f, 0.f};
                }
                atomicMax(&s_whwmax[ll], (int)hw);
            } else if (narrow) {
                atomicMax(&s_hwmax[ll], (int)hw);
            }
            if (!narrow && hi > lo) keep_hw[it] = (int)hw, keep_chw[it] = delegated ? -keep_chw[it] : keep_chw[it];  // (the word is stored below, once the line's widest window is known)
            // a gather block knows its lines' positions in hlist: the list-ordered copy of the scan word is written here
            // (culled runs; otherwise k_hscan makes it once the list exists)
            if (gather && w.hscan && l0 + ll < n_h) w.hscan[(size_t)(d0 + dd) * n_lines + l0 + ll] = sc;
        }
        // line-major outputs, depth fastest: the stores coalesce
        const size_t o = (size_t)l * n_depth + (d0 + dd);
        if (out_lo_ref) {  // sdx_line_windows_dev (no wide records there: the window itself)
            out_lo_ref[o] = lo;
            out_hi_ref[o] = hi;
        }
        if (w.nhw) {
            // the narrow role's window: a narrow item's own half-width, the delegated core's, or nothing
            w.nhw[o] = (unsigned char)(narrow ? (int)hw : (delegated ? core_hw : 0));
            if ((narrow || delegated) && !w.narrow_raw) {
                if (w.n_inv32) {
                    w.n_inv32[o] = (float)inv;
                    w.n_y32[o] = (float)yy;
                    w.n_amp32[o] = (float)amp;
                } else {
                    w.n_inv[o] = inv;
                    w.n_y[o] = yy;
                    w.n_amp[o] = amp;
                }
            }
        }
        if constexpr (kCountEvals) {
            if (hi > lo) ev += (unsigned long long)(hi - lo);
        }
    }
    SDX_PRE_STAMP(4);  // arithmetic and per-item stores issued
    __syncthreads();
    SDX_PRE_STAMP(5);
    // the scan words (depth-major): every tile of the wide role scans the word of a line it considers — all lines of a short
    // list, the hlist / wlist lines of a long one.  A line of a long list without a wide window at any depth is in neither
    // list: its 16 bytes per depth (0.9 of 2.8 GB of pre-pass writes at 1e6 lines) are not written.
    if (w.wscan) {
#pragma unroll
        for (int it = 0; it < kPreItems; ++it) {
            const int k = tid + it * kPreBlock;
            if (k >= nl * nd) continue;
            const int ll = small_div(k, nd_magic), dd = k - ll * nd;
            if (w.skip_unlisted_scan && s_whwmax[ll] == 0) continue;
            WideScan sc = {0, 0, 0, 0};
            if (keep_hw[it] > 0) {  // the word of the arithmetic pass, from the same integers
                const int64_t c = s_c[ll], hw = keep_hw[it], chw = keep_chw[it] < 0 ? -(int64_t)keep_chw[it] : (int64_t)keep_chw[it];
                const int64_t lw = c - hw, hw_end = c + hw;
                sc.lo = (int)(lw < 0 ? 0 : lw);
                sc.hi = (int)(hw_end > n_nu ? n_nu : hw_end);
                sc.clo = max((int)max(c - chw, (int64_t)0), sc.lo);
                sc.chi = chw > 0 ? min((int)min(c + chw, n_nu), sc.hi) : sc.clo;
                if (keep_chw[it] < 0) sc.clo = -sc.clo - 1;
            }
            w.wscan[(size_t)(d0 + dd) * n_lines + SDX_LINE_OF(ll)] = sc;
        }
    }
    // per-line summary for the narrow kernel's candidate test: centre index and the largest narrow half-width
    if (w.nhw_max && tid < nl) {
        if (gy == 1) {
            w.nhw_max[SDX_LINE_OF(tid)] = s_hwmax[tid];
            // (write-through where the block that lists the wide lines reads it in this launch)
            if (LIST && kPreLines <= 32 && w.n_csplit) __hip_atomic_store(&w.whw_max[SDX_LINE_OF(tid)], s_whwmax[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else w.whw_max[SDX_LINE_OF(tid)] = s_whwmax[tid];
        } else {  // deep models: several depth blocks per line, both arrays zeroed by the host first
            atomicMax(&w.nhw_max[SDX_LINE_OF(tid)], s_hwmax[tid]);
            atomicMax(&w.whw_max[SDX_LINE_OF(tid)], s_whwmax[tid]);
        }
        if constexpr (!PLANNED) if (by == 0) w.centre[SDX_LINE_OF(tid)] = (int)s_c[tid];
        if (by == 0 && w.lnu32) {
            const double lnu = s_lnu[tid];
            w.lnu32[SDX_LINE_OF(tid)] = float2v{(float)lnu, (float)(lnu - (double)(float)lnu)};
        }
    }
    if constexpr (kCountEvals) {
        if (w.evals) {
            for (int off = 32; off > 0; off >>= 1) ev += __shfl_xor(ev, off);
            if ((tid & 63) == 0) s_ev[tid >> 6] = ev;
            __syncthreads();
            if (tid == 0) {
                for (int i = 1; i < (nthreads >> 6); ++i) ev += s_ev[i];
                if (ev) atomicAdd(w.evals, ev);
            }
        }
    }
    // Short lists: the LAST line block to finish lists the lines with a wide window for the wide role (LineWork::n_csplit) — in this
    // launch, and no block waits for another.  whw_max went out write-through (an atomic store / atomicMax at the L2); every storing
    // wave drains its stores, ONE lane draws the block's ticket, and in the block that drew the last one that lane's agent-scope
    // acquire precedes the block's (vector) loads of whw_max.  The launch boundary publishes the list to the line kernel.
    // (short lists run 16 or 32 lines per block, never the counter-driven launch)
    if constexpr (LIST && kPreLines <= 32) if (w.n_csplit) {  // (block-uniform)
        __shared__ int s_last;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const int t = __hip_atomic_fetch_add(w.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = t == n_line_blocks * gy - 1 ? 1 : 0;
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(w.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the next step counts from zero
            }
            s_last = last;
        }
        __syncthreads();
        if (s_last) compact_wide_lines(w, n_lines, reinterpret_cast<unsigned long long*>(s_coarse), tid);
    }
#ifdef SDX_PRE_STATS
    if (tid == 0) {
        unsigned long long* const o = g_pre_stats + (size_t)((bx * 2 + (gather ? 1 : 0)) & (kPreStatSlots - 1)) * 8;
        o[0] = ((unsigned long long)bx << 8) | (gather ? 2 : 0) | 1;
        for (int q = 0; q < 6; ++q) o[1 + q] = pst[q];
        o[7] = wall_clock64();
    }
#endif
#undef SDX_LINE_OF
}

template <bool GEN, int LINES>
__global__ __launch_bounds__(kPreBlock) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(8, 8))) void k_line_prepass(int n_depth, int64_t n_nu, const double* __restrict__ nus,
                                                         const double* __restrict__ dnu_partial, int n_partial,
                                                         int64_t n_lines, const double* __restrict__ line_nus,
                                                         const double* __restrict__ doppler,
                                                         const double* __restrict__ gammas, int gamma_cols,
                                                         const double* __restrict__ alphas, LineWork w,
                                                         int* __restrict__ out_lo_ref, int* __restrict__ out_hi_ref,
                                                         int n_line_blocks, LineParams lp)
{
    // (dispatching the pixel and gather blocks of a culled shard BEFORE its line blocks — a rotated grid — was measured in round 4:
    // 47 against 44 us for this launch on an eighth of S-c3; the order stays [line | pixel | gather])
    int bx = blockIdx.x;
    if (w.sel && w.front) {
        // A culled shard's grid is one block per CANDIDATE (every block of consecutive lines twice over, 9 500 at S-c3) of which a
        // few hundred have work — somewhere in the middle of the range for most ranks, behind thousands of blocks that only look at
        // `sel` and leave, each holding a block slot (70 KB of LDS) for a round trip.  Here the blocks that have work are the FIRST of
        // the grid, whatever the rank: block index -> item by the counts the list launch left (range blocks, gather blocks, pixel
        // blocks; the long items first), and everything behind them returns.  Which block prepares an item does not matter.
        const int first = w.sel[2] / LINES, n_range = max((w.sel[3] + LINES - 1) / LINES - first, 0);
        const int n_g = (w.hcount[0] + (w.xlist ? w.hcount[2] : 0) + LINES - 1) / LINES;
        const int item = bx;
        if (item < n_range) bx = first + item;
        else if (item < n_range + n_g) bx = n_line_blocks + w.n_pix + (item - n_range);
        else if (item < n_range + n_g + w.n_pix) bx = n_line_blocks + (item - n_range - n_g);
        else return;
    }
    prepass_block<GEN, LINES>(bx, blockIdx.y, gridDim.y, n_depth, n_nu, nus, dnu_partial, n_partial, n_lines, line_nus, doppler, gammas,
                       gamma_cols, alphas, w, out_lo_ref, out_hi_ref, n_line_blocks, lp);
}

// The pre-pass of a CULLED shard.  Which blocks have work is only known on the device (sel, the list counts); one block per
// candidate is every block of the list twice over — 9 500 blocks for 600 with work at an eighth of S-c3, 62 000 for 5 000 at 1e6
// lines, each costing a dispatch, 70 KB of LDS and a dependent load before it returns (a third of that launch at 1e6 lines).  Here
// as many blocks as the chip holds draw the items that exist from a counter — the range blocks, then the gather blocks, then the
// pixel blocks — until none is left.  Which block prepares an item does not matter: every item writes its own outputs.  The thread index
// goes through an empty asm inside the loop: left visible, everything that depends only on it (a dozen addresses, the grid sample)
// is hoisted out of the loop and kept in registers — 91 VGPRs instead of 51, one resident block per CU instead of two.
template <int LINES>
__global__ __launch_bounds__(kPreBlock) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(8, 8))) void k_line_prepass_ticket(
    int n_depth, int64_t n_nu, const double* __restrict__ nus, const double* __restrict__ dnu_partial, int n_partial, int64_t n_lines,
    const double* __restrict__ line_nus, const double* __restrict__ doppler, const double* __restrict__ gammas, int gamma_cols,
    const double* __restrict__ alphas, LineWork w, int n_line_blocks, LineParams lp)
{
    __shared__ int s_item;
    const int first = w.sel[2] / LINES, n_range = max((w.sel[3] + LINES - 1) / LINES - first, 0);
    const int n_g = w.hcount[0] + (w.xlist ? w.hcount[2] : 0);
    const int total = w.n_pix + n_range + (n_g + LINES - 1) / LINES;
    for (;;) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        if (tid == 0) s_item = atomicAdd(w.ticket + blockIdx.y, 1);
        __syncthreads();
        const int item = s_item;
        __syncthreads();  // (s_item is drawn again at the top; the block's LDS arrays serve its next item)
        if (item >= total) return;
        // (the long items first, the pixel blocks — a binary search per thread — last: they fill the launch's tail)
        const int n_long = total - w.n_pix;
        const int bx = item < n_range ? first + item : (item < n_long ? n_line_blocks + w.n_pix + (item - n_range) : n_line_blocks + (item - n_long));
        prepass_block<false, LINES, false>(bx, blockIdx.y, gridDim.y, n_depth, n_nu, nus, dnu_partial, n_partial, n_lines, line_nus, doppler, gammas, gamma_cols, alphas, w,
                                    nullptr, nullptr, n_line_blocks, lp, tid);
    }
}

// ------------------------------------------------------------------------------------------------
// Line opacity, wide windows, gather form.  One single-wave block owns (depth d, a tile of 64*R grid points, one
// of S line subsets); lane k owns grid points t0 + k + 64 r (r < R) and accumulates in registers.  The block
// streams its subset of the line list in chunks of 64 (chunk c belongs to subset c mod S): each lane tests one
// line's window against the tile, survivors are compacted (order-preserving, wave ballot) into LDS together with
// their depth-column constants, then every lane walks the compacted list.  Splitting the line list over S blocks
// shortens the serial chain of the deepest (hottest) layers, whose windows are widest; the S partial planes are
// added in subset order by the consumer (k_reduce_partials / k_total_alphas).  No atomics: bit-stable results.
// ------------------------------------------------------------------------------------------------
// Line opacity, wide windows, gather form.  One wave owns (depth d, a tile of 64 R grid points, one of S line subsets);
// lane k owns grid points t0 + k + 64 r (r < R) and accumulates in registers.  The wave goes through its candidate lines
// 64 at a time (chunk q of 64 consecutive candidates belongs to subset q mod S):
//   scan   each lane tests ONE candidate's window against the tile (16 B per candidate, coalesced) -> two wave masks:
//          `hit` (window overlaps the tile) and `fast` (the tile lies wholly inside the window and wholly outside the
//          line's core range, so every point is in Faddeeva region I and inside: no per-point tests);
//   walk   the hits in ascending order; the 48-byte record of a hit (line frequency, 1 / doppler, region-I constants) is
//          fetched from ONE address by the whole wave — scalar or broadcast loads, no LDS staging, no cross-lane traffic —
//          the next hit's record being requested before the current one is evaluated.
// Candidates: every line of the list (short lists), or — long lists — first the lines whose widest window exceeds
// kMediumHalfWidth (`hlist`, they may reach any tile) and then the lines whose CENTRE lies within kMediumHalfWidth of the
// tile, a contiguous index range read from cnt_ge (lines are sorted, so centres descend).  Chunks are counted from the start
// of the list (hlist position / line index), so the partition into subsets — and with it the summation order of a grid
// point — does not depend on the tile or on how the grid is sharded.
// The S subsets of a (depth, tile) are the S waves of one workgroup: their partial sums meet in LDS and wave 0 adds them in
// subset order and writes the tile — one line-opacity plane, no atomics, bit-stable results.
// ------------------------------------------------------------------------------------------------
// FAR FIELD.  The reference's window of a strong line spans thousands of grid points ((gamma + doppler) alpha / d_nu * 20 pixels,
// base.py:561-575): nine tenths of all window evaluations of the 3000 - 10000 A workloads lie more than two tiles away from
// the line's centre, where the profile is the region-I rational — a smooth function of frequency whose nearest singularity is
// the line itself.  For a full tile [i0, i1) of 64 R points with end frequencies nu_a > nu_b, centre c = (nu_a + nu_b) / 2 and
// half-width h = (nu_a - nu_b) / 2, a (line, depth) item is FAR when the tile lies wholly inside its window, clear of its core
// range (every point in region I) and |c - nu_l| >= 6 h (decided in index space, k_far_ranges).  The sum of the far items of a tile is then evaluated at the tile's
// kFarNodes = 16 Chebyshev nodes c + h cos(pi (j + 1/2) / 16) — the same rational, the same records, fp64 — and carried to
// the tile's grid points by the degree-15 interpolant (line_far_body): 16 evaluations per (item, tile) instead of 64 R.  The
// interpolation error of a function analytic inside the ellipse through a pole at distance D from the centre is
// ~ (D/h + sqrt((D/h)^2 - 1))^-16 <= 11.9^-16 = 6e-18 of the item's value; measured against 80-bit sums of the far items of
// S-c3's tiles: 2.5e-14 relative, rounding included (the direct fp64 sum: 4e-15).  The opacity tolerance is 1e-12, the flux's 1e-10.
// Which triples are far is a property of the grid and the list (global tiles), not of the shard or the launch geometry; both
// kernels decide it with THIS function on the same operands, so every triple is evaluated exactly once.
constexpr int kFarWaveLdsDoubles = 64 * 6 + 64;  // per wave of the far role: 64 staged records, the queue's line indices and tile masks
// The distance test in INDEX space, once per tile (one thread each): a line's centre index is cidx = #{i : nus[i] >= nu_l}
// (closest_index, the reference's own quantity), so with ihi = #{i : nus[i] >= c + 6 h} and ilo = #{i : nus[i] >= c - 6 h}
//   cidx < ihi  =>  nu_l > nus[ihi - 1] >= c + 6 h        cidx > ilo  =>  nu_l <= nus[ilo] < c - 6 h
// — rigorous on any descending grid, whatever its spacing does, and the kernels compare integers per candidate instead of
// carrying its frequency.  Tiles without a far field (cut by the grid's end, or of zero width) get (0, INT_MAX): never far.
// (far_ranges_block, near the top of this file: it rides in the launch that measures the grid's spacing.)
// The centre index itself is not needed: the core range of a scan word always holds it (prepass_block: clo <= c <= chi, both equal
// to c where the core is empty), so chi < ihi or clo > ilo decide the same thing from the 16 bytes every candidate test reads anyway
// — conservatively where a core is wide, which only leaves a few more tiles to the direct sum.
__device__ __forceinline__ bool far_eligible(const WideScan& sc, int i0, int i1, int ihi, int ilo)
{
    const int clo = sc.clo < 0 ? -sc.clo - 1 : sc.clo;
    return (sc.lo <= i0) & (sc.hi >= i1) & ((i1 <= clo) | (i0 >= sc.chi)) & ((sc.chi < ihi) | (clo > ilo));
}

constexpr int kWideLdsDoubles = 64 * 8;  // per wave: R <= 8 partial sums per lane
// ... and in the fp64 kernels with a far field, whose wide role queues its hits (line_wide_walk): 64 staged records (48 B), their
// scan words (16 B) and the queue itself (64 ints)
constexpr int kWideFarLdsDoubles = 64 * 6 + 64 * 2 + 32;
#ifndef SDX_WIDE_QUEUED  // (A/B builds: 0 = the direct walk in the far-field kernels too)
#define SDX_WIDE_QUEUED 1
#endif
#ifndef SDX_SCAN_BATCH   // (A/B builds: chunks of candidates requested together by a queued walk)
#define SDX_SCAN_BATCH 1
#endif
#ifndef SDX_FAR_WAVES    // (A/B builds: waves per SIMD the fp64 far-field line kernels are compiled for)
#define SDX_FAR_WAVES 6
#endif

template <int R, int STRIDE = kWideLdsDoubles>
__device__ __forceinline__ void wide_reduce_and_store(const int split, const int n_split, double (&acc)[R], const int idx0, const int64_t s0,
                                                      const int64_t s1, double* __restrict__ lds_all, double* __restrict__ plane, int64_t pld,
                                                      const int d)
{
    const int lane = threadIdx.x & 63;
    if (n_split > 1) {
        if (split > 0) {
            double* mine = lds_all + (size_t)split * STRIDE;
#pragma unroll
            for (int r = 0; r < R; ++r) mine[r * 64 + lane] = acc[r];
        }
        __syncthreads();
        if (split == 0) {
#pragma unroll 1  // (unrolled eight times the reads of all subsets are hoisted above the sums and spill)
            for (int s = 1; s < n_split; ++s) {
                const double* other = lds_all + (size_t)s * STRIDE;
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = add_rn(acc[r], other[r * 64 + lane]);
            }
        }
    }
    if (split == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (idx0 + 64 * r >= s0 && idx0 + 64 * r < s1) plane[(size_t)d * pld + (idx0 + 64 * r - s0)] = acc[r];  // the shard's columns only
    }
}

// fp32 evaluation of the region-I rational for the mixed-precision mode, TWO grid points per instruction (v_pk_add / mul /
// fma_f32: a packed instruction issues like one fp64 instruction and does two evaluations; only the reciprocal is per
// point).  x = fma(dq, inv, c0) like the fp64 walk's: dq = the lane's frequencies as OFFSETS from the tile's base frequency
// (formed in fp64, rounded once: 1.2e4 Hz at the far end of a tile, 1e-5 of a Doppler width) and c0 = (base - nu_l) * inv from
// the hi / lo split of the line frequency, formed once per (line, tile) — ONE packed instruction per pair of points where rounds
// 2 - 4 spent three on the hi / lo split of both frequencies (round 5: 18 -> 14 packed instructions per line and lane).
// Everything else is plain fp32 (v_rcp_f32 is good to 1 ulp).
__device__ __forceinline__ float region1_c0(float base_h, const WideRec32& k)
{
    return fmaf(base_h - k.nuh, k.inv, k.ncl);  // ((base_h - nuh) - nul) * inv: the difference of two fp32 frequencies is exact
}
__device__ __forceinline__ float2v region1_f32x2(float2v acc, float2v dq, float c0, const WideRec32& k)
{
    const float2v x = __builtin_elementwise_fma(dq, (float2v)(k.inv), (float2v)(c0));
    const float2v v = __builtin_elementwise_fma(x, x, (float2v)(k.cv));
    const float2v den = __builtin_elementwise_fma(v, v, (float2v)(k.cd));
    const float2v num = __builtin_elementwise_fma((float2v)(k.yk), v, (float2v)(k.yk));
    float2v r;
    r.x = __builtin_amdgcn_rcpf(den.x);
    r.y = __builtin_amdgcn_rcpf(den.y);
    // no inline asm here: its operands come straight from v_rcp_f32, and the compiler does not insert the wait state a
    // transcendental result needs before a VALU use when the user is an asm statement
    return __builtin_elementwise_fma(num, r, acc);
}

// DEFER: the partial sums of this wave are handed back (acc_out) instead of being reduced and stored here — the kernel of dense
// long lists has ONE reduction for both roles (line_all_body)
// STAGED (fp32-mixed mode, the kernel of very dense lists): the records of a chunk's hits reach the lanes through LDS (below)
// LISTED (fp64, short lists): the candidates are this subset's list of wide lines (LineWork::n_csplit) — a kernel of its own
// (k_line_listed), so that the kernels that scan compile to what they were
template <int R, bool MIXED, bool DEFER = false, bool STAGED = false, bool FAR = false, bool LISTED = false>
__device__ __forceinline__ void line_wide_walk(const int tile_idx, const int split, const int n_split, const int d, int64_t n_nu,
                                               const double* __restrict__ nus, int64_t nu_begin, int64_t nu_count, int64_t n_lines,
                                               LineWork w, double* __restrict__ plane, int64_t pld, double* __restrict__ lds_all,
                                               double* __restrict__ acc_out = nullptr)
{
    constexpr int kTile = 64 * R;
    // GLOBAL tiles: tile boundaries are multiples of kTile from grid index 0 whatever the shard, and a tile cut by a shard
    // boundary is classified and evaluated whole (only the stores are masked).  How a (line, depth, tile) is treated — test-free,
    // edge, core — and which four points of a lane share one reciprocal is then a property of the grid alone: a frequency shard
    // produces the bits of the unsharded run.
    const int64_t t0 = (nu_begin / kTile + (int64_t)tile_idx) * kTile;
    const int64_t t1 = min(t0 + kTile, n_nu);
    const int64_t s0 = nu_begin, s1 = nu_begin + nu_count;  // columns stored by this launch
    const int lane = threadIdx.x & 63;
    const int it0 = (int)t0, it1 = (int)t1;

    // fp64 mode: the lane's frequencies as offsets from the tile's first frequency (exact: neighbouring grid frequencies are
    // within a factor of two), so that x = (nu_i - nu_l) / doppler is ONE instruction per point,
    // x = fma(dnu_i, inv, c0) with c0 = (nu_base - nu_l) * inv formed once per (line, tile).  Mixed mode: hi + lo fp32 pairs only
    // (the fp64 value is their exact sum to 2^-48, rebuilt on the rare general path), so that R = 8 points per lane fit the
    // register budget
    double dnu[MIXED ? 1 : R], acc[R];
    float2v dq[MIXED ? R / 2 : 1], acc32[MIXED ? R / 2 : 1];  // pairs of points (r, r + 1): offsets from the tile's base frequency, fp32 sums
    // (grid index of point r of this lane: it0 + lane + 64 r, formed where it is needed — an edge test, the final store —
    // instead of living in registers through the walk)
    const int idx0 = it0 + lane;
    // (both halves through readfirstlane: the base is wave-uniform and ends up in an SGPR pair)
    const double nu_base_v = nus[t0];
    const double nu_base = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(nu_base_v)), __builtin_amdgcn_readfirstlane(__double2loint(nu_base_v)));
    // ... and a copy pinned in a VGPR pair: c0 = (nu_base - nu_l) * inv takes the record's nu_l as its scalar operand (a VALU
    // instruction reads one SGPR pair), otherwise the compiler moves nu_l into vector registers for every line it walks
    double nu_base_vec = nu_base;
    asm("" : "+v"(nu_base_vec));
    // mixed mode: the base frequency as an fp32 number (in a VGPR: it meets the record's scalar operands in one instruction)
    float base_h = (float)nu_base;
    asm("" : "+v"(base_h));
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = t0 + lane + r * 64;
        const double nu = i < t1 ? nus[i] : nu_base;
        acc[r] = 0.0;
        if constexpr (MIXED) {
            dq[r >> 1][r & 1] = (float)(nu - (double)base_h);  // (exact in fp64, rounded once)
            acc32[r >> 1][r & 1] = 0.f;
        } else {
            dnu[r] = nu - nu_base;
        }
    }
    // far field: the triples the far role evaluates at the tile's Chebyshev nodes are no hits here (full tiles only)
    // (FAR is a kernel of its own: the candidate's centre index is one more register carried through the walk, and the walk's
    // budget has none to spare — with the test in the one kernel its sums spilled to scratch)
    static_assert(!FAR || kTile == kFarTile, "the far field lives on 256-point tiles");
    [[maybe_unused]] int far_ihi = 0, far_ilo = 0x7FFFFFFF;  // (never far)
    if constexpr (FAR) {
        far_ihi = __builtin_amdgcn_readfirstlane(w.far_range[2 * (t0 / kTile)]);
        far_ilo = __builtin_amdgcn_readfirstlane(w.far_range[2 * (t0 / kTile) + 1]);
    }
    const size_t row = (size_t)d * n_lines;
    const WideScan* __restrict__ scan_row = w.wscan + row;
    const WideScan* __restrict__ hscan_row = w.hscan + row;
    const WideRec* __restrict__ rec_row = w.wrec + row;
    const WideSlow* __restrict__ slow_row = w.wslow + row;
    const WideRec32* __restrict__ rec32_row = MIXED ? w.wrec32 + row : nullptr;
    const int n_h = w.hlist ? __builtin_amdgcn_readfirstlane(*w.hcount) : 0;
    int pending32 = 0;  // fp32 terms accumulated since the last flush into the fp64 sums
#ifdef SDX_WALK_STATS
    const unsigned long long st_t0 = wall_clock64();
    int st_chunks = 0, st_fast = 0, st_general = 0, st_if = 0, st_slow = 0, st_flush = 0;  // (st_flush: ticks spent evaluating queued hits)
#endif

    // With a far field the hits that remain are few (the near zone of a line, window edges, cores: ~1 per chunk of 64 candidates
    // at S-c3 where the direct walk met 14), and a wave that fetches the record of every hit where it meets it is one dependent
    // round trip after the other (measured: 3.4 us per chunk).  The fp64 kernels with a far field therefore QUEUE their hits in LDS —
    // line index + test-free flag, list order — and evaluate a full queue (64 hits) at once: lane j fetches hit j's record and scan
    // word, all in one round trip, into LDS; the wave then goes through them with broadcast reads.  Same hits, same order, same
    // arithmetic as the direct walk.
    constexpr bool QUEUED = FAR && !MIXED && SDX_WIDE_QUEUED;
    constexpr int kLdsStride = QUEUED ? kWideFarLdsDoubles : kWideLdsDoubles;
    [[maybe_unused]] WideRec* const q_rec = reinterpret_cast<WideRec*>(lds_all + (size_t)split * kLdsStride);  // 64 x 48 B
    [[maybe_unused]] WideScan* const q_sc = reinterpret_cast<WideScan*>(lds_all + (size_t)split * kLdsStride + 64 * 6);
    [[maybe_unused]] int* const q_ent = reinterpret_cast<int*>(lds_all + (size_t)split * kLdsStride + 64 * 8);
    [[maybe_unused]] int q_count = 0;
    [[maybe_unused]] auto q_flush = [&](int cnt) {
      if constexpr (QUEUED) {
        if (cnt == 0) return;
        wave_sync();
        const bool mine = lane < cnt;
        const int ent = mine ? q_ent[lane] : 0;
        const int ql = ent & 0x7FFFFFFF;
        if (mine) {
            q_rec[lane] = rec_row[ql];
            q_sc[lane] = scan_row[ql];
        }
        const unsigned long long mfq = __ballot(mine && ent < 0);
        wave_sync();
        for (int k = 0; k < cnt; ++k) {
            const WideRec cur = q_rec[k];  // (one address for the whole wave: a broadcast read)
            const RegionI k1 = {cur.yk, cur.cv, cur.cd};
            const double c0 = (nu_base_vec - cur.lnu) * cur.inv;
            if ((mfq >> k) & 1) {
                region1_add_shared<R>(acc, dnu, cur.inv, c0, k1);
#ifdef SDX_WALK_STATS
                ++st_fast;
#endif
                continue;
            }
#ifdef SDX_WALK_STATS
            ++st_general;
#endif
            // the tile touches a window edge or the core (the direct walk below has the commentary)
            const WideScan hs = q_sc[k];
            const int jlo = __builtin_amdgcn_readfirstlane(hs.lo), jhi = __builtin_amdgcn_readfirstlane(hs.hi);
            const int jc = __builtin_amdgcn_readfirstlane(hs.clo), jchi = __builtin_amdgcn_readfirstlane(hs.chi);
            const bool delegated = jc < 0;
            const int jclo = delegated ? -jc - 1 : jc;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int a = it0 + 64 * r, z = min(a + 64, it1);
                if (z <= jlo || a >= jhi || a >= it1) continue;
                const bool over_core = !(z <= jclo || a >= jchi);
#ifdef SDX_WALK_STATS
                if (!over_core || delegated) ++st_if; else ++st_slow;
#endif
                if (!over_core || delegated) {
                    const int ir = idx0 + 64 * r;
                    const bool take = ir >= jlo && ir < jhi && !(over_core && ir >= jclo && ir < jchi);
                    acc[r] = region1_add_if(acc[r], fma(dnu[MIXED ? 0 : r], cur.inv, c0), k1, take);
                } else {
                    const WideSlow sl = slow_row[__builtin_amdgcn_readlane(ql, k)];
                    if (idx0 + 64 * r >= jlo && idx0 + 64 * r < jhi) acc[r] = voigt_add_x(acc[r], fma(dnu[MIXED ? 0 : r], cur.inv, c0), sl.y, sl.amp, k1);
                }
            }
        }
        wave_sync();  // (the queue and the staged records are written again)
      }
    };

    for (int pass = w.hlist ? 0 : 1; pass < 2; ++pass) {
        // candidate positions [ka, kb) of this pass: hlist positions (pass 0); wlist positions or — short lists — line indices (pass 1)
        int ka = 0, kb = n_h;
        // short lists with a compacted candidate list: this subset's own list, chunk after chunk — the lines it would meet as
        // possible hits scanning every chunk q = split (mod n_split) of the whole list, in the same order
        const int* clist_s = nullptr;
        int q_step = n_split;
        if (pass == 1) {
            kb = (int)n_lines;
            if constexpr (LISTED && !MIXED) if (!w.hlist && w.n_csplit) {
                const int* const ccount = wide_list_counts(w);
                kb = __builtin_amdgcn_readfirstlane(ccount[split]);
                clist_s = wide_list_of(w, n_lines) + __builtin_amdgcn_readfirstlane(ccount[8 + split]);
                q_step = 1;
            }
            if (w.hlist) {  // lines whose centre c satisfies t0 - H < c < t1 + H: line indices [la, lb), wlist positions [wrank[la], wrank[lb])
                const int64_t pa = max(t0 - kMediumHalfWidth + 1, (int64_t)0), pb = min(t1 + kMediumHalfWidth - 1, n_nu);
                ka = __builtin_amdgcn_readfirstlane(w.wrank[w.cnt_ge[pb + 1]]);
                kb = __builtin_amdgcn_readfirstlane(w.wrank[w.cnt_ge[pa]]);
                // A culled shard has prepared only the wlist lines centred within kMediumHalfWidth of ITS OWN columns (range
                // blocks + xlist); a tile cut by the shard boundary reaches up to kTile - 1 points further, and the records of the
                // lines centred out there are whatever the workspace held.  None of them can reach a STORED column (half-width <=
                // kMediumHalfWidth), and a candidate's subset is its position in wlist, so leaving them out changes no stored bit.
                if (w.sel) {
                    ka = max(ka, __builtin_amdgcn_readfirstlane(w.wrank[w.sel[0]]));
                    kb = min(kb, __builtin_amdgcn_readfirstlane(w.wrank[w.sel[1]]));
                }
            }
        }
        if (kb <= ka) continue;
        const int q_first = ka >> 6, q_last = (kb - 1) >> 6;
        int q = clist_s ? 0 : q_first + ((split - q_first % n_split) + n_split) % n_split;  // first chunk >= q_first of this subset
        // the scan word of the NEXT chunk is requested behind the current chunk's arithmetic
        auto fetch = [&](int qq, int& line, WideScan& sc) {
            const int k = qq * 64 + lane;
            line = -1;
            sc = WideScan{0, 0, 0, 0};
            if (qq <= q_last && k >= ka && k < kb) {
                if (pass == 0) {
                    line = w.hlist[k];
                    sc = w.hscan ? hscan_row[k] : scan_row[line];
                } else {
                    line = w.hlist ? w.wlist[k] : (clist_s ? clist_s[k] : k);
                    sc = scan_row[line];
                }
            }
        };
        if constexpr (QUEUED) {
            // the scan of a queued walk has nothing to wait for but its own loads: kScanBatch chunks are requested together (a chunk is
            // two dependent loads in the wlist pass), tested, and their hits appended in list order
            constexpr int kScanBatch = SDX_SCAN_BATCH;
            for (; q <= q_last; q += kScanBatch * q_step) {
                int bl[kScanBatch];
                WideScan bs[kScanBatch];
#pragma unroll
                for (int u = 0; u < kScanBatch; ++u) fetch(q + u * q_step, bl[u], bs[u]);
#pragma unroll
                for (int u = 0; u < kScanBatch; ++u) {
                    const int line = bl[u];
                    const WideScan sc = bs[u];
                    const bool far = far_eligible(sc, it0, it1, far_ihi, far_ilo);  // the far role's
                    const bool hit = (line >= 0) & (sc.lo < it1) & (sc.hi > it0) & !far;
                    const int clo = sc.clo < 0 ? -sc.clo - 1 : sc.clo;
                    const bool fast = hit & (sc.lo <= it0) & (sc.hi >= it1) & ((it1 <= clo) | (it0 >= sc.chi));
                    const unsigned long long m = __ballot(hit);
#ifdef SDX_WALK_STATS
                    if (q + u * q_step <= q_last) ++st_chunks;
#endif
                    if (m == 0) continue;
                    const int n = __popcll(m);
                    if (q_count + n > 64) {
#ifdef SDX_WALK_STATS
                        const unsigned long long tq = wall_clock64();
#endif
                        q_flush(q_count);
#ifdef SDX_WALK_STATS
                        st_flush += (int)(wall_clock64() - tq);
#endif
                        q_count = 0;
                    }
                    if (hit) q_ent[q_count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = line | (fast ? (int)0x80000000 : 0);
                    q_count += n;
                }
            }
            continue;
        }
        int line_next;
        WideScan sc_next;
        fetch(q, line_next, sc_next);
        for (; q <= q_last; q += q_step) {
            const int line = line_next;
            const WideScan sc = sc_next;
            fetch(q + q_step, line_next, sc_next);
            const bool far = FAR && far_eligible(sc, it0, it1, far_ihi, far_ilo);  // the far role's
            const bool hit = (line >= 0) & (sc.lo < it1) & (sc.hi > it0) & !far;  // narrow / empty items have lo = hi = 0
            const int clo = sc.clo < 0 ? -sc.clo - 1 : sc.clo;                // sign: core delegated to the narrow role
            const bool fast = hit & (sc.lo <= it0) & (sc.hi >= it1) & ((it1 <= clo) | (it0 >= sc.chi));
            unsigned long long m = __ballot(hit);
#ifdef SDX_WALK_STATS
            ++st_chunks;
#endif
            if (m == 0) continue;
            const unsigned long long mf = __ballot(fast);
            if constexpr (MIXED) pending32 += __popcll(m);
            if constexpr (MIXED && STAGED) {
                // fp32-mixed mode, lists whose tiles find most of a chunk's candidates hitting (1e6 lines: 10 000 lines wider than
                // 4096 points, every tile walks them all): the hits of the chunk are COMPACTED — one wave permutation puts hit j's line index, lane and
                // test-free flag into lane j — and lane j fetches hit j's 32-byte fp32 record and stages it in LDS.  The walk is
                // then over hit ordinals: a run of test-free hits is a counted loop whose records arrive by broadcast LDS reads,
                // two per trip — no mask arithmetic, no address arithmetic, no scalar load per hit.  (Round 4's walk fetched every
                // record with scalar loads: ~20 scalar instructions per hit — lowest set bit, read-lane, 64-bit address, two
                // s_load, the test for the next hit — next to ~19 vector ones.)  Same records, same order, same pairing of the fp32
                // sums: the bits of the scalar walk.  Measured in round 5 (two builds, alternating): the line kernel of the 1e6-line
                // list 7.59 -> 6.70 ms, that of the 1.5e5-line list 1.60 -> 1.69 ms (a few hits per chunk: the staging of a chunk —
                // three permutations, a gathered load, two hand-overs through LDS — costs more than its scalar fetches) — hence only
                // in the kernel that very dense lists run.
                WideRec32* const stage = reinterpret_cast<WideRec32*>(lds_all + (size_t)split * kWideLdsDoubles);  // 64 x 32 B of this wave's LDS
                const int n_hits = __popcll(m);
                const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));  // hit lanes below this one
                const int dst = (hit ? below : n_hits + (lane - below)) << 2;  // a permutation: the hits first, in order
                const int line_c = __builtin_amdgcn_ds_permute(dst, line);
                const int lane_c = __builtin_amdgcn_ds_permute(dst, lane);
                const int fast_c = __builtin_amdgcn_ds_permute(dst, fast ? 1 : 0);
                const unsigned long long fast_o = __ballot(fast_c != 0);  // bit j: hit j is test-free
                if (lane < n_hits) stage[lane] = rec32_row[line_c];
                wave_sync();
                int k = 0;
                while (k < n_hits) {
                    const unsigned long long rest = ~(fast_o >> k);
                    const int run = rest ? __builtin_ctzll(rest) : 64;  // test-free hits from ordinal k on
                    for (int j = 0; j < run; j += 2) {
                        // two hits per trip; an odd last one runs a second time with a zero amplitude (adds exactly 0)
                        const bool two = j + 1 < run;
                        const WideRec32 ra = stage[k + j];
                        WideRec32 rb = stage[k + j + (two ? 1 : 0)];
                        rb.yk = two ? rb.yk : 0.f;
                        const float ca = region1_c0(base_h, ra), cb = region1_c0(base_h, rb);
#pragma unroll
                        for (int r = 0; r < R / 2; ++r) {
                            acc32[r] = region1_f32x2(acc32[r], dq[r], ca, ra);
                            acc32[r] = region1_f32x2(acc32[r], dq[r], cb, rb);
                        }
                    }
                    k += run;
                    if (k >= n_hits) break;
                    // hit k touches a window edge or the core (the fp64 branch below has the commentary)
                    const int b = __builtin_amdgcn_readlane(lane_c, k);
                    const int e = __builtin_amdgcn_readlane(line_c, k);
                    ++k;
                    const WideRec cur = rec_row[e];
                    const WideRec32 cur32 = rec32_row[e];
                    const int jlo = __builtin_amdgcn_readlane(sc.lo, b), jhi = __builtin_amdgcn_readlane(sc.hi, b);
                    const int jc = __builtin_amdgcn_readlane(sc.clo, b), jchi = __builtin_amdgcn_readlane(sc.chi, b);
                    const bool delegated = jc < 0;
                    const int jclo = delegated ? -jc - 1 : jc;
                    const RegionI k1 = {cur.yk, cur.cv, cur.cd};
                    float2v term32[R / 2];  // sum + fp32 rational of every point pair, once per hit
                    const float c32 = region1_c0(base_h, cur32);
#pragma unroll
                    for (int p = 0; p < R / 2; ++p) term32[p] = region1_f32x2(acc32[p], dq[p], c32, cur32);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int a = it0 + 64 * r, z = min(a + 64, it1);
                        if (z <= jlo || a >= jhi || a >= it1) continue;
                        const bool over_core = !(z <= jclo || a >= jchi);
                        if (!over_core || delegated) {
                            const int ir = idx0 + 64 * r;
                            const bool take = ir >= jlo && ir < jhi && !(over_core && ir >= jclo && ir < jchi);
                            acc32[r >> 1][r & 1] = take ? term32[r >> 1][r & 1] : acc32[r >> 1][r & 1];
                        } else {
                            const WideSlow sl = slow_row[e];
                            if (idx0 + 64 * r >= jlo && idx0 + 64 * r < jhi) {
                                const double nu_r = nus[(int64_t)idx0 + 64 * r];  // (a core kept by the wide role: rare; the exact frequency)
                                acc[r] = voigt_add(acc[r], nu_r - cur.lnu, cur.inv, sl.y, sl.amp, k1);
                            }
                        }
                    }
                }
                wave_sync();  // (the next chunk's records go into the same LDS)
                if (pending32 >= 48) {
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r] += (double)acc32[r >> 1][r & 1], acc32[r >> 1][r & 1] = 0.f;
                    pending32 = 0;
                }
                continue;
            }
            // walk the hits in ascending order.  The record is fetched with scalar loads straight into SGPRs, which the fp64
            // instructions take as operands (one each): no copy, no vector registers.  Its latency is not hidden by a
            // software prefetch — carrying a record across iterations makes the compiler park it in 12 VGPRs and move it
            // there with six v_mov per hit — but by the other waves of the SIMD.
            for (;;) {
                // A run of test-free hits (every point of the tile inside the window and in region I: the operations of
                // voigt_add's region-I branch, bit-identical, or the fp32 rational of the mixed-precision mode) is a loop of
                // its own — a single basic block, so the sums stay in their registers; as one arm of an if / else with the
                // general case the compiler forms them in fresh registers and copies them back, five v_mov_b64 per hit.
                while ((m & (0ull - m)) & mf) {
                    const int e = __builtin_amdgcn_readlane(line, __builtin_ctzll(m));
                    const unsigned long long m1 = m & (m - 1);
                    if constexpr (MIXED) {
                        // two test-free hits per trip: both 32-byte records are requested together (one wait instead of
                        // two — the fp32 arithmetic is short enough for the record fetch to show), the sums keep list order.
                        // When the next hit is not test-free the second evaluation runs on the first record again with a
                        // zero amplitude (a scalar select; adds exactly 0): the loop stays one basic block
                        const bool two = ((m1 & (0ull - m1)) & mf) != 0;
                        const int e1 = __builtin_amdgcn_readlane(line, __builtin_ctzll(two ? m1 : m));
                        const WideRec32 ra = rec32_row[e];
                        WideRec32 rb = rec32_row[e1];
                        rb.yk = two ? rb.yk : 0.f;
                        const float ca = region1_c0(base_h, ra), cb = region1_c0(base_h, rb);
#pragma unroll
                        for (int r = 0; r < R / 2; ++r) {
                            acc32[r] = region1_f32x2(acc32[r], dq[r], ca, ra);
                            acc32[r] = region1_f32x2(acc32[r], dq[r], cb, rb);
                        }
                        m = two ? (m1 & (m1 - 1)) : m1;
                        continue;
                    } else {
                        const WideRec cur = rec_row[e];
                        const RegionI k1 = {cur.yk, cur.cv, cur.cd};
                        const double c0 = (nu_base_vec - cur.lnu) * cur.inv;
                        region1_add_shared<R>(acc, dnu, cur.inv, c0, k1);
                    }
#ifdef SDX_WALK_STATS
                    ++st_fast;
#endif
                    m = m1;
                }
                if (!m) break;
                const int b = __builtin_ctzll(m);
                const int e = __builtin_amdgcn_readlane(line, b);
                const WideRec cur = rec_row[e];
                WideRec32 cur32;
                if (MIXED) cur32 = rec32_row[e];
                m &= m - 1;
#ifdef SDX_WALK_STATS
                ++st_general;
#endif
                {
                    // The tile touches a window edge or the core.  Per 64-point block r (scalar tests): outside the window:
                    // nothing; clear of the core: the region-I rational for the whole block, added where the point is
                    // inside the window; over a DELEGATED core: the same, minus the core points (the narrow role adds
                    // them); over a core kept here (wider than a narrow window): the full Voigt term per point.
                    const int jlo = __builtin_amdgcn_readlane(sc.lo, b), jhi = __builtin_amdgcn_readlane(sc.hi, b);
                    const int jc = __builtin_amdgcn_readlane(sc.clo, b), jchi = __builtin_amdgcn_readlane(sc.chi, b);
                    const bool delegated = jc < 0;
                    const int jclo = delegated ? -jc - 1 : jc;
                    const RegionI k1 = {cur.yk, cur.cv, cur.cd};
                    const double c0 = (nu_base_vec - cur.lnu) * cur.inv;
                    float2v term32[MIXED ? R / 2 : 1];  // mixed mode: sum + fp32 rational of every point pair, once per hit
                    if constexpr (MIXED) {
                        const float c32 = region1_c0(base_h, cur32);
#pragma unroll
                        for (int p = 0; p < R / 2; ++p) term32[p] = region1_f32x2(acc32[p], dq[p], c32, cur32);
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int a = it0 + 64 * r, z = min(a + 64, it1);
                        if (z <= jlo || a >= jhi || a >= it1) continue;
                        const bool over_core = !(z <= jclo || a >= jchi);
#ifdef SDX_WALK_STATS
                        if (!over_core || delegated) ++st_if; else ++st_slow;
#endif
                        if (!over_core || delegated) {
                            const int ir = idx0 + 64 * r;  // (points beyond the grid's end lie beyond every window: jhi <= N_nu)
                            const bool take = ir >= jlo && ir < jhi && !(over_core && ir >= jclo && ir < jchi);
                            if constexpr (MIXED) {  // the tolerance path evaluates window edges in fp32 too (pairs of blocks)
                                acc32[r >> 1][r & 1] = take ? term32[r >> 1][r & 1] : acc32[r >> 1][r & 1];
                            } else {
                                acc[r] = region1_add_if(acc[r], fma(dnu[MIXED ? 0 : r], cur.inv, c0), k1, take);
                            }
                        } else {
                            const WideSlow sl = slow_row[e];
                            if (idx0 + 64 * r >= jlo && idx0 + 64 * r < jhi) {
                                if constexpr (MIXED) {
                                    const double nu_r = nus[(int64_t)idx0 + 64 * r];  // (a core kept by the wide role: rare; the exact frequency)
                                    acc[r] = voigt_add(acc[r], nu_r - cur.lnu, cur.inv, sl.y, sl.amp, k1);
                                } else {
                                    // x from the tile offsets like every other point of the tile (a core kept here is wider than 128
                                    // points: |c0| stays below ~50, x is good to 1e-14 absolute) — forming nu_i = dnu + nu_base instead
                                    // made the compiler hoist four sums out of the walk and spill them to scratch in every wave
                                    acc[r] = voigt_add_x(acc[r], fma(dnu[MIXED ? 0 : r], cur.inv, c0), sl.y, sl.amp, k1);
                                }
                            }
                        }
                    }
                }
                if (!m) break;
            }
            if constexpr (MIXED) {
                // the fp32 running sums go into the fp64 sums once ~64 terms have gathered (checked per chunk, not per hit: a
                // branch around the fp64 accumulators inside the walk costs eight register copies per hit)
                if (pending32 >= 48) {
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r] += (double)acc32[r >> 1][r & 1], acc32[r >> 1][r & 1] = 0.f;
                    pending32 = 0;
                }
            }
        }
    }
#ifdef SDX_WALK_STATS
    const unsigned long long tq_last = wall_clock64();
#endif
    if constexpr (QUEUED) q_flush(q_count);
#ifdef SDX_WALK_STATS
    st_flush += (int)(wall_clock64() - tq_last);
#endif
    if constexpr (MIXED) {
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += (double)acc32[r >> 1][r & 1];
    }
#ifdef SDX_WALK_STATS
    if (lane == 0) {  // (a device array read back by sdx_walk_stats_read: printf's host calls slowed the whole launch a thousandfold)
        const int slot = ((d * 512 + tile_idx) * 8 + split) & (kWalkStatSlots / 2 - 1);
        unsigned long long* const o = g_walk_stats + (size_t)slot * 8;
        o[0] = ((unsigned long long)d << 40) | ((unsigned long long)tile_idx << 8) | (unsigned long long)split | (1ull << 63);
        o[1] = st_t0, o[2] = wall_clock64(), o[3] = (unsigned long long)st_chunks | ((unsigned long long)(unsigned)st_flush << 32), o[4] = st_fast, o[5] = st_general, o[6] = st_if, o[7] = st_slow;
    }
#endif
    if constexpr (DEFER) {
#pragma unroll
        for (int r = 0; r < R; ++r) acc_out[r] = acc[r];
    } else {
        wide_reduce_and_store<R, kLdsStride>(split, n_split, acc, idx0, s0, s1, lds_all, plane, pld, d);
    }
}

// Long line lists: two stable compactions of the per-line classes in two small launches (per-block counts, then every
// block sums the counts before it — a few hundred integers — and scatters its own lines):
//   hlist  the lines whose widest window exceeds kMediumHalfWidth (they may reach any tile: every tile visits them all)
//   wlist  the other lines with a wide window at some depth, + wrank[l] = wlist entries below line l
constexpr int kHlistBlock = 1024;
__device__ __forceinline__ int line_class(int whw) { return whw > kMediumHalfWidth ? 2 : (whw > kNarrowHalfWidth ? 1 : 0); }

// (xlist: the class-1 lines of [sel[0], sel[1]) outside the blocks of pre_lines consecutive lines that cover [sel[2], sel[3]))
__device__ __forceinline__ bool in_xlist(int64_t l, int cls, const int* __restrict__ sel, int pre_lines)
{
    if (!sel || cls != 1) return false;
    const int ra = sel[2] / pre_lines * pre_lines, rb = (sel[3] + pre_lines - 1) / pre_lines * pre_lines;
    return l >= sel[0] && l < sel[1] && !(sel[3] > sel[2] && l >= ra && l < rb);
}

// the window half-width of the largest (gamma + dw) alpha of a line (:561-575; NaN or negative: the 10-point floor)
__device__ __forceinline__ int half_width_of(double m, double d_nu, int64_t n_nu)
{
    const double pixels = mul_rn(m / d_nu, 20.0);
    const double forced = pixels > 10.0 ? pixels : 10.0;
    return (int)(forced >= (double)n_nu ? n_nu : (int64_t)forced);
}
// (culled runs: the class comes from the classification pass's largest (gamma + dw) alpha per line and the grid spacing)
struct ClassSource {
    const int* whw_max;       // per line, from a full pre-pass; or nullptr:
    const double* m_max;      // per line, from k_classify
    const double* dnu_partial;
    int n_partial;
    int64_t n_nu;
};
__device__ __forceinline__ int class_of_line(const ClassSource& cs, int64_t l, double d_nu)
{
    return line_class(cs.whw_max ? cs.whw_max[l] : half_width_of(cs.m_max[l], d_nu, cs.n_nu));
}
__global__ __launch_bounds__(kHlistBlock) void k_hlist_count(int64_t n_lines, ClassSource cs, int* __restrict__ block_cnt,
                                                            const int* __restrict__ sel, int pre_lines, int* __restrict__ ticket)
{
    __shared__ int s_wave[3][kHlistBlock / 64];
    __shared__ double s_dnu[kHlistBlock / 64];
    if (ticket && blockIdx.x == 0 && threadIdx.x < 8) ticket[threadIdx.x] = 0;  // (the work counters of the pre-pass launch that follows)
    const double d_nu = cs.whw_max ? 0.0 : block_dnu(cs.dnu_partial, cs.n_partial, s_dnu);
    const int64_t l = (int64_t)blockIdx.x * kHlistBlock + threadIdx.x;
    const int cls = l < n_lines ? class_of_line(cs, l, d_nu) : 0;
    const unsigned long long mh = __ballot(cls == 2), mw = __ballot(cls == 1), mx = __ballot(in_xlist(l, cls, sel, pre_lines));
    if ((threadIdx.x & 63) == 0)
        s_wave[0][threadIdx.x >> 6] = __popcll(mh), s_wave[1][threadIdx.x >> 6] = __popcll(mw), s_wave[2][threadIdx.x >> 6] = __popcll(mx);
    __syncthreads();
    if (threadIdx.x < 3) {
        int tot = 0;
        for (int k = 0; k < kHlistBlock / 64; ++k) tot += s_wave[threadIdx.x][k];
        block_cnt[3 * blockIdx.x + threadIdx.x] = tot;
    }
}
__global__ __launch_bounds__(kHlistBlock) void k_hlist_scatter(int64_t n_lines, ClassSource cs, const int* __restrict__ block_cnt,
                                                              int* __restrict__ hlist, int* __restrict__ wlist, int* __restrict__ wrank,
                                                              int* __restrict__ hcount, int* __restrict__ xlist, const int* __restrict__ sel,
                                                              int pre_lines)
{
    __shared__ int s_wave[3][kHlistBlock / 64];
    __shared__ int s_red[3][kHlistBlock / 64];
    __shared__ double s_dnu[kHlistBlock / 64];
    const double d_nu = cs.whw_max ? 0.0 : block_dnu(cs.dnu_partial, cs.n_partial, s_dnu);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int bh = 0, bw = 0, bx = 0;
    for (int k = threadIdx.x; k < (int)blockIdx.x; k += kHlistBlock) bh += block_cnt[3 * k], bw += block_cnt[3 * k + 1], bx += block_cnt[3 * k + 2];
    for (int off = 32; off > 0; off >>= 1) bh += __shfl_xor(bh, off), bw += __shfl_xor(bw, off), bx += __shfl_xor(bx, off);
    const int64_t l = (int64_t)blockIdx.x * kHlistBlock + threadIdx.x;
    const int cls = l < n_lines ? class_of_line(cs, l, d_nu) : 0;
    const bool isx = in_xlist(l, cls, sel, pre_lines);
    const unsigned long long mh = __ballot(cls == 2), mw = __ballot(cls == 1), mx = __ballot(isx);
    if (lane == 0) {
        s_red[0][wave] = bh, s_red[1][wave] = bw, s_red[2][wave] = bx;
        s_wave[0][wave] = __popcll(mh), s_wave[1][wave] = __popcll(mw), s_wave[2][wave] = __popcll(mx);
    }
    __syncthreads();
    int base_h = 0, base_w = 0, base_x = 0;
    for (int k = 0; k < kHlistBlock / 64; ++k) base_h += s_red[0][k], base_w += s_red[1][k], base_x += s_red[2][k];
    for (int k = 0; k < wave; ++k) base_h += s_wave[0][k], base_w += s_wave[1][k], base_x += s_wave[2][k];
    const unsigned long long below = (1ull << lane) - 1ull;
    const int pos_h = base_h + __popcll(mh & below), pos_w = base_w + __popcll(mw & below), pos_x = base_x + __popcll(mx & below);
    if (cls == 2) hlist[pos_h] = (int)l;
    if (cls == 1) wlist[pos_w] = (int)l;
    if (isx) xlist[pos_x] = (int)l;
    if (l < n_lines) wrank[l] = pos_w;
    if (l == n_lines - 1) {
        wrank[n_lines] = pos_w + (cls == 1);
        hcount[0] = pos_h + (cls == 2);
        hcount[1] = pos_w + (cls == 1);
        hcount[2] = pos_x + (isx ? 1 : 0);
    }
}

// hscan[d][k] = wscan[d][hlist[k]]: every tile scans ALL the huge lines; gathering their 16-byte scan words through the
// list costs a 64-byte sector each.  Copied once into list order they are read as contiguous kilobytes.
__global__ __launch_bounds__(kBlock) void k_hscan(int n_depth, int64_t n_lines, const int* __restrict__ hlist, const int* __restrict__ hcount,
                                                  const WideScan* __restrict__ wscan, WideScan* __restrict__ hscan)
{
    const int n_h = hcount[0];
    const int d = blockIdx.y;
    for (int k = blockIdx.x * kBlock + threadIdx.x; k < n_h; k += gridDim.x * kBlock)
        hscan[(size_t)d * n_lines + k] = wscan[(size_t)d * n_lines + hlist[k]];
}

// sel[0..1] = [la, lb): the lines whose centre c satisfies begin - H < c < end + H for the columns [begin, end) of the shard's
// tiles and H = kMediumHalfWidth; sel[2..3] = [na, nb): the same for the shard's own columns with H = 2 kNarrowReach
// (centre_l = #{i : nus[i] >= line_nu_l}; lines ascend in frequency, so centres descend with the line index)
__device__ __forceinline__ void shard_range(int64_t n_nu, const double* __restrict__ nus, int64_t n_lines, const double* __restrict__ line_nus,
                                            int64_t nu_begin, int64_t nu_count, int* __restrict__ sel)
{
    // one WAVE per bound (the first four waves of the block), each a 64-ary search: three round trips to memory for 1.5e5 lines
    // where a thread's bisection makes seventeen — in the two-collective mode the classification launch is a few microseconds of
    // streaming, and the four chains of dependent loads were what it waited for (24 - 29 us on an eighth of S-c3)
    const int which = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (which >= 4) return;
    // lines with centre >= p  <=>  line_nu <= nus[p - 1]: their number is cnt_ge[p]
    const int64_t H = which < 2 ? kMediumHalfWidth : 2 * kNarrowReach;
    // ... [la, lb) for the shard's columns rounded out to whole TILES of the wide role (kMaxTile covers every tile width): a tile
    // cut by the shard boundary is walked whole, and its candidate list — with it the points at which the fp32-mixed mode folds its
    // running sums into the fp64 ones, which count the hits of the whole tile — must be the unsharded run's for the shard to
    // reproduce that run's bits in BOTH precisions (tests/test_gpu_long_random.py found mixed-mode shards a few 1e-8 apart)
    const int64_t ext = which < 2 ? kMaxTile - 1 : 0;
    const int64_t pa = max(nu_begin - ext - H + 1, (int64_t)0), pb = min(nu_begin + nu_count + ext + H - 1, n_nu);
    const int64_t p = (which & 1) == 0 ? pb + 1 : pa;  // sel[0] = cnt_ge[pb + 1], sel[1] = cnt_ge[pa]
    int64_t cnt;
    if (p == 0) cnt = n_lines;
    else if (p >= n_nu + 1) cnt = 0;
    else {
        const double v = nus[p - 1];
        int64_t lo = 0, hi = n_lines;  // the first l with line_nus[l] > v lies in [lo, hi]
        while (hi > lo) {
            const int64_t step = (hi - lo + 63) / 64;
            const int64_t idx = lo + (int64_t)lane * step;  // the lanes' probes ascend: `le` is true on a prefix of them
            const bool le = idx < hi && line_nus[idx] <= v;
            const int k = __popcll(__ballot(le));
            const int64_t base = lo;
            lo = k > 0 ? base + (int64_t)(k - 1) * step + 1 : base;
            hi = min(base + (int64_t)k * step, hi);
        }
        cnt = lo;
    }
    if (lane == 0) sel[which] = (int)cnt;
}

// Frequency-sharded runs of long lists, stage A: how wide the widest window of every line is (over all depths) — which lines can
// reach any column (-> hlist) or, from just outside the shard's own line range, its edge columns (-> xlist) — before the full
// pre-pass runs on the lines the shard needs.  The half-width of the window rule (:561-575), int(max(10, (gamma + dw) alpha / d_nu
// * 20)), is a non-decreasing function of m = (gamma + dw) alpha, so the widest window of a line is the window of its LARGEST m:
// this pass streams the dense inputs once and leaves max_d m per line; the list kernels apply the rule (they, not this pass,
// need the grid spacing — whose partial maxima the FIRST blocks of this launch compute on the side: one launch fewer per step).
// One wave per line at a time, lane <-> depth: a line's 56 values are one contiguous 448-byte request per array, the maximum is
// a wave reduction, the result a plain store — no atomics, nothing to clear beforehand.  (Round 3 accumulated integer half-widths
// with atomicMax behind a pre-filter that needed d_nu: k_dnu_partial had to run, and clear the maxima, before every step.)
// NaN terms are ignored (their window is the 10-point floor: never the widest).
constexpr int kClsLinesPerWave = 4;  // lines in flight per wave: 12 independent loads per lane
__device__ __forceinline__ void classify_block(const int bid, const int n_blocks, int n_depth, const int64_t cls_begin, const int64_t cls_end,
                                               const double* __restrict__ doppler, const double* __restrict__ gammas, int gamma_cols,
                                               const double* __restrict__ alphas, double* __restrict__ m_max)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    // the lines [cls_begin, cls_end) — the whole list, or this rank's share of it (two-collective mode: the ranks exchange their
    // shares of m_max) — in contiguous runs per block; a block's waves take consecutive groups of kClsLinesPerWave lines
    const int64_t per_block = (cls_end - cls_begin + n_blocks - 1) / n_blocks;
    const int64_t l0 = cls_begin + (int64_t)bid * per_block, l1 = min(l0 + per_block, cls_end);
    for (int64_t base = l0 + (int64_t)wave * kClsLinesPerWave; base < l1; base += (int64_t)n_waves * kClsLinesPerWave) {
        double m[kClsLinesPerWave];
#pragma unroll
        for (int j = 0; j < kClsLinesPerWave; ++j) m[j] = -INFINITY;
        for (int d = lane; d < n_depth; d += 64) {
            double dw[kClsLinesPerWave], al[kClsLinesPerWave], g[kClsLinesPerWave];
#pragma unroll
            for (int j = 0; j < kClsLinesPerWave; ++j) {
                const int64_t l = min(base + j, l1 - 1);  // (clamped: a repeated line changes nothing)
                dw[j] = doppler[l * n_depth + d];
                al[j] = alphas[l * n_depth + d];
                g[j] = gamma_cols > 1 ? gammas[l * gamma_cols + d] : gammas[l];
            }
#pragma unroll
            for (int j = 0; j < kClsLinesPerWave; ++j) m[j] = fmax(m[j], mul_rn(add_rn(g[j], dw[j]), al[j]));  // (fmax drops a NaN)
        }
#pragma unroll
        for (int j = 0; j < kClsLinesPerWave; ++j) {
            for (int off = 32; off > 0; off >>= 1) m[j] = fmax(m[j], __shfl_xor(m[j], off));
            if (lane == 0 && base + j < l1) m_max[base + j] = m[j];
        }
    }
}
// this block's share of max(diff(nus)) -> partial[bid]  (blocks [0, n_dnu) of the classification launches)
__device__ __forceinline__ void dnu_partial_block(const int bid, const int n_blocks, int64_t n_nu, const double* __restrict__ nus,
                                                  double* __restrict__ partial, double* s_red, const FarReq& far)
{
    far_ranges_block(bid, n_blocks, n_nu, nus, far);
    grid_sample_block(bid, n_blocks, n_nu, nus, partial + kGridSampleOffset);
    // four independent pairs of loads in flight per thread: the scan is a chain of round trips, not a stream (the grid sits in L2)
    double m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
    const int64_t step = (int64_t)n_blocks * blockDim.x;
    int64_t i = (int64_t)bid * blockDim.x + threadIdx.x;
    for (; i + 3 * step + 1 < n_nu; i += 4 * step) {
        const double a0 = nus[i], b0 = nus[i + 1], a1 = nus[i + step], b1 = nus[i + step + 1];
        const double a2 = nus[i + 2 * step], b2 = nus[i + 2 * step + 1], a3 = nus[i + 3 * step], b3 = nus[i + 3 * step + 1];
        m0 = fmax(m0, b0 - a0), m1 = fmax(m1, b1 - a1), m2 = fmax(m2, b2 - a2), m3 = fmax(m3, b3 - a3);
    }
    for (; i + 1 < n_nu; i += step) m0 = fmax(m0, nus[i + 1] - nus[i]);
    double m = fmax(fmax(m0, m1), fmax(m2, m3));
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, s_red[w]);
        partial[bid] = m;
    }
}

__global__ __launch_bounds__(kBlock) void k_classify(int n_dnu, int n_depth, int64_t n_nu, int64_t n_lines, double* __restrict__ dnu_partial,
                                                     const double* __restrict__ doppler, const double* __restrict__ gammas,
                                                     int gamma_cols, const double* __restrict__ alphas, double* __restrict__ m_max,
                                                     const double* __restrict__ nus, const double* __restrict__ line_nus, int64_t nu_begin,
                                                     int64_t nu_count, int* __restrict__ sel, int64_t cls_begin, int64_t cls_end, FarReq far)
{
    __shared__ double s_red[kBlock / 64];
    const int b = blockIdx.x;
    if (b < n_dnu) {
        dnu_partial_block(b, n_dnu, n_nu, nus, dnu_partial, s_red, far);
        return;
    }
    // four threads of the LAST block find the shard's line ranges on the side (four binary searches: chains of dependent loads
    // that vanish behind this stream)
    if (sel && b == (int)gridDim.x - 1) shard_range(n_nu, nus, n_lines, line_nus, nu_begin, nu_count, sel);
    classify_block(b - n_dnu, (int)gridDim.x - n_dnu, n_depth, cls_begin, cls_end, doppler, gammas, gamma_cols, alphas, m_max);
}


// Narrow windows (half-width <= kNarrowHalfWidth, e.g. the reference's 10-pixel floor for weak lines, :565-567):
// a 256-point tile would be almost empty for them.  Here a wave owns ONE frequency and its lanes are the depth
// points (lane <-> depth, line-major parameter arrays so the loads coalesce): a weak line covers either all
// depths of that frequency or none, and all lanes share x = (nu_i - nu_l)/doppler up to the slowly varying Doppler
// width, so the Faddeeva region rarely diverges inside a wave.  The candidate lines of a frequency are the
// contiguous index range whose centre lies within kNarrowHalfWidth of it, read from cnt_ge; each lane walks that
// range in ascending line order, tests its own window and accumulates in a register.  Deterministic, no atomics.
// (This is what line_narrow_walk<1, false, false> below would be, as text of its own — a wave past the shard's end returns instead of
// keeping act[], and SDX_WALK_STATS counts here.  Folding it into the walk was tried in three spellings: the four fp64 kernels without
// subsets kept their registers, spills and occupancy and their bits, with a reordered schedule, and k_line_all ran 1217.9 us at S-c3
// against the parent's 1213.2 - 1215.2 in seven alternated rounds: it stays, profiles/EXPERIMENTS.md.)
__device__ __forceinline__ void line_narrow_wave(const int64_t i, const int depth_chunk, int n_depth, int64_t n_nu, const double* __restrict__ nus,
                                                        int64_t nu_begin, int64_t nu_count, int64_t n_lines,
                                                        const double* __restrict__ line_nus, LineWork w,
                                                        double* __restrict__ plane, int64_t pld)
{
    const int lane = threadIdx.x & 63;
    if (i >= nu_begin + nu_count) return;
    const int d = depth_chunk * 64 + lane;
    const bool valid = d < n_depth;
    const int dc = valid ? d : n_depth - 1;
    const unsigned dcu = (unsigned)dc;
    const bool one_gamma = w.narrow_raw == 1;  // (raw inputs with gammas (N_l, 1): the line's one value for every depth)
    const int ii = (int)i;
    // lines with centre c in [i - H + 1, i + H]
    const int64_t pa = max(i - kNarrowReach + 1, (int64_t)0);
    const int64_t pb = min(i + kNarrowReach, n_nu);
    const int la = __builtin_amdgcn_readfirstlane(w.cnt_ge[pb + 1]);
    const int lb = __builtin_amdgcn_readfirstlane(w.cnt_ge[pa]);
    const double nu_i = nus[i];
    double acc = 0.0;
#ifdef SDX_WALK_STATS
    const unsigned long long st_t0 = wall_clock64();
    int st_chunks = 0, st_rel = 0, st_eval = 0;
#endif
    for (int base = la; base < lb; base += 64) {
        // lanes test 64 candidate lines at once against this frequency (per-line bound), then the wave visits
        // only the relevant ones, in ascending line order
        const int lc = base + lane;
        bool rel = false;
        int c = 0;
        if (lc < lb) {
            const int hwm = w.nhw_max[lc];
            c = w.centre[lc];
            rel = hwm > 0 && ii >= c - hwm && ii < c + hwm;
        }
        unsigned long long m = __ballot(rel);
#ifdef SDX_WALK_STATS
        ++st_chunks, st_rel += __popcll(m);
#endif
        // the parameters of the NEXT relevant line are requested before the current one is evaluated (all six loads at
        // once, used or not): one global-memory round trip per line hides behind the previous line's arithmetic.  (Two lines in
        // flight — pairs — and the next chunk's candidates requested ahead were measured in round 4: 24.4 against 24.2 us for the
        // role alone at S-c2, 37.1 against 37.0 together: a wave's line takes ~1 us because seven waves share the SIMD's
        // arithmetic, not because it waits for memory.)
        int h = 0, cl = 0;  // this depth's half-width, the line's centre (scalar)
        double y = 0.0, amp = 0.0, inv = 0.0, lnu = 0.0;
        // addresses: a per-line base (uniform: scalar arithmetic) + the lane's depth as an unsigned 32-bit offset
        if (m) {
            const int bit = __builtin_ctzll(m);
            const int l = base + bit;
            const size_t ob = (size_t)l * n_depth;
            cl = __builtin_amdgcn_readlane(c, bit);
            h = (w.nhw + ob)[dcu], y = (w.n_y + (one_gamma ? (size_t)l : ob))[one_gamma ? 0u : dcu], amp = (w.n_amp + ob)[dcu], inv = (w.n_inv + ob)[dcu], lnu = line_nus[l];
        }
        while (m) {
            m &= m - 1;
            int h_n = 0, cl_n = 0;
            double y_n = 0.0, amp_n = 0.0, inv_n = 0.0, lnu_n = 0.0;
            if (m) {
                const int bit = __builtin_ctzll(m);
                const int l = base + bit;
                const size_t ob = (size_t)l * n_depth;
                cl_n = __builtin_amdgcn_readlane(c, bit);
                h_n = (w.nhw + ob)[dcu], y_n = (w.n_y + (one_gamma ? (size_t)l : ob))[one_gamma ? 0u : dcu], amp_n = (w.n_amp + ob)[dcu], inv_n = (w.n_inv + ob)[dcu], lnu_n = line_nus[l];
            }
#ifdef SDX_WALK_STATS
            if (__ballot(valid && ii >= cl - h && ii < cl + h)) ++st_eval;
#endif
            if (valid && ii >= cl - h && ii < cl + h) {  // (h = 0: empty)
                if (w.narrow_raw) narrow_params(inv, y, amp, inv, y, amp);  // (inv, y, amp hold dw, gamma, alpha)
                const RegionI k1 = region1_setup(y, amp);
                acc = voigt_add(acc, nu_i - lnu, inv, y, amp, k1);
            }
            h = h_n, cl = cl_n, y = y_n, amp = amp_n, inv = inv_n, lnu = lnu_n;
        }
    }
#ifdef SDX_WALK_STATS
    if (lane == 0) {
        const int slot = (int)(kWalkStatSlots / 2 + (i & (kWalkStatSlots / 2 - 1)));
        unsigned long long* const o = g_walk_stats + (size_t)slot * 8;
        o[0] = (unsigned long long)i | (3ull << 62);
        o[1] = st_t0, o[2] = wall_clock64(), o[3] = st_chunks, o[4] = st_rel, o[5] = st_eval, o[6] = 0, o[7] = 0;
    }
#endif
    if (valid) plane[(size_t)d * pld + (i - nu_begin)] = acc;
}

// The same walk for F CONSECUTIVE frequencies per wave (F = 2, 4; groups aligned to the global grid index), in all its forms:
// line_narrow_walk<F, SUB, F32> — the frequencies per wave, whether the wave walks one of four line subsets, and the arithmetic
// (fp64 records, or the mixed-precision mode's fp32 ones).  The forms differ in the four places marked (1) - (4) below and nowhere else.
//
// F frequencies per wave: the records of a visited line — five coalesced loads, 1.9 KB per wave — serve up to F evaluations
// instead of one, the candidate test and the region-I constants are shared, and a lane has F independent evaluations in flight.
// At 1e6 lines the one-frequency walk fetched 16 GB per launch through its record loads (each of the ~20 frequencies of a weak
// line's window loaded them again, and 900 waves per XCD, each with its own 170 lines, do not fit the L2); a group fetches a line's
// records once.  Every frequency still adds its lines in ascending line order: the bits are those of the one-frequency walk,
// whatever F — which may therefore depend on the size of the launch (small grids keep F = 1: they need the waves).
//
// SUB, the narrow role of DENSE long lists (at least one line per two grid points, four line subsets): the four waves of a workgroup
// share ONE group of F consecutive frequencies and split its candidate lines — wave s takes the lines l with (l / 16) % 4 == s,
// sixteen-line runs of the LIST going round the waves, so every wave gets a quarter of every stretch of the list — and the four
// partial sums meet in LDS, where wave 0 adds them in subset order.  A wave still fetches a visited line's records once for up to
// F evaluations (what F = 4 frequencies per wave saved: a third of the role's instructions and three quarters of its fetch), but
// there are as many waves as with one frequency per wave: a frequency SHARD of 11 000 - 21 000 columns fills the chip (round 4 had
// to fall back to one frequency per wave there: 3 000 four-times-longer waves are a launch's tail).  Which lines share a partial
// sum is a property of the list (the run index of a line), so shards reproduce the unsharded bits; the sums differ from the
// sequential walk's in the last bits (four partial sums instead of one).
//
// F32, the narrow role of the mixed-precision mode: every term evaluated by voigt_add32 (packed fp32, all four regions) from fp32
// records; the frequency difference comes from the hi + lo float pairs of both frequencies (exact to 2^-48 of the frequency, i.e.
// ~1e-7 of a narrow window's reach), the terms of one trip — 64 candidates — gather in an fp32 sum that goes into the fp64 sum once
// per trip.

// (1) lane -> candidate: line j of a trip that starts at base.  64 contiguous lines per trip; SUB: the 64 lines of this subset out of a
// stretch of 256 aligned to the LIST (lanes ascend with the line index)
#define SDX_NARROW_LINE(base, j) (SUB ? base + ((j >> 4) << 6) + (subset << 4) + (j & 15) : base + j)
// The records of the lowest line of m into h##S, cl##S, ...: this depth's half-width, the line's centre (scalar), and (3).  fp64 addresses:
// a per-line base (uniform: scalar arithmetic) + the lane's depth as an unsigned 32-bit offset.  Both are local macros because only
// they give the instructions of the walks this one replaced: a lambda or an inline function, however spelled (results through
// references or in a struct, always_inline or not), reordered all twelve line kernels, the mapping alone the six SUBSETS ones.
#define SDX_NARROW_FETCH(S)                                                                                                                     \
    do {                                                                                                                                        \
        const int bit = __builtin_ctzll(m);                                                                                                     \
        const int l = SDX_NARROW_LINE(base, bit);                                                                                               \
        cl##S = __builtin_amdgcn_readlane(c, bit);                                                                                              \
        if constexpr (F32) {                                                                                                                    \
            const size_t o = (size_t)l * n_depth + dc;                                                                                          \
            h##S = w.nhw[o], y##S = w.n_y32[o], amp##S = w.n_amp32[o], inv##S = w.n_inv32[o], lnu##S = w.lnu32[l];                              \
        } else {                                                                                                                                \
            const size_t ob = (size_t)l * n_depth;                                                                                              \
            h##S = (w.nhw + ob)[dcu], y##S = (w.n_y + (one_gamma ? (size_t)l : ob))[one_gamma ? 0u : dcu], amp##S = (w.n_amp + ob)[dcu],        \
            inv##S = (w.n_inv + ob)[dcu], lnu##S = line_nus[l];                                                                                 \
        }                                                                                                                                       \
    } while (0)
template <int F, bool SUB, bool F32>
__device__ __forceinline__ void line_narrow_walk(const int64_t i0, const int depth_chunk, const int subset, int n_depth, int64_t n_nu,
                                                 const double* __restrict__ nus, int64_t nu_begin, int64_t nu_count,
                                                 const double* __restrict__ line_nus, LineWork w, double* __restrict__ out, int64_t pld)
{
    constexpr int kStretch = SUB ? 256 : 64;
    // (2) where the first trip starts.  At the list's own stretches (base = kStretch k) wherever the stretch a line falls into decides
    // which partial sum its term joins — SUB: the run index of a line; F32: the fp32 sum of a trip, folded into the fp64 sum once per
    // trip — because which terms share a sum must not depend on where the candidate range of a frequency, or of a group of F
    // frequencies, happens to start: F follows the launch's width, and a shard's differs from the whole grid's.  The sequential
    // fp64 sum has no such groups and starts at its first candidate.
    constexpr bool kListAligned = SUB || F32;
    // (3) the records and the term: fp64 ones for region1_setup and voigt_add (raw inputs through narrow_params), or fp32 ones for
    // voigt_add32
    using Rec = std::conditional_t<F32, float, double>;
    using RecNu = std::conditional_t<F32, float2v, double>;
    const int lane = threadIdx.x & 63;
    const int d = depth_chunk * 64 + lane;
    const bool valid = d < n_depth;
    const int dc = valid ? d : n_depth - 1;
    [[maybe_unused]] const unsigned dcu = (unsigned)dc;
    [[maybe_unused]] const bool one_gamma = w.narrow_raw == 1;  // (raw inputs with gammas (N_l, 1): the line's one value for every depth)
    const int ia = (int)i0;
    // lines with centre c in [i0 - H + 1, i0 + F - 1 + H]
    const int64_t pa = max(i0 - kNarrowReach + 1, (int64_t)0);
    const int64_t pb = min(i0 + F - 1 + kNarrowReach, n_nu);
    const int la = __builtin_amdgcn_readfirstlane(w.cnt_ge[pb + 1]);
    const int lb = __builtin_amdgcn_readfirstlane(w.cnt_ge[pa]);
    [[maybe_unused]] double nu_k[F];
    [[maybe_unused]] float nih[F], nil[F];
    double acc[F];
    bool act[F];  // the frequency belongs to this launch's columns (wave-uniform)
#pragma unroll
    for (int k = 0; k < F; ++k) {
        act[k] = i0 + k >= nu_begin && i0 + k < nu_begin + nu_count;
        const double nu = nus[min(i0 + k, n_nu - 1)];
        if constexpr (F32) {
            nih[k] = (float)nu;
            nil[k] = (float)(nu - (double)nih[k]);
        } else {
            nu_k[k] = nu;
        }
        acc[k] = 0.0;
    }
    const int lane_off = SDX_NARROW_LINE(0, lane);
    for (int base = kListAligned ? la & ~(kStretch - 1) : la; base < lb; base += kStretch) {
        const int lc = base + lane_off;
        bool rel = false;
        int c = 0;
        if ((!kListAligned || lc >= la) && lc < lb) {
            const int hwm = w.nhw_max[lc];
            c = w.centre[lc];
            rel = hwm > 0 && ia + (F - 1) >= c - hwm && ia < c + hwm;
        }
        unsigned long long m = __ballot(rel);
        [[maybe_unused]] float acc32[F];
        if constexpr (F32) {
#pragma unroll
            for (int k = 0; k < F; ++k) acc32[k] = 0.f;
        }
        // the records of the NEXT relevant line are requested before the current one is evaluated (line_narrow_wave says why, and what
        // else was measured)
        int h = 0, cl = 0;
        Rec y = 0, amp = 0, inv = 0;
        RecNu lnu{};
        if (m) SDX_NARROW_FETCH();
        while (m) {
            m &= m - 1;
            int h_n = 0, cl_n = 0;
            Rec y_n = 0, amp_n = 0, inv_n = 0;
            RecNu lnu_n{};
            if (m) SDX_NARROW_FETCH(_n);
            const int lo = cl - h, hi = cl + h;  // (h = 0: empty; the clamp to the grid is implied by ia + k being a grid index)
            if (valid && ia + (F - 1) >= lo && ia < hi) {
                if constexpr (F32) {  // (3)
#pragma unroll
                    for (int k = 0; k < F; ++k)
                        if (act[k] && ia + k >= lo && ia + k < hi) acc32[k] = voigt_add32(acc32[k], ((nih[k] - lnu.x) + (nil[k] - lnu.y)) * inv, y, amp);
                } else {
                    if (w.narrow_raw) narrow_params(inv, y, amp, inv, y, amp);  // (inv, y, amp hold dw, gamma, alpha)
                    const RegionI k1 = region1_setup(y, amp);
#pragma unroll
                    for (int k = 0; k < F; ++k)
                        if (act[k] && ia + k >= lo && ia + k < hi) acc[k] = voigt_add(acc[k], nu_k[k] - lnu, inv, y, amp, k1);
                }
            }
            h = h_n, cl = cl_n, y = y_n, amp = amp_n, inv = inv_n, lnu = lnu_n;
        }
        if constexpr (F32) {
#pragma unroll
            for (int k = 0; k < F; ++k) acc[k] += (double)acc32[k];
        }
    }
    // (4) where the sums go: the narrow plane, or SUB: the kernel's common reduction, where the four subsets of a group meet
#pragma unroll
    for (int k = 0; k < F; ++k) {
        if constexpr (SUB) out[k] = acc[k];
        else if (valid && act[k]) out[(size_t)d * pld + (i0 + k - nu_begin)] = acc[k];
    }
}
#undef SDX_NARROW_FETCH
#undef SDX_NARROW_LINE

// The one-frequency walk of the mixed-precision mode: what line_narrow_walk<1, false, true> would be, as text of its own (a wave past
// the shard's end returns instead of keeping act[]).  Folding it into the walk was tried in two spellings: k_line_all_mixed<4, false,
// false> and <4, false, true> came out 26 and 15 instructions shorter but with 56 and 80 spilled SGPRs against 55 and 78, and the line
// path takes no spill more than its parent's (profiles/EXPERIMENTS.md): it stays.
__device__ __forceinline__ void line_narrow_wave32(const int64_t i, const int depth_chunk, int n_depth, int64_t n_nu, const double* __restrict__ nus,
                                                          int64_t nu_begin, int64_t nu_count, LineWork w, double* __restrict__ plane, int64_t pld)
{
    const int lane = threadIdx.x & 63;
    if (i >= nu_begin + nu_count) return;
    const int d = depth_chunk * 64 + lane;
    const bool valid = d < n_depth;
    const int dc = valid ? d : n_depth - 1;
    const int ii = (int)i;
    const int64_t pa = max(i - kNarrowReach + 1, (int64_t)0);
    const int64_t pb = min(i + kNarrowReach, n_nu);
    const int la = __builtin_amdgcn_readfirstlane(w.cnt_ge[pb + 1]);
    const int lb = __builtin_amdgcn_readfirstlane(w.cnt_ge[pa]);
    const double nu_i = nus[i];
    const float nih = (float)nu_i, nil = (float)(nu_i - (double)nih);
    double acc = 0.0;
    // (trips aligned to the list, like every walk with fp32 sums: (2) in line_narrow_walk)
    for (int base = la & ~63; base < lb; base += 64) {
        const int lc = base + lane;
        bool rel = false;
        int c = 0;
        if (lc >= la && lc < lb) {
            const int hwm = w.nhw_max[lc];
            c = w.centre[lc];
            rel = hwm > 0 && ii >= c - hwm && ii < c + hwm;
        }
        unsigned long long m = __ballot(rel);
        float acc32 = 0.f;
        int h = 0, cl = 0;
        float y = 0.f, amp = 0.f, inv = 0.f;
        float2v lnu = {0.f, 0.f};
        if (m) {
            const int bit = __builtin_ctzll(m);
            const int l = base + bit;
            const size_t o = (size_t)l * n_depth + dc;
            cl = __builtin_amdgcn_readlane(c, bit);
            h = w.nhw[o], y = w.n_y32[o], amp = w.n_amp32[o], inv = w.n_inv32[o], lnu = w.lnu32[l];
        }
        while (m) {
            m &= m - 1;
            int h_n = 0, cl_n = 0;
            float y_n = 0.f, amp_n = 0.f, inv_n = 0.f;
            float2v lnu_n = {0.f, 0.f};
            if (m) {
                const int bit = __builtin_ctzll(m);
                const int l = base + bit;
                const size_t o = (size_t)l * n_depth + dc;
                cl_n = __builtin_amdgcn_readlane(c, bit);
                h_n = w.nhw[o], y_n = w.n_y32[o], amp_n = w.n_amp32[o], inv_n = w.n_inv32[o], lnu_n = w.lnu32[l];
            }
            if (valid && ii >= cl - h && ii < cl + h) acc32 = voigt_add32(acc32, ((nih - lnu.x) + (nil - lnu.y)) * inv, y, amp);
            h = h_n, cl = cl_n, y = y_n, amp = amp_n, inv = inv_n, lnu = lnu_n;
        }
        acc += (double)acc32;
    }
    if (valid) plane[(size_t)d * pld + (i - nu_begin)] = acc;
}

// FAR FIELD of the line opacity (far_eligible above): the third plane of the line kernels.  One workgroup owns (depth d, a unit of
// 4 RF consecutive global tiles, RF = 1 or 2); lane <-> (tile 4 r + lane / 16 of the unit, Chebyshev node lane % 16), r < RF.  Its
// n_split waves (the line kernel's, whose far role this is) go through the candidate lists exactly
// as the wide role does (hlist, then the wlist range around the unit; chunk q of 64 candidates belongs to wave q mod n_split): each
// lane tests ONE candidate against the unit (its whole span first, the single tiles where that does not settle it) and keeps the
// mask of the tiles it is far from; the hits are queued in LDS in list order and evaluated 64 at a time — records fetched by the
// lanes in one round trip — at the lanes' nodes with the wide role's own arithmetic (x = fma(dnu, inv, c0), region1_add), test-free
// when the candidate is far from every tile of the unit.  The waves' node sums meet in LDS (subset order), wave 0 turns the 16 node
// values of a tile into the coefficients of its Chebyshev series (kFarCoef), and every wave evaluates the series of its share of
// the tiles at their grid points (Clenshaw) and writes the plane — zeros where a tile has no far field.  The sum of a (tile, node)
// adds its lines in list order within a subset and the subsets in order, whatever RF and whatever the shard: RF is pure scheduling.
// F32 (the fp32-mixed tolerance mode, units of 8 tiles): the node sums in PACKED fp32 — a lane's two nodes are one float pair, a hit is
// region1_f32x2 on the pre-pass's 32-byte fp32 record (nine instructions where the fp64 form takes twenty-three for the pair) — and the
// Chebyshev transform and the Clenshaw recurrence in fp64 as before.  Per term ~1e-6 relative (the node's distance from the line is
// known to 3e-7: offsets from an fp32 base frequency, exact difference of two fp32 frequencies), well inside the mode's 1e-4.
template <int R, int RF, bool F32 = false>
__device__ __forceinline__ void line_far_body(const int block, const int units, const int n_split, int n_depth, int64_t n_nu, const double* __restrict__ nus,
                                              int64_t nu_begin, int64_t nu_count, int64_t n_lines, LineWork w, double* __restrict__ plane, int64_t pld,
                                              double* __restrict__ s_far)
{
    // s_far: [n_split][64 RF] partial node sums, [64 RF] node values, [64 RF] coefficients, [n_split][kFarWaveLdsDoubles]
    constexpr int kTile = 64 * R, kUnitTiles = 4 * RF;
    const int lane = threadIdx.x & 63;
    const int split = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int d = block / units, u = block - d * units;
    const int64_t T_first = nu_begin / kTile, T_last = (nu_begin + nu_count - 1) / kTile;  // the global tiles that hold the shard's columns
    const int64_t Tu = (T_first / kUnitTiles + u) * kUnitTiles;                          // units are aligned to the global tiles too
    const int64_t Ta = max(Tu, T_first), Tb = min(Tu + kUnitTiles - 1, T_last);
    if (Ta > Tb) return;
    const int64_t g0 = Ta * kTile, g1 = min((Tb + 1) * kTile, n_nu);  // the grid points of the tiles this workgroup handles
    const int64_t s0 = nu_begin, s1 = nu_begin + nu_count;

    // the tiles' far ranges, wave-uniform (scalar loads): the candidate tests below
    static_assert(kTile == kFarTile, "the far field lives on 256-point tiles");
    int ihi[kUnitTiles], ilo[kUnitTiles];
    unsigned all_mask = 0;
#pragma unroll
    for (int t = 0; t < kUnitTiles; ++t) {
        const int64_t T = Tu + t;
        const bool mine = T >= Ta && T <= Tb;
        ihi[t] = mine ? w.far_range[2 * T] : 0;
        ilo[t] = mine ? w.far_range[2 * T + 1] : 0x7FFFFFFF;
        all_mask |= (ihi[t] != 0 || ilo[t] != 0x7FFFFFFF) ? (1u << t) : 0u;  // (0, INT_MAX): no far field
    }
    // ... and what decides most candidates without a look at the single tiles: the span of the tiles that have a far field (they are
    // consecutive: only the grid's last tile can lack one) and the tightest of their ranges
    int span_lo = 0x7FFFFFFF, span_hi = 0, min_ihi = 0x7FFFFFFF, max_ilo = 0;
#pragma unroll
    for (int t = 0; t < kUnitTiles; ++t) {
        if ((all_mask >> t) & 1u) {
            span_lo = min(span_lo, (int)((Tu + t) * kTile));
            span_hi = max(span_hi, (int)((Tu + t + 1) * kTile));
            min_ihi = min(min_ihi, ihi[t]);
            max_ilo = max(max_ilo, ilo[t]);
        }
    }
    if (all_mask == 0) {  // nothing but a partial last tile: zeros
        for (int t = split; t < kUnitTiles; t += n_split) {
            const int64_t T = Tu + t;
            if (T < Ta || T > Tb) continue;
            for (int p = 0; p < R; ++p) {
                const int64_t i = T * kTile + lane + 64 * p;
                if (i < n_nu && i >= s0 && i < s1) plane[(size_t)d * pld + (i - s0)] = 0.0;
            }
        }
        return;
    }
    // the lane's nodes as offsets from a base frequency (the wide role's form of x) that depends on neither the shard nor RF: the
    // first frequency of the block of 16 global tiles the unit lies in
    const double nu_base_v = nus[(Tu / 16) * 16 * kTile];
    const double nu_base = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(nu_base_v)), __builtin_amdgcn_readfirstlane(__double2loint(nu_base_v)));
    double nu_base_vec = nu_base;
    asm("" : "+v"(nu_base_vec));
    double dnu[RF], acc[RF];
    const int tg = lane >> 4;
    const double node = kFarNode[lane & 15];
#pragma unroll
    for (int r = 0; r < RF; ++r) {
        const int64_t T = Tu + 4 * r + tg, i0 = T * kTile;
        acc[r] = 0.0;
        dnu[r] = 0.0;
        if (T >= Ta && T <= Tb && i0 + kTile <= n_nu) {
            double c, h;
            far_tile_geometry(nus[i0], nus[i0 + kTile - 1], c, h);
            dnu[r] = fma(h, node, c - nu_base);
        }
    }
    const size_t row = (size_t)d * n_lines;
    const WideScan* __restrict__ scan_row = w.wscan + row;
    const WideScan* __restrict__ hscan_row = w.hscan + row;
    const WideRec* __restrict__ rec_row = w.wrec + row;
    [[maybe_unused]] const WideRec32* __restrict__ rec32_row = F32 ? w.wrec32 + row : nullptr;
    const int n_h = w.hlist ? __builtin_amdgcn_readfirstlane(*w.hcount) : 0;
    // F32: the lane's two nodes as fp32 offsets from the base frequency ROUNDED to fp32 (what the fp32 records' hi parts are differences to)
    static_assert(!F32 || RF == 2, "the packed fp32 far role pairs a lane's two nodes");
    [[maybe_unused]] float base_h = (float)nu_base;
    [[maybe_unused]] float2v dq32 = {0.f, 0.f}, acc32 = {0.f, 0.f};
    if constexpr (F32) {
        asm("" : "+v"(base_h));
        const double shift = nu_base - (double)base_h;
        dq32.x = (float)(dnu[0] + shift);
        dq32.y = (float)(dnu[RF - 1] + shift);
    }

    // Scan and evaluation are decoupled: a wave that fetched the record of every hit when it met it spent its time waiting for one
    // dependent load after the other (~500 hits, a microsecond each).  The hits of the chunks are QUEUED in LDS instead — line index
    // and tile mask, in list order — and a full queue (64 hits) is evaluated at once: lane j fetches hit j's 48-byte record, all 64
    // in ONE round trip, into LDS, and the wave goes through them with broadcast reads.
    double* const wave_lds = s_far + (size_t)(n_split + 2) * RF * 64 + (size_t)split * kFarWaveLdsDoubles;
    WideRec* const stage = reinterpret_cast<WideRec*>(wave_lds);  // 64 x 48 B
    [[maybe_unused]] WideRec32* const stage32 = reinterpret_cast<WideRec32*>(wave_lds);  // (F32: 64 x 32 B in the same space)
    int* const q_line = reinterpret_cast<int*>(wave_lds + 64 * 6);
    int* const q_mask = q_line + 64;
    int count = 0;
    auto flush = [&](int cnt) {
        if (cnt == 0) return;
        wave_sync();
        const bool mine = lane < cnt;
        const unsigned qm = mine ? (unsigned)q_mask[lane] : 0u;
        if constexpr (F32) {
            if (mine) stage32[lane] = rec32_row[q_line[lane]];
        } else {
            if (mine) stage[lane] = rec_row[q_line[lane]];
        }
        const unsigned long long mfull = __ballot(mine && qm == all_mask);
        wave_sync();
        if constexpr (F32) {
            for (int k = 0; k < cnt; ++k) {
                const WideRec32 cur = stage32[k];  // (one address for the whole wave: a broadcast read)
                const float c0 = region1_c0(base_h, cur);
                if ((mfull >> k) & 1) {  // far from every tile of the unit: no per-lane tests
                    acc32 = region1_f32x2(acc32, dq32, c0, cur);
                } else {
                    const unsigned tm = (unsigned)__builtin_amdgcn_readlane((int)qm, k);
                    // (the accumulating FMA of the test-free form, kept or dropped per node: a tile's sum must not depend on whether its
                    // unit's other tiles — which a shard may not own — let the hit take the test-free path)
                    const float2v v = region1_f32x2(acc32, dq32, c0, cur);
                    acc32.x = ((tm >> tg) & 1u) ? v.x : acc32.x;
                    acc32.y = ((tm >> (4 + tg)) & 1u) ? v.y : acc32.y;
                }
            }
            wave_sync();
            return;
        }
        for (int k = 0; k < cnt; ++k) {
            const WideRec cur = stage[k];  // (one address for the whole wave: a broadcast read)
            const RegionI k1 = {cur.yk, cur.cv, cur.cd};
            const double c0 = (nu_base_vec - cur.lnu) * cur.inv;
            if (((mfull >> k) & 3) == 3 && k + 1 < cnt) {
                // two test-free hits at once: two independent chains of dependent instructions (a shard's launch has two or three
                // waves per SIMD: nothing else fills the gaps); the sums keep list order
                const WideRec nxt = stage[k + 1];
                const RegionI k2 = {nxt.yk, nxt.cv, nxt.cd};
                const double c1 = (nu_base_vec - nxt.lnu) * nxt.inv;
#pragma unroll
                for (int r = 0; r < RF; ++r) {
                    acc[r] = region1_add(acc[r], fma(dnu[r], cur.inv, c0), k1);
                    acc[r] = region1_add(acc[r], fma(dnu[r], nxt.inv, c1), k2);
                }
                ++k;
            } else if ((mfull >> k) & 1) {  // far from every tile of the unit: no per-lane tests
#pragma unroll
                for (int r = 0; r < RF; ++r) acc[r] = region1_add(acc[r], fma(dnu[r], cur.inv, c0), k1);
            } else {
                const unsigned tm = (unsigned)__builtin_amdgcn_readlane((int)qm, k);
#pragma unroll
                for (int r = 0; r < RF; ++r) {
                    if (((tm >> (4 * r)) & 15u) == 0) continue;  // (scalar)
                    const bool take = (tm >> (4 * r + tg)) & 1u;
                    acc[r] = region1_add_if(acc[r], fma(dnu[r], cur.inv, c0), k1, take);
                }
            }
        }
        wave_sync();  // (the queue and the staged records are written again)
    };

    for (int pass = w.hlist ? 0 : 1; pass < 2; ++pass) {
        int ka = 0, kb = n_h;
        if (pass == 1) {
            kb = (int)n_lines;
            if (w.hlist) {  // (the wide role's candidate range, around the unit instead of a tile)
                const int64_t pa = max(g0 - kMediumHalfWidth + 1, (int64_t)0), pb = min(g1 + kMediumHalfWidth - 1, n_nu);
                ka = __builtin_amdgcn_readfirstlane(w.wrank[w.cnt_ge[pb + 1]]);
                kb = __builtin_amdgcn_readfirstlane(w.wrank[w.cnt_ge[pa]]);
                if (w.sel) {
                    ka = max(ka, __builtin_amdgcn_readfirstlane(w.wrank[w.sel[0]]));
                    kb = min(kb, __builtin_amdgcn_readfirstlane(w.wrank[w.sel[1]]));
                }
            }
        }
        if (kb <= ka) continue;
        const int q_first = ka >> 6, q_last = (kb - 1) >> 6;
        int q = q_first + ((split - q_first % n_split) + n_split) % n_split;
        auto fetch = [&](int qq, int& line, WideScan& sc) {
            const int k = qq * 64 + lane;
            line = -1;
            sc = WideScan{0, 0, 0, 0};
            if (qq <= q_last && k >= ka && k < kb) {
                if (pass == 0) {
                    line = w.hlist[k];
                    sc = w.hscan ? hscan_row[k] : scan_row[line];
                } else {
                    line = w.hlist ? w.wlist[k] : k;
                    sc = scan_row[line];
                }
            }
        };
        int line_next;
        WideScan sc_next;
        fetch(q, line_next, sc_next);
        for (; q <= q_last; q += n_split) {
            const int line = line_next;
            const WideScan sc = sc_next;
            fetch(q + n_split, line_next, sc_next);
            // Most candidates are far from every tile of the unit (a strong line somewhere else on the grid) or reach none of them: one test
            // of the whole span each — far_eligible of the span with the tightest range implies it of every tile — and the tile-by-tile
            // tests only for a chunk that holds a candidate neither settles
            const bool all_far = far_eligible(sc, span_lo, span_hi, min_ihi, max_ilo);
            const bool none = (line < 0) | (sc.hi - sc.lo < kTile) | (sc.hi <= span_lo) | (sc.lo >= span_hi);
            unsigned tmask = all_far && !none ? all_mask : 0u;
            if (__ballot(!all_far && !none)) {
                unsigned tm = 0;
#pragma unroll
                for (int t = 0; t < kUnitTiles; ++t) {
                    const int i0 = (int)min((Tu + t) * kTile, n_nu);  // (tiles beyond the grid: never far)
                    tm |= far_eligible(sc, i0, i0 + kTile, ihi[t], ilo[t]) ? (1u << t) : 0u;
                }
                if (!all_far && !none) tmask = tm;
            }
            // the hits join the wave's queue (list order); a full queue is evaluated (flush)
            const unsigned long long m = __ballot(tmask != 0);
            const int n = __popcll(m);
            if (n == 0) continue;
            if (count + n > 64) {
                flush(count);
                count = 0;
            }
            if (tmask != 0) {
                const int at = count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                q_line[at] = line;
                q_mask[at] = (int)tmask;
            }
            count += n;
        }
    }
    flush(count);
    if constexpr (F32) acc[0] = (double)acc32.x, acc[RF - 1] = (double)acc32.y;

    // the subsets' node sums, in subset order
    double* red = s_far;
    double* sV = s_far + (size_t)n_split * RF * 64;
    double* sC = sV + RF * 64;
    if (split > 0) {
#pragma unroll
        for (int r = 0; r < RF; ++r) red[((size_t)split * RF + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (split == 0) {
        for (int s = 1; s < n_split; ++s) {
#pragma unroll
            for (int r = 0; r < RF; ++r) acc[r] = add_rn(acc[r], red[((size_t)s * RF + r) * 64 + lane]);
        }
#pragma unroll
        for (int r = 0; r < RF; ++r) sV[r * 64 + lane] = acc[r];
        wave_sync();
        // node values -> Chebyshev coefficients: lane <-> (tile, k)
        const int k = lane & 15;
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            const double* v = sV + r * 64 + (lane & 48);
            double c = 0.0;
#pragma unroll
            for (int j = 0; j < kFarNodes; ++j) c = fma(kFarCoef[k][j], v[j], c);
            sC[r * 64 + lane] = c;  // = sC[(4 r + tg) * 16 + k]
        }
    }
    __syncthreads();
    // the series at the grid points of the tiles (Clenshaw), one tile at a time per wave
    for (int t = split; t < kUnitTiles; t += n_split) {
        const int64_t T = Tu + t, i0 = T * kTile;
        if (T < Ta || T > Tb) continue;
        bool okt = i0 + kTile <= n_nu;
        double c = 0.0, h = 1.0;
        if (okt) {
            far_tile_geometry(nus[i0], nus[i0 + kTile - 1], c, h);
            okt = h > 0.0;
        }
        const double rh = okt ? 1.0 / h : 0.0;
        const double* cf = sC + t * kFarNodes;
#pragma unroll
        for (int p = 0; p < R; ++p) {
            const int64_t i = i0 + lane + 64 * p;
            if (i >= n_nu) continue;
            double val = 0.0;
            if (okt) {
                const double x = (nus[i] - c) * rh, x2 = x + x;
                double b1 = 0.0, b2 = 0.0;
#pragma unroll
                for (int k = kFarNodes - 1; k >= 1; --k) {
                    const double b0 = fma(x2, b1, cf[k] - b2);
                    b2 = b1, b1 = b0;
                }
                val = fma(x, b1, cf[0] - b2);
            }
            if (i >= s0 && i < s1) plane[(size_t)d * pld + (i - s0)] = val;
        }
    }
}

// The kernels with a far field (FAR) take the launch as LineWords instead: the four words of the host's choices, which every wave
// decodes itself with the divisions that LineGeom (sdx_line_geom.h) spares the others.  Every FAR instantiation fills its 80 registers
// (six waves per SIMD) without a spill only as long as its entry code is what it was: with LineGeom's decode in the place of the one below
// each of them spilled a vector register, and a kernel that spills is not run.  Their grids are large
// and their waves long: ~600 scalar instructions at the head of a narrow wave are below one per cent of such a launch.
// roles: bit 0 wide, bit 1 narrow; bits 2-3 narrow order; bits 4-7 wide group; bits 8-11 F; bits 16-17 RF of the far role in front of the grid (0: none —
// the second of two split launches).  Same grid, same units in the same order as line_launch_make's.
struct LineWords {
    int n_wide, tiles, roles, far_units;
};
template <bool FAR>
using LineLaunchArg = std::conditional_t<FAR, LineWords, LineGeom>;

// Both line kernels in ONE launch of workgroups of S waves (S = number of line subsets): workgroups [0, n_wide) take the
// wide role — one (depth, tile) each, wave s walks subset s — depth slowest, hottest layers first; the rest take the narrow
// role, one frequency per wave.  The two roles only share the pre-pass, and each leaves issue slots idle on its own; a
// cross-stream fork/join would cost two ~12 us inter-queue edges per step, one grid costs nothing.
// roles: bit 0 wide, bit 1 narrow (both by default; one at a time for split-launch profiling, SDX_SPLIT_LAUNCHES=1); bits 16-17: the
// far field's workgroups (line_far_body) come FIRST in the grid, n_depth x far_units of them (fp64 kernels with a far field).
// Output planes: [0] the wide windows (all subsets summed), [1] the narrow windows.
template <int R, bool MIXED, bool SUBSETS, bool FAR = false, bool LISTED = false>
__device__ __forceinline__ void line_all_body(LineLaunchArg<FAR> g, int n_split, int n_depth, int64_t n_nu,
                                                   const double* __restrict__ nus, int64_t nu_begin, int64_t nu_count,
                                                   int64_t n_lines, const double* __restrict__ line_nus, LineWork w,
                                                   double* __restrict__ planes, int64_t pld)
{
    extern __shared__ double s_wide[];  // n_split x kWideLdsDoubles
    // block -> unit of work.  Without a far field: sdx_line_geom.h — the launch's constants come formed from the host, no wave divides by
    // one; g is read where a role begins and nowhere else (n_split, which lives as long as the walks, is an argument of its own: a word of
    // g that stays live keeps the words it was loaded with in registers, or in spill lanes).  FAR: LineWords, decoded here.
    int b = blockIdx.x;
    // (fp32-mixed kernels with a far field: what is left to the wide role — a line's near zone, window edges, kept cores — is walked in
    // fp64 by the queued walk like the fp64 kernels'; the narrow role and the formal solution stay the mode's fp32)
    constexpr bool WM = MIXED && !FAR;  // the wide role's arithmetic
    if constexpr (FAR) {
        // far role (roles bits 16-17: RF, 0 = no far workgroups in this launch): the FIRST workgroups of the grid — their waves are
        // the longest chains of the launch (a unit walks every huge line of the list) — n_depth x far_units of them
        const int rf = (g.roles >> 16) & 3;
        if (rf) {
            const int n_far = n_depth * g.far_units;
            if (b < n_far) {
                double* const far_plane = planes + (size_t)2 * n_depth * pld;
                // (fp32-mixed mode: the node sums in packed fp32 — units of 8 tiles)
                // (the host sets rf to 0 or 2.  Deleting the <R, 1> branch was tried: 1460 - 1660 fewer instructions in each of the six
                // kernels, but more spilled SGPRs in three to five of them however the test is written — k_line_all<4, true, true>
                // 58 -> 63 or 67, k_line_listed<4, false, true> 76 -> 80 or 94: it stays, profiles/EXPERIMENTS.md)
                if (rf == 2) line_far_body<R, 2, MIXED>(b, g.far_units, n_split, n_depth, n_nu, nus, nu_begin, nu_count, n_lines, w, far_plane, pld, s_wide);
                else line_far_body<R, 1>(b, g.far_units, n_split, n_depth, n_nu, nus, nu_begin, nu_count, n_lines, w, far_plane, pld, s_wide);
                return;
            }
            b -= n_far;
        }
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform, which the compiler cannot see: chunk and frequency indices stay scalar
    // SUBSETS (the kernel of dense long lists): both roles end in ONE reduction — every wave of a workgroup brings R partial sums per
    // lane (a wide wave: R points of its tile; a narrow wave: the R = F frequencies of the workgroup's group), they meet in LDS
    // and wave 0 adds them in subset order and writes.  One barrier in the kernel: with a second one in the narrow branch the
    // compiler spilled the WIDE walk's registers, and a kernel that touches scratch at all ran a third slower (round 5).
    [[maybe_unused]] double part[R];
    [[maybe_unused]] int out_row = 0, out_col = 0;      // where lane's sums go: row (depth), first column; columns step 64 (wide) or 1 (narrow)
    [[maybe_unused]] bool out_wide = true, out_valid = true;
    bool wide_role;
    if constexpr (FAR) wide_role = b < g.n_wide;
    else wide_role = b < g.narrow_first;
    if (wide_role) {
        // XCD-aware tile order: workgroup i runs on XCD i % 8, each with its own L2.  Within a depth the workgroups of one XCD
        // take CONTIGUOUS tiles (position p -> tile prefix(p % 8) + p / 8), so neighbouring tiles, whose line ranges
        // overlap, hit the same L2 instead of pulling the same records into all eight.
        int tile, d;
        if constexpr (FAR) {
            if (!(g.roles & 1)) return;
            const int tiles = g.tiles;
            // (the host sets the wide group to 0.  Deleting the other decode here and in wide_unit was tried: spilled SGPRs 46 -> 49 in
            // k_line_all<4, true, false>, 76 -> 81 in k_line_listed<4, false, true>, 76 -> 86 in k_line_all_mixed<4, true, true>: it stays)
            const int wg = (g.roles >> 4) & 15;  // 0: one contiguous eighth of the tiles per XCD; g > 0: groups of g tiles going round the XCDs
            if (wg == 0) {
                const int p = b % tiles;
                d = b / tiles;
                tile = p >> 3;
                for (int f = 0; f < (p & 7); ++f) tile += (tiles - f + 7) >> 3;
            } else {
                // (the host pads the tiles of a depth to whole rounds of 8 g workgroups: b % 8 is then the XCD within every depth)
                const int tiles_pad = (tiles + 8 * wg - 1) / (8 * wg) * (8 * wg);
                const int p = b % tiles_pad, j = p >> 3;
                d = b / tiles_pad;
                tile = ((j / wg) * 8 + (p & 7)) * wg + j % wg;
                if (tile >= tiles) return;
            }
        } else {
            const WideUnit wu = wide_unit(g, b);
            if (!wu.live) return;
            tile = wu.tile, d = wu.depth;
        }
        if constexpr (SUBSETS) {
            line_wide_walk<R, WM, true, WM, FAR, LISTED>(tile, wave, n_split, d, n_nu, nus, nu_begin, nu_count, n_lines, w, planes, pld, s_wide, part);
            out_row = d;
            out_col = (int)((nu_begin / (64 * R) + (int64_t)tile) * (64 * R)) + (int)(threadIdx.x & 63);
        } else {
            line_wide_walk<R, WM, false, false, FAR, LISTED>(tile, wave, n_split, d, n_nu, nus, nu_begin, nu_count, n_lines, w, planes, pld, s_wide);
        }
    } else {
        // A wave writes one value into each of the N_d rows of the narrow plane: the waves that fill a 64-byte sector of a
        // row (8 consecutive frequencies) should share an L2, or every XCD writes its own fragment of every sector back on
        // its own.  Workgroups p, p + 8, ... (one XCD) therefore take GROUPS of kNarrowGroup consecutive workgroups' worth
        // of frequencies, the groups going round the XCDs.  (Giving each XCD one contiguous eighth of the grid was measured
        // 45 % slower: the lines per grid point follow the frequency, so one XCD gets several times the work of another.)
        // (SUBSETS: a workgroup is ONE group of frequencies, not four — sixteen workgroups keep the 64 consecutive frequencies per XCD
        // whose lines' records then meet in one L2)
        // F consecutive frequencies per wave (1, 2 or 4 — 8 was measured slower), groups aligned to the global grid.
        // dense long lists (a kernel of their own — SUBSETS — so that neither walk pays for the other's registers: with both narrow
        // walks in one kernel the WIDE role spilled, and a kernel that touches scratch memory ran a third slower): the workgroup's
        // four waves share one group of F = 4 frequencies
        int64_t i0;
        int chunk;
        [[maybe_unused]] int F;
        if constexpr (FAR) {
            if (!(g.roles & 2)) return;
            constexpr int kNarrowGroup = SUBSETS ? kNarrowGroupSubsets : kNarrowGroupPlain;
            F = max(1, (g.roles >> 8) & 15);
            const int64_t g0 = nu_begin / F;
            const int64_t n_grp = (nu_begin + nu_count + F - 1) / F - g0;
            const int64_t n_narrow = n_grp * ((n_depth + 63) / 64);
            const int64_t n_nb = SUBSETS ? n_narrow : (n_narrow + n_split - 1) / n_split;
            const int64_t p = b - g.n_wide, j = p >> 3;
            // (the host sets the order to 0.  Deleting orders 1 and 2 here and in narrow_unit was tried: spilled SGPRs 51 -> 60 in
            // k_line_all<4, false, false>, 46 -> 56 in k_line_all<4, true, false>, 80 -> 90 in k_line_listed<4, false, false>: they stay)
            const int order = (g.roles >> 2) & 3;  // 0 grouped (what the host sets), 1 plain, 2 one block per XCD
            int64_t wg = ((j / kNarrowGroup) * 8 + (p & 7)) * kNarrowGroup + j % kNarrowGroup;
            if (order == 1) wg = p;
            if (order == 2) wg = (p & 7) * ((n_nb + 7) / 8) + j;
            if ((order == 2 && j >= (n_nb + 7) / 8) || wg >= n_nb) return;
            const int64_t c = SUBSETS ? wg : wg * n_split + wave;
            if (c >= n_narrow) return;  // (subsets: the whole workgroup)
            i0 = (g0 + c % n_grp) * F;
            chunk = (int)(c / n_grp);
        } else {
            const NarrowUnit unit = narrow_unit<SUBSETS>(g, b, wave);
            if (!unit.live) return;  // (subsets: the whole workgroup)
            i0 = unit.i0, chunk = unit.chunk, F = 1 << g.f_shift;
        }
        double* __restrict__ nplane = planes + (size_t)n_depth * pld;
        if constexpr (SUBSETS) {
            static_assert(!SUBSETS || R == 4, "the common reduction: R points per wide lane = F frequencies per narrow group");
            line_narrow_walk<4, true, MIXED>(i0, chunk, wave, n_depth, n_nu, nus, nu_begin, nu_count, line_nus, w, part, 0);
            out_wide = false;
            out_row = chunk * 64 + (int)(threadIdx.x & 63);
            out_valid = out_row < n_depth;
            out_col = (int)i0;
        } else {
            if (F == 4) line_narrow_walk<4, false, MIXED>(i0, chunk, 0, n_depth, n_nu, nus, nu_begin, nu_count, line_nus, w, nplane, pld);
            else if (F == 2) line_narrow_walk<2, false, MIXED>(i0, chunk, 0, n_depth, n_nu, nus, nu_begin, nu_count, line_nus, w, nplane, pld);
            else if constexpr (MIXED) line_narrow_wave32(i0, chunk, n_depth, n_nu, nus, nu_begin, nu_count, w, nplane, pld);
            else line_narrow_wave(i0, chunk, n_depth, n_nu, nus, nu_begin, nu_count, n_lines, line_nus, w, nplane, pld);
        }
    }
    if constexpr (SUBSETS) {
        constexpr int kLdsStride = (FAR && SDX_WIDE_QUEUED) ? kWideFarLdsDoubles : kWideLdsDoubles;  // (the wide walk's)
        const int lane = threadIdx.x & 63;
        if (wave > 0) {
            double* mine = s_wide + (size_t)wave * kLdsStride;
#pragma unroll
            for (int r = 0; r < R; ++r) mine[r * 64 + lane] = part[r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll 1
            for (int s = 1; s < n_split; ++s) {
                const double* other = s_wide + (size_t)s * kLdsStride;
#pragma unroll
                for (int r = 0; r < R; ++r) part[r] = add_rn(part[r], other[r * 64 + lane]);
            }
            const int64_t s0 = nu_begin, s1 = nu_begin + nu_count;  // the columns this launch stores
            double* __restrict__ dst = planes + (out_wide ? (size_t)0 : (size_t)n_depth * pld) + (size_t)out_row * pld;
            const int stride = out_wide ? 64 : 1;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t col = (int64_t)out_col + (int64_t)r * stride;
                if (out_valid && col >= s0 && col < s1) dst[col - s0] = part[r];
            }
        }
    }
}

template <int R, bool SUBSETS = false, bool FAR = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(FAR ? SDX_FAR_WAVES : 7, 8))) void k_line_all(LineLaunchArg<FAR> g, int n_split, int n_depth, int64_t n_nu,
                                                   const double* __restrict__ nus, int64_t nu_begin, int64_t nu_count,
                                                   int64_t n_lines, const double* __restrict__ line_nus, LineWork w,
                                                   double* __restrict__ planes, int64_t pld)
{
    line_all_body<R, false, SUBSETS, FAR>(g, n_split, n_depth, n_nu, nus, nu_begin, nu_count, n_lines, line_nus, w, planes, pld);
}
// short lists whose pre-pass has listed their wide lines (LineWork::n_csplit, context option "wide_list"): the wide role walks its
// subset's list instead of scanning every line; everything else is k_line_all
template <int R, bool SUBSETS = false, bool FAR = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(FAR ? SDX_FAR_WAVES : 7, 8))) void k_line_listed(LineLaunchArg<FAR> g, int n_split, int n_depth, int64_t n_nu,
                                                   const double* __restrict__ nus, int64_t nu_begin, int64_t nu_count,
                                                   int64_t n_lines, const double* __restrict__ line_nus, LineWork w,
                                                   double* __restrict__ planes, int64_t pld)
{
    line_all_body<R, false, SUBSETS, FAR, true>(g, n_split, n_depth, n_nu, nus, nu_begin, nu_count, n_lines, line_nus, w, planes, pld);
}
// the mixed-precision variant (R = 4: 256-point tiles, six waves per SIMD; with 512-point tiles, measured slower and no longer
// instantiated, the budget was capped at 128 registers — what exceeds it sits in the rarely taken fp64 general path)
template <int R, bool SUBSETS = false, bool FAR = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(R == 4 ? 6 : 4, 8))) void k_line_all_mixed(
    LineLaunchArg<FAR> g, int n_split, int n_depth, int64_t n_nu, const double* __restrict__ nus, int64_t nu_begin, int64_t nu_count,
    int64_t n_lines, const double* __restrict__ line_nus, LineWork w, double* __restrict__ planes, int64_t pld)
{
    line_all_body<R, true, SUBSETS, FAR>(g, n_split, n_depth, n_nu, nus, nu_begin, nu_count, n_lines, line_nus, w, planes, pld);
}

// out (+)= sum over the S line subsets, in subset order
__global__ __launch_bounds__(kBlock) void k_reduce_partials(int n_depth, int64_t nu_count, int n_split,
                                                            const double* __restrict__ partial, int64_t pld,
                                                            double* __restrict__ out, int64_t out_ld, int accumulate)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int d = blockIdx.y;
    if (j >= nu_count) return;
    double v = partial[(size_t)d * pld + j];
    for (int s = 1; s < n_split; ++s) v = add_rn(v, partial[((size_t)s * n_depth + d) * pld + j]);
    double* p = out + (size_t)d * out_ld + j;
    *p = accumulate ? add_rn(*p, v) : v;
}

// ------------------------------------------------------------------------------------------------
// element-wise entry points
__global__ __launch_bounds__(kBlock) void k_faddeeva(int64_t n, const double* __restrict__ z, double* __restrict__ wout)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const c64 r = faddeeva_full(c64{z[2 * i], z[2 * i + 1]});
    wout[2 * i] = r.re;
    wout[2 * i + 1] = r.im;
}

__global__ __launch_bounds__(kBlock) void k_voigt_profile(int64_t n, const double* __restrict__ dnu,
                                                          const double* __restrict__ dw, const double* __restrict__ g,
                                                          double* __restrict__ phi)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) phi[i] = voigt_profile_full(dnu[i], dw[i], g[i]);
}

// The routine the line kernels evaluate per (line, depth, frequency) — region1_setup + voigt_term, i.e. the FMA /
// real-part-only variant of voigt.py:17-86,113-150 — exposed element-wise so that it can be pinned point by point against
// the reference's Faddeeva / Voigt golden vectors (the element-wise sdx_faddeeva_dev / sdx_voigt_profile_dev run the
// reference-order routine faddeeva_full instead).  out = amp * Re w((delta_nu + i gamma / (sqrt(pi) pi)) / doppler_width)
// with the pre-pass's derived constants: inv_dw = 1 / dw, y = (gamma / (sqrt(pi) pi)) / dw, amp as given.
__global__ __launch_bounds__(kBlock) void k_voigt_term(int64_t n, const double* __restrict__ dnu, const double* __restrict__ inv_dw,
                                                       const double* __restrict__ y, const double* __restrict__ amp,
                                                       double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const RegionI k1 = region1_setup(y[i], amp[i]);
    out[i] = voigt_term(dnu[i], inv_dw[i], y[i], amp[i], k1);
}

// The fp32 routine of the mixed-precision mode's narrow role (voigt_add32), element-wise: inputs rounded to fp32 as the
// pre-pass and the kernel round them.
__global__ __launch_bounds__(kBlock) void k_voigt_term32(int64_t n, const double* __restrict__ dnu, const double* __restrict__ inv_dw,
                                                         const double* __restrict__ y, const double* __restrict__ amp,
                                                         double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = (double)voigt_add32(0.f, (float)dnu[i] * (float)inv_dw[i], (float)y[i], (float)amp[i]);
}

// F_lambda = F_nu * nu / lambda (stardis/base.py:137-141: spectrum_lambda; the unit conversion there has scale 1)
__global__ __launch_bounds__(kBlock) void k_flux_nu_to_lambda(int64_t n, const double* __restrict__ f_nu, const double* __restrict__ nus,
                                                              const double* __restrict__ lambdas, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = mul_rn(f_nu[i], nus[i]) / lambdas[i];
}
__global__ __launch_bounds__(kBlock) void k_divide(int64_t n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = a[i] / b[i];
}

__global__ __launch_bounds__(kBlock) void k_blackbody(int n_depth, int64_t n_nu, const double* __restrict__ nus,
                                                      const double* __restrict__ temps, double* __restrict__ out, int64_t ld)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int d = blockIdx.y;
    if (i < n_nu) out[(size_t)d * ld + i] = planck(nus[i], temps[d]);
}

__global__ __launch_bounds__(kBlock) void k_weights(int64_t n, const double* __restrict__ tau, double* __restrict__ w0,
                                                    double* __restrict__ w1, double* __restrict__ w2)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double a, b, c;
    rt_weights(tau[i], a, b, c);
    w0[i] = a;
    w1[i] = b;
    w2[i] = c;
}

// ------------------------------------------------------------------------------------------------
// broadening kernels (scalar formulas: sdx_broadening.h)
__global__ __launch_bounds__(kBlock) void k_calc_gamma(int64_t n_lines, int n_depth, const int* __restrict__ z,
                                                       const int* __restrict__ ion, const double* __restrict__ e_ion,
                                                       const double* __restrict__ e_up, const double* __restrict__ e_lo,
                                                       const double* __restrict__ a_ul, const double* __restrict__ ne,
                                                       const double* __restrict__ temps, const double* __restrict__ nh,
                                                       int flags, double* __restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_lines * n_depth) return;
    const int64_t l = k / n_depth;
    const int d = (int)(k - l * n_depth);
    const double nu_ = n_effective(ion[l], e_ion[l], e_up[l]);
    const double nl_ = n_effective(ion[l], e_ion[l], e_lo[l]);
    const double g_lin = ((flags & 1) && z[l] == 1) ? gamma_linear_stark(nu_, nl_, ne[d]) : 0.0;
    const double g_q = (flags & 2) ? gamma_quadratic_stark(ion[l], nu_, nl_, ne[d], temps[d]) : 0.0;
    const double g_w = (flags & 4) ? gamma_van_der_waals(ion[l], nu_, nl_, temps[d], nh[d]) : 0.0;
    const double g_r = (flags & 8) ? a_ul[l] : 0.0;
    out[k] = add_rn(add_rn(add_rn(g_lin, g_q), g_w), g_r);  // broadening.py:649-654
}

__global__ __launch_bounds__(kBlock) void k_doppler_widths(int64_t n_lines, int n_depth, const double* __restrict__ lnu,
                                                           const double* __restrict__ mass, const double* __restrict__ temps,
                                                           double xi, double* __restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_lines * n_depth) return;
    const int64_t l = k / n_depth;
    const int d = (int)(k - l * n_depth);
    out[k] = doppler_width(lnu[l], temps[d], mass[l], xi);
}

// the three dense tables of the reference from a LineParams description (parity checks of the f1 path; any output may be null)
__global__ __launch_bounds__(kBlock) void k_line_params(int64_t n_lines, int n_depth, const double* __restrict__ line_nus,
                                                        LineParams lp, double* __restrict__ alphas, double* __restrict__ gammas,
                                                        int gamma_cols, double* __restrict__ doppler)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_lines * n_depth) return;
    const int64_t l = k / n_depth;
    const int d = (int)(k - l * n_depth);
    const double lnu = line_nus[l];
    const GenDepth D = gen_depth(lp, d);
    const GenLine L = gen_line(lp, lnu, l);
    if (alphas) alphas[k] = gen_alpha(lp, L, D, d, n_depth);
    if (doppler) doppler[k] = gen_doppler(lp, L, D);
    if (gammas && (gamma_cols > 1 || d == 0)) gammas[l * gamma_cols + (gamma_cols > 1 ? d : 0)] = gen_gamma(lp, L, D);
}

// plasma/base.py:130-175 AlphaLine: alpha = ((ALPHA_COEFFICIENT * n_lower) * stimulated_emission_factor) * f_lu, n_lower
// gathered from the level populations by lines_lower_level_index (numpy take, mode="raise": the host checks the range)
__global__ __launch_bounds__(kBlock) void k_alpha_line_levels(int64_t n_lines, int n_depth, const double* __restrict__ level_density,
                                                              const int* __restrict__ lower_index, const double* __restrict__ stim,
                                                              const double* __restrict__ f_lu, double coefficient,
                                                              double* __restrict__ alphas)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_lines * n_depth) return;
    const int64_t l = k / n_depth;
    const int d = (int)(k - l * n_depth);
    const double n_lower = level_density[(size_t)lower_index[l] * n_depth + d];
    alphas[k] = mul_rn(mul_rn(mul_rn(coefficient, n_lower), stim[k]), f_lu[l]);
}

// the reference's element-wise ufuncs (broadening.py:69-71, :140-146, :232-234, :346-360, :476-490)
enum BroadeningOp { kOpDoppler = 0, kOpNEff = 1, kOpLinearStark = 2, kOpQuadraticStark = 3, kOpVanDerWaals = 4 };
__global__ __launch_bounds__(kBlock) void k_broadening_scalar(int op, int64_t n, const double* __restrict__ a,
                                                              const double* __restrict__ b, const double* __restrict__ c,
                                                              const double* __restrict__ d, const double* __restrict__ e,
                                                              double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double r = 0.0;
    switch (op) {
        case kOpDoppler: r = doppler_width(a[i], b[i], c[i], d[i]); break;                              // nu, T, mass, xi
        case kOpNEff: r = n_effective((int)a[i], b[i], c[i]); break;                                    // ion, E_ion, E_lev
        case kOpLinearStark: r = gamma_linear_stark(a[i], b[i], c[i]); break;                           // n_up, n_lo, n_e
        case kOpQuadraticStark: r = gamma_quadratic_stark((int)a[i], b[i], c[i], d[i], e[i]); break;    // ion, n_up, n_lo, n_e, T
        case kOpVanDerWaals: r = gamma_van_der_waals((int)a[i], b[i], c[i], d[i], e[i]); break;         // ion, n_up, n_lo, T, n_H
    }
    out[i] = r;
}

__global__ __launch_bounds__(kBlock) void k_calc_vald_gamma(int64_t n_lines, int n_depth, const int* __restrict__ z,
                                                            const int* __restrict__ ion, const double* __restrict__ e_ion,
                                                            const double* __restrict__ e_up, const double* __restrict__ e_lo,
                                                            const double* __restrict__ a_ul, const double* __restrict__ stark,
                                                            const double* __restrict__ waals, const double* __restrict__ mass,
                                                            const double* __restrict__ ne, const double* __restrict__ temps,
                                                            const double* __restrict__ nh, int flags, double* __restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_lines * n_depth) return;
    const int64_t l = k / n_depth;
    const int d = (int)(k - l * n_depth);
    double g = 0.0;
    if (flags & 8) g = add_rn(g, a_ul[l]);
    if ((flags & 1) && z[l] == 1) {
        const double nu_ = n_effective(ion[l], e_ion[l], e_up[l]);
        const double nl_ = n_effective(ion[l], e_ion[l], e_lo[l]);
        g = add_rn(g, gamma_linear_stark(nu_, nl_, ne[d]));
    }
    if (flags & 2) g = add_rn(g, vald_stark(ne[d], stark[l], temps[d]));
    if (flags & 4) g = add_rn(g, vald_vdw(waals[l], temps[d], mass[l], e_up[l], e_lo[l], nh[d], ion[l], e_ion[l]));
    out[k] = (flags & 16) ? g : g / 2;  // broadening.py:1084; the molecular branch (:771-799) does not halve
}

// ------------------------------------------------------------------------------------------------
// continuum sources (opacities_solvers/base.py:40-317).  Each returns the value for one (depth, nu).
__device__ __forceinline__ double interp1(double x, int n, const double* __restrict__ xp, const double* __restrict__ fp)
{  // np.interp, xp ascending
    if (x <= xp[0]) return fp[0];
    if (x >= xp[n - 1]) return fp[n - 1];
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (xp[mid] <= x) lo = mid; else hi = mid;
    }
    if (xp[lo] == x) return fp[lo];
    const double slope = sub_rn(fp[lo + 1], fp[lo]) / sub_rn(xp[lo + 1], xp[lo]);
    return add_rn(mul_rn(slope, sub_rn(x, xp[lo])), fp[lo]);
}
__device__ __forceinline__ double inv_nu3(double nu) { return 1.0 / mul_rn(mul_rn(nu, nu), nu); }  // nu ** -3

// bf (:178-271): per (level, depth) coefficient BF_CONSTANT * Z**4 * n / n5 (:267-268), precomputed once
__global__ __launch_bounds__(kBlock) void k_bf_coef(int n_depth, int n_species, const int* __restrict__ offs,
                                                    const int* __restrict__ ions, const double* __restrict__ cutoff,
                                                    const double* __restrict__ level_density, double* __restrict__ coef)
{
    const int n_levels = offs[n_species];
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_levels * n_depth) return;
    const int L = k / n_depth;
    int s = 0;
    while (s + 1 < n_species && L >= offs[s + 1]) ++s;
    const int zi = ions[s] + 1;
    const double zeff = (double)zi;
    const double r = mul_rn(zeff, sqrt(kRydFreq / cutoff[L]));
    const double r2 = mul_rn(r, r);
    const double n5 = mul_rn(mul_rn(r2, r2), r);  // (...) ** 5
    coef[k] = mul_rn(mul_rn(kBfConst, (double)(zi * zi * zi * zi)), level_density[k]) / n5;
}

struct ContinuumArgs {
    // mirrors sdx_continuum (device pointers)
    const double* lambdas;
    int n_table;
    const double* table_wavelength;
    const double* table_sigma;
    const double* table_density;
    int bf_n_species;
    const int* bf_species_offsets;
    const int* bf_species_ion_number;
    const double* bf_cutoff;
    int bf_n_levels;                 // = bf_species_offsets[bf_n_species] when the host knows it, else 0
    const double* bf_coef;           // [n_levels][n_depth] from k_bf_coef (stand-alone bf source)
    const double* bf_level_density;  // [n_levels][n_depth] (fused total: coefficients formed in LDS)
    int ff_n_species;
    const int* ff_species_ion_number;
    const double* ff_number_density;
    const double* ray_n_h;
    const double* ray_n_he;
    const double* ray_n_h2;
    int rayleigh_enabled;
    const double* electron_density;
    const double* temperature;
    int n_file_planes;             // further tabulated sources as finished planes [n_depth][file_plane_ld], global columns
    const double* file_plane[4];
    int64_t file_plane_ld;
};

__device__ inline double alpha_bf_point(int n_depth, int d, double nu, int n_species, const int* __restrict__ offs,
                                        const double* __restrict__ cutoff, const double* __restrict__ coef)
{
    double total = 0.0;
    for (int s = 0; s < n_species; ++s) {
        double spec = 0.0;  // alpha_spec (:214), levels in plasma order (:221-233)
        for (int L = offs[s]; L < offs[s + 1]; ++L)
            spec = add_rn(spec, nu >= cutoff[L] ? coef[(size_t)L * n_depth + d] : 0.0);
        total = add_rn(total, spec);  // alpha_bf += alpha_spec (:235)
    }
    return mul_rn(total, inv_nu3(nu));  // :237
}
__device__ inline double alpha_ff_point(int n_depth, int d, double nu, double temp, int n_species,
                                        const int* __restrict__ ions, const double* __restrict__ number_density)
{
    double total = 0.0;
    for (int s = 0; s < n_species; ++s) {
        double v = number_density[(size_t)s * n_depth + d] / sqrt(temp);
        v = mul_rn(v, mul_rn(kFfConst, (double)(ions[s] * ions[s])));
        total = add_rn(total, v);
    }
    return mul_rn(total, inv_nu3(nu));
}
__device__ inline double alpha_rayleigh_point(int d, double nu, const double* __restrict__ nh, const double* __restrict__ nhe,
                                              const double* __restrict__ nh2)
{
    double c4 = 0, c6 = 0, c8 = 0;
    if (nh) { c4 = add_rn(c4, mul_rn(20.24, nh[d])); c6 = add_rn(c6, mul_rn(239.2, nh[d])); c8 = add_rn(c8, mul_rn(2256.0, nh[d])); }
    if (nhe) { c4 = add_rn(c4, mul_rn(1.913, nhe[d])); c6 = add_rn(c6, mul_rn(4.52, nhe[d])); c8 = add_rn(c8, mul_rn(7.90, nhe[d])); }
    if (nh2) { c4 = add_rn(c4, mul_rn(28.39, nh2[d])); c6 = add_rn(c6, mul_rn(215.0, nh2[d])); c8 = add_rn(c8, mul_rn(1303.0, nh2[d])); }
    const double nuc = nu > 2.3e15 ? 0.0 : nu;
    const double r = nuc / mul_rn(2.0, mul_rn(kC, kRydCm));
    const double r2 = mul_rn(r, r), r4 = mul_rn(r2, r2);
    const double r6 = mul_rn(r4, r2), r8 = mul_rn(r4, r4);
    return mul_rn(add_rn(add_rn(mul_rn(c4, r4), mul_rn(c6, r6)), mul_rn(c8, r8)), kSigmaT);
}

enum ContSource { kSrcFile1d = 0, kSrcBf = 1, kSrcFf = 2, kSrcRayleigh = 3, kSrcElectron = 4 };

// one source -> out (drop-in calc_alpha_* functions)
__global__ __launch_bounds__(kBlock) void k_continuum_source(int src, int n_depth, int64_t n_nu,
                                                             const double* __restrict__ nus, ContinuumArgs a,
                                                             double* __restrict__ out, int64_t ld)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int d = blockIdx.y;
    if (i >= n_nu) return;
    double v = 0.0;
    switch (src) {
        case kSrcFile1d: v = mul_rn(interp1(a.lambdas[i], a.n_table, a.table_wavelength, a.table_sigma), a.table_density[d]); break;
        case kSrcBf: v = alpha_bf_point(n_depth, d, nus[i], a.bf_n_species, a.bf_species_offsets, a.bf_cutoff, a.bf_coef); break;
        case kSrcFf: v = alpha_ff_point(n_depth, d, nus[i], a.temperature[d], a.ff_n_species, a.ff_species_ion_number, a.ff_number_density); break;
        case kSrcRayleigh: v = alpha_rayleigh_point(d, nus[i], a.ray_n_h, a.ray_n_he, a.ray_n_h2); break;
        case kSrcElectron: v = mul_rn(kSigmaT, a.electron_density[d]); break;
    }
    out[(size_t)d * ld + i] = v;
}

// sigma_file for the 2-D cross-section tables (opacities_solvers/util.py:35-91): scipy's LinearNDInterpolator on the
// table's Delaunay triangulation, evaluated at the mesh (lambda_k, second_d) — second is T (H2+ bf) or 5040/T (H- ff).
// scipy (interpnd.pyx _evaluate_double, qhull.pyx _barycentric_coordinates): barycentric coordinates from Qhull's
// transform of the simplex, c_i = sum_j T[i][j] (x_j - T[2][j]), c_2 = 1 - c_0 - c_1; a point is inside when every
// c >= -eps (eps = 100 DBL_EPSILON); value = sum_j c_j v_j; outside the hull 0 (the reference's fill value).  The
// triangles of a rectilinear table lie two per cell, so the search is a cell look-up and at most two tests.
// scale_kind 1: x 1e-18 (:58); 2: x 1e-26 x k_B x T (:83-88).  zero_rows[d] is raised when a row holds an exact zero
// (the reference's "outside of interpolation range" warning, :59-62, :89-92).
constexpr int kTableAxisMax = 512;
__device__ __forceinline__ int last_le_clipped(const double* a, int n, double v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return max(0, min(lo - 1, n - 2));
}
__global__ __launch_bounds__(kBlock) void k_sigma_table_2d(int n_x, const double* __restrict__ x_axis, int n_y,
                                                           const double* __restrict__ y_axis, const int* __restrict__ cell_simplices,
                                                           const double* __restrict__ transform,
                                                           const double* __restrict__ simplex_values, int n_depth, int64_t n_nu,
                                                           const double* __restrict__ lambdas, const double* __restrict__ second,
                                                           int scale_kind, const double* __restrict__ temperature,
                                                           double* __restrict__ sigma, int64_t ld, int* __restrict__ zero_rows)
{
    __shared__ double s_x[kTableAxisMax];
    __shared__ int s_zero;
    for (int i = threadIdx.x; i < n_x; i += kBlock) s_x[i] = x_axis[i];
    if (threadIdx.x == 0) s_zero = 0;
    __syncthreads();
    const int d = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < n_nu) {
        const double qx = lambdas[k], qy = second[d];
        const int i = last_le_clipped(s_x, n_x, qx);
        const int j = last_le_clipped(y_axis, n_y, qy);
        constexpr double eps = 100.0 * 2.220446049250313e-16;
        double val = 0.0;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int sidx = cell_simplices[(i * (n_y - 1) + j) * 2 + c];
            const double* t = transform + (size_t)sidx * 6;
            const double dx = sub_rn(qx, t[4]), dy = sub_rn(qy, t[5]);
            const double c0 = add_rn(mul_rn(t[0], dx), mul_rn(t[1], dy));
            const double c1 = add_rn(mul_rn(t[2], dx), mul_rn(t[3], dy));
            const double c2 = sub_rn(sub_rn(1.0, c0), c1);
            if (c0 >= -eps && c1 >= -eps && c2 >= -eps && c0 <= 1.0 + eps && c1 <= 1.0 + eps && c2 <= 1.0 + eps) {
                const double* v = simplex_values + (size_t)sidx * 3;
                val = add_rn(add_rn(mul_rn(c0, v[0]), mul_rn(c1, v[1])), mul_rn(c2, v[2]));
                break;
            }
        }
        if (scale_kind == 1) val = mul_rn(val, 1e-18);
        else if (scale_kind == 2) val = mul_rn(mul_rn(mul_rn(val, 1e-26), kKB), temperature[d]);
        sigma[(size_t)d * ld + k] = val;
        if (val == 0.0) s_zero = 1;
    }
    __syncthreads();
    if (zero_rows && threadIdx.x == 0 && s_zero) zero_rows[d] = 1;
}

__global__ __launch_bounds__(kBlock) void k_rayleigh_clip(int64_t n_nu, double* __restrict__ nus)
{  // base.py:99: tracing_nus[tracing_nus > 2.3e15] = 0, in the caller's array
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n_nu && nus[i] > 2.3e15) nus[i] = 0.0;
}

__global__ __launch_bounds__(kBlock) void k_scale_rows(int n_depth, int64_t n_nu, const double* __restrict__ src, int64_t src_ld,
                                                       const double* __restrict__ density, double* __restrict__ out, int64_t ld)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int d = blockIdx.y;
    if (i < n_nu) out[(size_t)d * ld + i] = mul_rn(src[(size_t)d * src_ld + i], density[d]);
}

__global__ __launch_bounds__(kBlock) void k_scale(int n_depth, int64_t n_nu, double* __restrict__ a, int64_t ld, double factor)
{  // F_nu *= (r[-1] / reference_r)**2, radiation_field_solvers/base.py:340-344
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int d = blockIdx.y;
    if (i < n_nu) a[(size_t)d * ld + i] = mul_rn(a[(size_t)d * ld + i], factor);
}

__global__ __launch_bounds__(kBlock) void k_accumulate(int n_depth, int64_t n_nu, double* __restrict__ total, int64_t tld,
                                                       const double* __restrict__ src, int64_t sld)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int d = blockIdx.y;
    if (i < n_nu) total[(size_t)d * tld + i] = add_rn(total[(size_t)d * tld + i], src[(size_t)d * sld + i]);
}

// fused: total = ((((0 + file) + bf) + ff) + rayleigh) + electron) + line  (calc_alphas order, :655-738,
// then Opacities.calc_total_alphas insertion order, opacities/base.py:24-28).  `line` holds n_split partial
// planes [n_split][n_depth][line_ld] summed here in subset order; line_out (optional) receives that sum.
// The bound-free per-level coefficients of this block's depth are formed in LDS first (k_bf_coef's formula).
template <int NP = 1>
__device__ __forceinline__ void total_alphas_block(const int bx, const int d, int n_depth, int64_t nu_begin, int64_t nu_count,
                                                         const double* __restrict__ nus, ContinuumArgs a,
                                                         const double* __restrict__ line, int64_t line_ld, int n_split,
                                                         double* __restrict__ line_out, int64_t line_out_ld,
                                                         double* __restrict__ total, int64_t total_ld, const bool stage_table = false)
{
    extern __shared__ double s_coef[];  // [n_levels] for depth d, then (stage_table) the 1-D cross-section table
    const int n_levels = a.bf_n_species > 0 ? (a.bf_n_levels > 0 ? a.bf_n_levels : a.bf_species_offsets[a.bf_n_species]) : 0;  // host value: no load to wait for
    // the tabulated cross-section is searched per point: from LDS the bisection costs ~10x less latency than from L2
    double* s_xp = s_coef + n_levels;
    double* s_fp = s_xp + a.n_table;
    if (stage_table && a.table_sigma)
        for (int k = threadIdx.x; k < a.n_table; k += blockDim.x) {
            s_xp[k] = a.table_wavelength[k];
            s_fp[k] = a.table_sigma[k];
        }
    for (int L = threadIdx.x; L < n_levels; L += blockDim.x) {
        int sp = 0;
        while (sp + 1 < a.bf_n_species && L >= a.bf_species_offsets[sp + 1]) ++sp;
        const int zi = a.bf_species_ion_number[sp] + 1;
        const double r = mul_rn((double)zi, sqrt(kRydFreq / a.bf_cutoff[L]));
        const double r2 = mul_rn(r, r);
        const double n5 = mul_rn(mul_rn(r2, r2), r);
        s_coef[L] = mul_rn(mul_rn(kBfConst, (double)(zi * zi * zi * zi)), a.bf_level_density[(size_t)L * n_depth + d]) / n5;
    }
    __syncthreads();
#pragma unroll
    for (int pt = 0; pt < NP; ++pt) {
    const int64_t j = ((int64_t)bx * NP + pt) * blockDim.x + threadIdx.x;
    if (j < nu_count) {
    const int64_t i = nu_begin + j;
    const double nu = nus[i];
    double t = 0.0;
    if (a.table_sigma)
        t = add_rn(t, mul_rn(stage_table ? interp1(a.lambdas[i], a.n_table, s_xp, s_fp) : interp1(a.lambdas[i], a.n_table, a.table_wavelength, a.table_sigma),
                             a.table_density[d]));
    for (int k = 0; k < a.n_file_planes; ++k) t = add_rn(t, a.file_plane[k][(size_t)d * a.file_plane_ld + i]);  // (wave-uniform count and pointers)
    {
        double bf = 0.0;
        for (int sp = 0; sp < a.bf_n_species; ++sp) {
            double spec = 0.0;
            for (int L = a.bf_species_offsets[sp]; L < a.bf_species_offsets[sp + 1]; ++L)
                spec = add_rn(spec, nu >= a.bf_cutoff[L] ? s_coef[L] : 0.0);
            bf = add_rn(bf, spec);
        }
        t = add_rn(t, a.bf_n_species > 0 ? mul_rn(bf, inv_nu3(nu)) : 0.0);
    }
    t = add_rn(t, a.ff_n_species > 0 ? alpha_ff_point(n_depth, d, nu, a.temperature[d], a.ff_n_species, a.ff_species_ion_number, a.ff_number_density) : 0.0);
    if (a.rayleigh_enabled) t = add_rn(t, alpha_rayleigh_point(d, nu, a.ray_n_h, a.ray_n_he, a.ray_n_h2));
    if (a.electron_density) t = add_rn(t, mul_rn(kSigmaT, a.electron_density[d]));
    if (line) {
        double v = line[(size_t)d * line_ld + j];
        for (int s = 1; s < n_split; ++s) v = add_rn(v, line[((size_t)s * n_depth + d) * line_ld + j]);
        if (line_out) line_out[(size_t)d * line_out_ld + j] = v;
        t = add_rn(t, v);
    }
    total[(size_t)d * total_ld + j] = t;
    }
    }
    __syncthreads();  // s_coef may be refilled for another depth by the caller
}

__global__ __launch_bounds__(kBlock) void k_total_alphas(int n_depth, int64_t nu_begin, int64_t nu_count,
                                                         const double* __restrict__ nus, ContinuumArgs a,
                                                         const double* __restrict__ line, int64_t line_ld, int n_split,
                                                         double* __restrict__ line_out, int64_t line_out_ld,
                                                         double* __restrict__ total, int64_t total_ld)
{
    total_alphas_block(blockIdx.x, blockIdx.y, n_depth, nu_begin, nu_count, nus, a, line, line_ld, n_split, line_out, line_out_ld, total,
                       total_ld);
}

// The continuum plane of the fused step, one block per (tile of blockDim frequencies, group of kContDepths depths).  Everything
// that depends on the frequency alone — the tabulated cross-section (a bisection), nu^-3 (a division), the Rayleigh powers,
// which bound-free edges lie below nu — is formed ONCE per frequency and everything that depends on the depth alone — the
// bound-free coefficients (a division and a square root per level), the free-free sum (a division and a square root per
// species), the Rayleigh and Thomson factors — once per block in LDS; a (depth, frequency) point is then ~25 additions and
// multiplications, in calc_alphas' order and rounding (:655-700), where evaluating every point from scratch
// (total_alphas_block) costs ~400 instructions.
constexpr int kContDepths = 8;  // at most; the host picks 1..8 depths per block so that small grids still fill the chip
// PLANNED (sdx_grid_plan): the per-frequency part — the interpolated cross-section, nu^-3, the Rayleigh powers — was formed once by
// k_grid_plan_build with the operations below and lies in `pf` ([5][pld], indexed by the GLOBAL frequency): the tile stages no table,
// requests its frequency's values BEFORE the per-depth staging and its barrier instead of behind them, and keeps the bound-free edges
// in LDS beside the coefficients.  The point loop is the same.
template <bool PLANNED = false>
__device__ __forceinline__ void continuum_tile_block(const int tile, const int dg, const int dgs, int n_depth, int64_t nu_begin, int64_t nu_count,
                                                     const double* __restrict__ nus, ContinuumArgs a, double* __restrict__ cont,
                                                     int64_t cont_ld, const bool stage_table, const double* __restrict__ pf = nullptr,
                                                     int64_t pld = 0)
{
    extern __shared__ double s_mem[];
    const int n_levels = a.bf_n_species > 0 ? a.bf_n_levels : 0;
    double* s_coef = s_mem;                              // [kContDepths][n_levels]
    double* s_dep = s_coef + kContDepths * n_levels;     // [kContDepths][6]: file density, ff sum, Rayleigh c4 c6 c8, Thomson
    double* s_xp = s_dep + kContDepths * 6;              // (PLANNED: the bound-free edges [n_levels] instead of the table)
    double* s_fp = s_xp + a.n_table;
    const int d0 = dg * dgs;
    const int nd = min(dgs, n_depth - d0);
    [[maybe_unused]] double p_nu = 0.0, p_sig = 0.0, p_inv3 = 0.0, p_r4 = 0.0, p_r6 = 0.0, p_r8 = 0.0;
    if constexpr (PLANNED) {
        const int64_t pj = (int64_t)tile * blockDim.x + threadIdx.x;
        if (pj < nu_count) {
            const int64_t pi = nu_begin + pj;
            p_nu = nus[pi];
            if (a.table_sigma) p_sig = pf[pi];
            if (a.bf_n_species > 0 || a.ff_n_species > 0) p_inv3 = pf[pld + pi];
            if (a.rayleigh_enabled) p_r4 = pf[2 * pld + pi], p_r6 = pf[3 * pld + pi], p_r8 = pf[4 * pld + pi];
        }
    }
    if constexpr (!PLANNED)
    if (stage_table && a.table_sigma)
        for (int k = threadIdx.x; k < a.n_table; k += blockDim.x) {
            s_xp[k] = a.table_wavelength[k];
            s_fp[k] = a.table_sigma[k];
        }
    for (int k = threadIdx.x; k < nd * n_levels; k += blockDim.x) {
        const int dd = k / n_levels, L = k - dd * n_levels;
        int sp = 0;
        while (sp + 1 < a.bf_n_species && L >= a.bf_species_offsets[sp + 1]) ++sp;
        const int zi = a.bf_species_ion_number[sp] + 1;
        if constexpr (PLANNED) if (dd == 0) s_xp[L] = a.bf_cutoff[L];
        const double r = mul_rn((double)zi, sqrt(kRydFreq / a.bf_cutoff[L]));
        const double r2 = mul_rn(r, r);
        const double n5 = mul_rn(mul_rn(r2, r2), r);
        s_coef[dd * n_levels + L] = mul_rn(mul_rn(kBfConst, (double)(zi * zi * zi * zi)), a.bf_level_density[(size_t)L * n_depth + d0 + dd]) / n5;
    }
    if (threadIdx.x < nd) {
        const int d = d0 + threadIdx.x;
        double* dep = s_dep + threadIdx.x * 6;
        dep[0] = a.table_sigma ? a.table_density[d] : 0.0;
        double ff = 0.0;  // alpha_ff_point's sum (:274-317), the part in front of nu^-3
        for (int sp = 0; sp < a.ff_n_species; ++sp) {
            double v = a.ff_number_density[(size_t)sp * n_depth + d] / sqrt(a.temperature[d]);
            v = mul_rn(v, mul_rn(kFfConst, (double)(a.ff_species_ion_number[sp] * a.ff_species_ion_number[sp])));
            ff = add_rn(ff, v);
        }
        dep[1] = ff;
        double c4 = 0, c6 = 0, c8 = 0;  // alpha_rayleigh_point's per-depth sums (:74-135)
        if (a.rayleigh_enabled) {
            if (a.ray_n_h) { c4 = add_rn(c4, mul_rn(20.24, a.ray_n_h[d])); c6 = add_rn(c6, mul_rn(239.2, a.ray_n_h[d])); c8 = add_rn(c8, mul_rn(2256.0, a.ray_n_h[d])); }
            if (a.ray_n_he) { c4 = add_rn(c4, mul_rn(1.913, a.ray_n_he[d])); c6 = add_rn(c6, mul_rn(4.52, a.ray_n_he[d])); c8 = add_rn(c8, mul_rn(7.90, a.ray_n_he[d])); }
            if (a.ray_n_h2) { c4 = add_rn(c4, mul_rn(28.39, a.ray_n_h2[d])); c6 = add_rn(c6, mul_rn(215.0, a.ray_n_h2[d])); c8 = add_rn(c8, mul_rn(1303.0, a.ray_n_h2[d])); }
        }
        dep[2] = c4, dep[3] = c6, dep[4] = c8;
        dep[5] = a.electron_density ? mul_rn(kSigmaT, a.electron_density[d]) : 0.0;
    }
    __syncthreads();
    const int64_t j = (int64_t)tile * blockDim.x + threadIdx.x;
    if (j >= nu_count) return;
    const int64_t i = nu_begin + j;
    double nu, sig, inv3;
    double r4 = 0, r6 = 0, r8 = 0;
    if constexpr (PLANNED) {
        nu = p_nu, sig = p_sig, inv3 = p_inv3, r4 = p_r4, r6 = p_r6, r8 = p_r8;
    } else {
    nu = nus[i];
    sig = a.table_sigma ? (stage_table ? interp1(a.lambdas[i], a.n_table, s_xp, s_fp) : interp1(a.lambdas[i], a.n_table, a.table_wavelength, a.table_sigma)) : 0.0;
    inv3 = (a.bf_n_species > 0 || a.ff_n_species > 0) ? inv_nu3(nu) : 0.0;
    if (a.rayleigh_enabled) {
        const double nuc = nu > 2.3e15 ? 0.0 : nu;
        const double r = nuc / mul_rn(2.0, mul_rn(kC, kRydCm));
        const double r2 = mul_rn(r, r);
        r4 = mul_rn(r2, r2), r6 = mul_rn(r4, r2), r8 = mul_rn(r4, r4);
    }
    }
    const double* const cut = PLANNED ? s_xp : a.bf_cutoff;  // the bound-free edges: from LDS in a planned tile
    for (int dd = 0; dd < nd; ++dd) {
        const double* dep = s_dep + dd * 6;
        const double* coef = s_coef + dd * n_levels;
        double t = 0.0;
        if (a.table_sigma) t = add_rn(t, mul_rn(sig, dep[0]));
        for (int k = 0; k < a.n_file_planes; ++k) t = add_rn(t, a.file_plane[k][(size_t)(d0 + dd) * a.file_plane_ld + i]);
        double bf = 0.0;
        for (int sp = 0; sp < a.bf_n_species; ++sp) {
            double spec = 0.0;  // alpha_spec (:214), levels in plasma order (:221-233)
            for (int L = a.bf_species_offsets[sp]; L < a.bf_species_offsets[sp + 1]; ++L) spec = add_rn(spec, nu >= cut[L] ? coef[L] : 0.0);
            bf = add_rn(bf, spec);
        }
        t = add_rn(t, a.bf_n_species > 0 ? mul_rn(bf, inv3) : 0.0);
        t = add_rn(t, a.ff_n_species > 0 ? mul_rn(dep[1], inv3) : 0.0);
        if (a.rayleigh_enabled) t = add_rn(t, mul_rn(add_rn(add_rn(mul_rn(dep[2], r4), mul_rn(dep[3], r6)), mul_rn(dep[4], r8)), kSigmaT));
        if (a.electron_density) t = add_rn(t, dep[5]);
        cont[(size_t)(d0 + dd) * cont_ld + j] = t;
    }
}

// Frequencies per thread of a continuum block in the fused pre-pass launch (2 was measured: no gain).
// The pre-pass kernels cap their SGPRs at 80: a 1024-thread block is 4 waves per SIMD, and at the 94 SGPRs the compiler
// would use only ONE such block fits a CU (7 waves per SIMD), which ran this launch in three block generations at S-c2
// size (scripts/occupancy_probe.hip: two fit below 64 VGPRs and 81 SGPRs).
constexpr int kContPoints = 1;
// Pre-pass and continuum in ONE launch: the pre-pass is a few latency-bound blocks (binary searches, a grid scan);
// the continuum plane depends on nothing and fills the rest of the chip meanwhile.
template <bool GEN, int LINES, bool PLANNED = false>
__global__ __launch_bounds__(kPreBlock) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(8, 8))) void k_prepass_continuum(int n_pre_x, int n_pre_y, int cont_tiles, int n_depth, int64_t n_nu,
                                                              const double* __restrict__ nus,
                                                              const double* __restrict__ dnu_partial, int n_partial,
                                                              int64_t n_lines, const double* __restrict__ line_nus,
                                                              const double* __restrict__ doppler,
                                                              const double* __restrict__ gammas, int gamma_cols,
                                                              const double* __restrict__ alphas, LineWork w, int n_line_blocks,
                                                              int64_t nu_begin, int64_t nu_count, ContinuumArgs ca,
                                                              double* __restrict__ cont_plane, int64_t cont_ld, LineParams lp, int stage_table)
{
    const int b = blockIdx.x;
    const int n_pre = n_pre_x * n_pre_y;
    if (b < n_pre) {
        prepass_block<GEN, LINES, true, PLANNED>(b % n_pre_x, b / n_pre_x, n_pre_y, n_depth, n_nu, nus, dnu_partial, n_partial, n_lines, line_nus, doppler,
                           gammas, gamma_cols, alphas, w, nullptr, nullptr, n_line_blocks, lp);
    } else {
        const int c = b - n_pre;
#ifdef SDX_PRE_STATS
        const unsigned long long st0 = wall_clock64();
#endif
        if constexpr (PLANNED)  // (a planned launch always runs the tiled continuum)
            continuum_tile_block<true>(c % cont_tiles, c / cont_tiles, (stage_table >> 4) & 15, n_depth, nu_begin, nu_count, nus, ca, cont_plane, cont_ld,
                                       false, dnu_partial + kPlanFreqOffset, n_nu);
        else if (stage_table & 2)  // bit 1: depth-group blocks (the per-depth factors of a group fit LDS); bits 4..7: depths per block
            continuum_tile_block(c % cont_tiles, c / cont_tiles, (stage_table >> 4) & 15, n_depth, nu_begin, nu_count, nus, ca, cont_plane, cont_ld,
                                 (stage_table & 1) != 0);
        else
            total_alphas_block<kContPoints>(c % cont_tiles, c / cont_tiles, n_depth, nu_begin, nu_count, nus, ca, nullptr, 0, 1, nullptr, 0,
                                            cont_plane, cont_ld, (stage_table & 1) != 0);
#ifdef SDX_PRE_STATS
        if (threadIdx.x == 0) {
            unsigned long long* const o = g_pre_stats + (size_t)((kPreStatSlots / 2 + c) & (kPreStatSlots - 1)) * 8;
            o[0] = ((unsigned long long)c << 8) | 4 | 1;
            o[1] = st0;
            o[7] = wall_clock64();
        }
#endif
    }
}

// The grid plan (sdx_grid_plan_create / _refresh): everything the un-culled pre-pass launch forms from the grid, the line frequencies
// and the tabulated cross-section alone, once instead of in every step — by the step's own device functions, so the values are the
// step's.  Block 0: the grid spacing and its reciprocal (block_dnu_scan; a maximum is exact, so the partial maxima of k_dnu_partial on
// long grids give the same number); then one thread per line: its centre index #{i : nus[i] >= line_nu} (what the sampled search of
// prepass_block resolves to on a descending grid); one thread per entry of cnt_ge (the pixel blocks' bisection); one thread per
// frequency: interp1, inv_nu3 and the Rayleigh powers as continuum_tile_block forms them.
__global__ __launch_bounds__(kPreBlock) void k_grid_plan_build(int64_t n_nu, const double* __restrict__ nus, int64_t n_lines,
                                                               const double* __restrict__ line_nus, const double* __restrict__ lambdas, int n_table,
                                                               const double* __restrict__ table_wavelength, const double* __restrict__ table_sigma,
                                                               double* __restrict__ pd, int* __restrict__ cnt_ge, int* __restrict__ centre,
                                                               int n_line_blocks, int n_pix_blocks)
{
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    if (b == 0) {
        __shared__ double s_red[kPreBlock / 64];
        const double d_nu = block_dnu_scan(nus, n_nu, s_red);
        if (tid == 0) pd[0] = d_nu, pd[1] = 1.0 / d_nu;
        return;
    }
    b -= 1;
    if (b < n_line_blocks) {
        const int64_t l = (int64_t)b * kPreBlock + tid;
        if (l < n_lines) centre[l] = (int)closest_index(nus, n_nu, line_nus[l]);
        return;
    }
    b -= n_line_blocks;
    if (b < n_pix_blocks) {
        const int64_t pidx = (int64_t)b * kPreBlock + tid;
        if (pidx <= n_nu + 1) {
            int64_t cnt;
            if (pidx == 0) cnt = n_lines;
            else if (pidx == n_nu + 1) cnt = 0;
            else {
                const double v = nus[pidx - 1];
                int64_t lo = 0, hi = n_lines;  // first l with line_nus[l] > v
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (line_nus[mid] <= v) lo = mid + 1; else hi = mid;
                }
                cnt = lo;
            }
            cnt_ge[pidx] = (int)cnt;
        }
        return;
    }
    b -= n_pix_blocks;
    const int64_t i = (int64_t)b * kPreBlock + tid;
    if (i >= n_nu) return;
    double* const pf = pd + kPlanFreqOffset;
    const double nu = nus[i];
    pf[i] = table_sigma ? interp1(lambdas[i], n_table, table_wavelength, table_sigma) : 0.0;
    pf[n_nu + i] = inv_nu3(nu);
    const double nuc = nu > 2.3e15 ? 0.0 : nu;
    const double r = nuc / mul_rn(2.0, mul_rn(kC, kRydCm));
    const double r2 = mul_rn(r, r);
    const double r4 = mul_rn(r2, r2);
    pf[2 * n_nu + i] = r4, pf[3 * n_nu + i] = mul_rn(r4, r2), pf[4 * n_nu + i] = mul_rn(r4, r4);
}

// Culled shards of the fused step: the classification stream (HBM-bound, vector units idle) and the continuum plane (arithmetic,
// no traffic to speak of) in ONE launch of 256-thread blocks — blocks [0, n_dnu) the grid-spacing partials, then the continuum
// tiles, then the n_cls streaming blocks.
__global__ __launch_bounds__(kBlock) void k_classify_continuum(int n_dnu, int n_cls, int n_depth, int64_t n_nu, int64_t n_lines, double* __restrict__ dnu_partial,
                                                               const double* __restrict__ doppler, const double* __restrict__ gammas,
                                                               int gamma_cols, const double* __restrict__ alphas, double* __restrict__ m_max,
                                                               const double* __restrict__ nus, int cont_tiles, int64_t nu_begin, int64_t nu_count,
                                                               ContinuumArgs ca, double* __restrict__ cont_plane, int64_t cont_ld, int stage_table,
                                                               const double* __restrict__ line_nus, int64_t shard_begin, int64_t shard_count,
                                                               int* __restrict__ sel, int64_t cls_begin, int64_t cls_end, FarReq far)
{
    // order of the roles in the grid = order of dispatch: the continuum tiles — chains of dependent work (coefficients, a barrier,
    // a table search), eight depths per block so that they are few and long — go first and run behind the stream (round 4, an
    // eighth of S-c3: this launch 62 us with one depth per block, 46 with eight; tiles first or last: 46 / 47)
    const int n_cont = (int)gridDim.x - n_dnu - n_cls;
    const int b = blockIdx.x;
    if (b < n_dnu) {
        __shared__ double s_red[kBlock / 64];
        dnu_partial_block(b, n_dnu, n_nu, nus, dnu_partial, s_red, far);
    } else if (b < n_dnu + n_cont) {
        const int c = b - n_dnu;
        continuum_tile_block(c % cont_tiles, c / cont_tiles, (stage_table >> 4) & 15, n_depth, nu_begin, nu_count, nus, ca, cont_plane, cont_ld,
                             (stage_table & 1) != 0);
    } else {
        const int k = b - n_dnu - n_cont;
        if (sel && k == n_cls - 1) shard_range(n_nu, nus, n_lines, line_nus, shard_begin, shard_count, sel);  // (four threads, on the side)
        classify_block(k, n_cls, n_depth, cls_begin, cls_end, doppler, gammas, gamma_cols, alphas, m_max);
    }
}

// ------------------------------------------------------------------------------------------------
// Formal solution (radiation_field_solvers/base.py:85-346).  A group of G adjacent lanes of one wave
// owns one frequency (64/G groups per wave); lane g of the group traces angle g through all depth gaps,
// keeping the rolling state — two mean opacities, three source values, one intensity — in registers.
// After every gap the group sums I_theta * w_theta in ascending-theta order with wave shuffles and lane 0
// adds it to F_nu[gap+1] (:336-338).  Geometric-mean opacity (:121), tau (:123-129), Planck source (:133)
// and the weights (:138) are formed with the reference's operations.
//
// One angle per lane, here and in k_raytrace, k_raytrace_cont and k_contribution (two and four: measured slower, removed).
// The lane's state stays one-element arrays walked by one-trip loops over k ON PURPOSE: with them the compiler emits, instruction for
// instruction, the code every recorded time was measured on; as scalars, or as the same arrays indexed by 0, all four kernels come out
// in another order and three of them longer (k_raytrace by 18 instructions; profiles/EXPERIMENTS.md): a change that has to be measured.
__global__ __launch_bounds__(kBlock) void k_raytrace_basic(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                     const double* __restrict__ nus, const double* __restrict__ temps,
                                                     const double* __restrict__ ray_dist, const double* __restrict__ wts,
                                                     const double* __restrict__ alphas, int64_t ald, double* __restrict__ F,
                                                     int64_t fld, double* __restrict__ I_nus, int accumulate)
{
    constexpr int P = 1;  // angles per lane: the note above
    // n_theta angles are traced here; ray_dist / I_nus rows have theta_stride entries (a chunk of a longer list)
    const int lane = threadIdx.x & 63;
    const int gpw = 64 / G;  // groups per wave
    const int grp = lane / G, g = lane - grp * G;
    const int64_t i = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * gpw + grp;
    const bool valid = grp < gpw && i < n_nu;
    const int64_t ic = i < n_nu ? i : n_nu - 1;
    const int lane0 = lane - g;
    const int n_gap = n_depth - 1;
    const double nu = nus[ic];

    double la0 = log(alphas[ic]);                                 // log alpha[gap]
    double la1 = log(alphas[(size_t)ald + ic]);                   // log alpha[gap+1]
    double mean0 = exp(mul_rn(add_rn(la1, la0), 0.5));            // :121
    double s0 = planck(nu, temps[0]), s1 = planck(nu, temps[1]);  // :133
    double inten[P], wt[P];
    int th[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        inten[k] = 0.0;  // I[0] = 0 (:134-136)
        th[k] = g;
        wt[k] = th[k] < n_theta ? wts[th[k]] : 0.0;
        if (valid && I_nus && th[k] < n_theta) I_nus[(size_t)i * theta_stride + th[k]] = 0.0;
    }

    for (int gap = 0; gap < n_gap; ++gap) {
        const bool last = gap == n_gap - 1;
        double mean1 = 0.0, s2 = 0.0, la2 = 0.0;
        if (!last) {
            la2 = log(alphas[(size_t)(gap + 2) * ald + ic]);
            mean1 = exp(mul_rn(add_rn(la2, la1), 0.5));
            s2 = planck(nu, temps[gap + 2]);
        }
        double fsum = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if (th[k] < n_theta) {
                const double tau0 = mul_rn(mean0, ray_dist[(size_t)gap * theta_stride + th[k]]);
                double inew;
                if (tau0 == 0.0) {
                    inew = inten[k];  // :203-206, :253-254
                } else {
                    double w0, w1, w2;
                    rt_weights(tau0, w0, w1, w2);
                    if (!last) {  // :208-249
                        const double tau1 = mul_rn(mean1, ray_dist[(size_t)(gap + 1) * theta_stride + th[k]]);
                        const double sum01 = add_rn(tau0, tau1);
                        const double second =
                            mul_rn(w1, sub_rn(mul_rn(sub_rn(s1, s2), tau0 / tau1), mul_rn(sub_rn(s1, s0), tau1 / tau0))) / sum01;
                        const double third = mul_rn(w2, add_rn(sub_rn(s2, s1) / tau1, sub_rn(s0, s1) / tau0)) / sum01;
                        inew = add_rn(add_rn(add_rn(mul_rn(sub_rn(1.0, w0), inten[k]), mul_rn(w0, s1)), second), third);
                    } else {  // :256-266
                        const double third = mul_rn(w2, sub_rn(s0, s1)) / mul_rn(tau0, tau0);
                        inew = add_rn(add_rn(mul_rn(sub_rn(1.0, w0), inten[k]), mul_rn(w0, s1)), third);
                    }
                }
                inten[k] = inew;
                if (valid && I_nus) I_nus[((size_t)(gap + 1) * n_nu + i) * theta_stride + th[k]] = inew;
            }
        }
        if (F) {
            if (G == 1) {
#pragma unroll
                for (int k = 0; k < P; ++k)
                    if (th[k] < n_theta) fsum = add_rn(fsum, mul_rn(inten[k], wt[k]));
            } else {
                // ascending theta: the group's lanes in order
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    const double mine = mul_rn(inten[k], wt[k]);
                    for (int gg = 0; gg < G; ++gg) {
                        const double v = __shfl(mine, lane0 + gg);
                        if (gg < n_theta) fsum = add_rn(fsum, v);
                    }
                }
            }
            if (valid && g == 0) {
                double* p = F + (size_t)(gap + 1) * fld + i;
                *p = accumulate ? add_rn(*p, fsum) : fsum;
                if (gap == 0 && !accumulate) F[i] = 0.0;
            }
        }
        la0 = la1; la1 = la2; mean0 = mean1; s0 = s1; s1 = s2;
    }
}

// ------------------------------------------------------------------------------------------------
// Formal solution, LDS-staged (the default).  Same lane <-> (frequency, angle) mapping as k_raytrace_basic:
// a group of G adjacent lanes owns one frequency, lane g traces angle g.  What is shared is
// prepared once and kept in LDS:
//   block    the ray-length table ray_dist[gap][theta] (:302-305) and its reciprocals;
//   group    phase 1: the G lanes split the N_d depth points: log(alpha) and the Planck source S (:133) -> LDS,
//            then per gap the geometric-mean opacity exp((log a[g+1] + log a[g]) * 0.5) (:121) and its reciprocal;
//   lane     phase 2: walks the gaps for its own angle: tau = mean * ray_dist (:123-129, the reference's
//            product), weights (:22-45), second-order recurrence (:200-266).  The divisions of :208-242 are
//            re-expressed with the slopes a = (S[g+2]-S[g+1])/tau[g+1], b = (S[g]-S[g+1])/tau[g]:
//                second = w1 (b tau[g+1] - a tau[g]) / (tau[g] + tau[g+1]),   third = w2 (a + b) / (tau[g] + tau[g+1])
//            with 1/tau formed as (1/mean)(1/ray_dist) — shared across angles / frequencies — and one reciprocal
//            per step for the sum.  tau = 0 gives the same inf/NaN pattern as the reference's unguarded divisions.
//   flux     I_theta * w_theta goes to LDS; every kBatch gaps the wave sums each (gap, frequency) over theta in
//            ascending order (the reference's order, :324-338) and writes F_nu.

// Optional fusion of Opacities.calc_total_alphas into the raytrace's column staging: total = continuum + line,
// line = sum of the partial planes in subset order (the same additions k_total_alphas performs).
struct FusedTotal {
    const double* cont;    // [n_depth][cld] continuum in calc_alphas order, or nullptr: read `alphas` instead
    int64_t cld;
    const double* planes;  // [n_planes][n_depth][pld] partial line-opacity planes, or nullptr (no lines)
    int n_planes;
    int64_t pld;
    double* total_out;     // [n_depth][out_ld], optional
    double* line_out;      // optional
    int64_t out_ld;
    // source function given by the caller as a plane [n_depth][sld] (RadiationField.source_function is any callable
    // (nu, T) -> (N_d, N_nu), radiation_field_solvers/base.py:133); nullptr: the Planck function, evaluated here
    const double* source;
    int64_t sld;
    // further line-opacity planes [n_depth][eld] the caller has formed (the molecular list of include_molecules,
    // opacities_solvers/base.py:716-736), added after the step's own line opacity in this order: total = (cont + line) + extra...
    const double* extra[2];
    int n_extra;
    int64_t eld;
};

// Formal solution, LDS-staged (grids that fill the chip; every geometry).  Lane <-> (frequency, angle): a group of G adjacent
// lanes owns one frequency, lane g traces angle g.  Staged once and kept in LDS:
//   block    the ray-length table ray_dist[gap][theta] (:302-305);
//   wave     per frequency of the wave, the G lanes of its group split the N_d depth points: the source function S (:133;
//            planck_staged, or the caller's plane) and sqrt(alpha).  The geometric-mean opacity of a gap (:121,
//            exp((log a[g+1] + log a[g]) / 2)) is the product of the two square roots at its ends — one correctly rounded
//            square root per point instead of a logarithm per point and an exponential per gap, and within 1e-15 of the
//            reference's value (whose own error is ~|log alpha| ulp);
//   lane     walks the gaps for its own angle: tau = mean * ray_dist (:123-129), then one rt_coef (sdx_math.h: the
//            step as an affine map of the incoming intensity, one reciprocal, the reference's weights) and one FMA;
//   flux     I_theta * w_theta goes to the wave's LDS; every kBatch gaps the wave sums each (gap, frequency) over theta in
//            two ascending halves and writes F_nu.
// Only the ray table is shared by the block: after the staging barrier the waves never meet again (wave-level hand-overs).
// kRtBlock and the LDS layout of every kernel of the family: sdx_rt_layout.h.
// lane / G for lane < 64 and 1 <= G <= 64 without an integer division (~25 instructions where G is a kernel argument): one multiply
// by g_recip = 65536 / G + 1, formed once on the host (lane_recip, stardis_hip.hip), and a shift.  Exact over that whole range.
// (k_raytrace_seg, whose prologue is a visible share of a wave's life; k_raytrace and k_raytrace_cont keep the division)
__device__ __forceinline__ int lane_div(int lane, int g_recip)
{
    return (lane * g_recip) >> 16;
}
__global__ __launch_bounds__(kRtBlock) void k_raytrace(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                     const double* __restrict__ nus, const double* __restrict__ temps,
                                                     const double* __restrict__ ray_dist, const double* __restrict__ wts,
                                                     const double* __restrict__ alphas, int64_t ald, double* __restrict__ F,
                                                     int64_t fld, double* __restrict__ I_nus, int accumulate, int inward, int gpw, FusedTotal ft)
{
    constexpr int P = 1, kBatch = kRtBatch;  // P: angles per lane (why the one-trip loops over k stay: the note above k_raytrace_basic)
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // gpw = groups (frequencies) per wave, <= 64 / G; the host lowers it when the LDS columns would not fit
    const int grp = lane / G, g = lane - grp * G;
    const int64_t i0 = ((int64_t)blockIdx.x * (kRtBlock / 64) + wave) * gpw;  // first frequency of this wave
    const int64_t i = i0 + grp;
    const bool active = grp < gpw;
    const bool valid = active && i < n_nu;
    const int64_t ic = i < n_nu ? i : n_nu - 1;
    const int n_gap = n_depth - 1;
    const int col = n_depth;  // LDS row stride per group
    const RtColumns lay(G, n_depth, gpw);
    double* wbase = smem + (size_t)wave * lay.wave_doubles();
    double2* sP = (double2*)(wbase + lay.pairs());  // (source function, sqrt(alpha)) [gpw][col]: a point's pair is ONE 16-byte LDS read
    double* sX = wbase + lay.flux();                // flux terms       [kBatch][gpw][G]
    const double nu = nus[ic];

    // (Staging the columns a batch of G depth points AHEAD of the recurrence — the loads of batch b + 1 requested when batch b is
    // committed, so that a shard's single generation of workgroups does not wait for all its planes before any wave computes — was
    // built and measured in round 5: k_raytrace 60 - 91 us instead of 55 - 84 on the eighths of S-c3 and 428 instead of 377 on the
    // whole grid.  The commit inside the gap loop needs the loop's registers: 46 spilled VGPRs at seven waves per SIMD, and a lone
    // generation is bound by the 55-step chain of each wave, not by its staging.  Removed.)
    if (active) {
        for (int d = g; d < n_depth; d += G) {
            double a;
            if (ft.cont) {
                a = ft.cont[(size_t)d * ft.cld + ic];
                if (ft.planes) {
                    double line = ft.planes[(size_t)d * ft.pld + ic];
                    for (int sp = 1; sp < ft.n_planes; ++sp) line = add_rn(line, ft.planes[((size_t)sp * n_depth + d) * ft.pld + ic]);
                    a = add_rn(a, line);
                    if (valid && ft.line_out) ft.line_out[(size_t)d * ft.out_ld + i] = line;
                }
                for (int x = 0; x < ft.n_extra; ++x) a = add_rn(a, ft.extra[x][(size_t)d * ft.eld + ic]);
                if (valid && ft.total_out) ft.total_out[(size_t)d * ft.out_ld + i] = a;
            } else {
                a = alphas[(size_t)d * ald + ic];
            }
            sP[grp * col + d] = double2{ft.source ? ft.source[(size_t)d * ft.sld + ic] : planck_staged(nu, temps[d]), sqrt(a)};
        }
    }
    wave_sync();  // (nothing is shared between the waves of a block any more: the ray table is read from L1)
    // (the step's constants stay literals here: the gap loop is rolled and the compiler already holds them in scalar registers across it
    // — no literal move in the loop body; pinned with rt_const_resident they cost k_raytrace five more SGPR spills and put two moves back)
    const RtConst kc = rt_const_literals();

    const int gi = (active ? grp : 0) * col;  // idle lanes shadow group 0 and never store
    double inten[P], wt[P];
    int th[P];
    bool on[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        th[k] = min(g, n_theta - 1);
        on[k] = g < n_theta;
        inten[k] = 0.0;  // np.zeros (:134)
        wt[k] = on[k] ? wts[th[k]] : 0.0;
    }
    if (inward) {
        // spherical geometry: sweep from the surface to the innermost point first (:141-198).  Only I[0] of this
        // sweep survives (the outward pass overwrites the other rows); gap 0 wraps to the LAST gap / depth exactly
        // as the reference's negative index does.  Either optical depth zero: no change (:146-149).
        for (int gap = n_gap - 1; gap >= 0; --gap) {
            const int gm = gap > 0 ? gap - 1 : n_gap - 1;
            const int dm = gap > 0 ? gap - 1 : n_depth - 1;
            const double2 q0 = sP[gi + gap + 1], q1 = sP[gi + gap], q2 = sP[gi + dm];
            const double s0 = q0.x, s1 = q1.x, s2 = q2.x;
            const double mg = q1.y * q0.y, mm = sP[gi + gm].y * sP[gi + gm + 1].y;
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const double tg = mul_rn(mg, ray_dist[(size_t)gap * theta_stride + th[k]]), tm = mul_rn(mm, ray_dist[(size_t)gm * theta_stride + th[k]]);
                double c, e;
                rt_coef<false>(tg, tm, s0 - s1, s2 - s1, s1, c, e, kc);
                inten[k] = tm == 0.0 ? inten[k] : fma(c, inten[k], e);
            }
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if (valid && I_nus && on[k]) I_nus[(size_t)i * theta_stride + th[k]] = inten[k];
            if (active) sX[grp * G + g] = inten[k] * wt[k];
        }
        wave_sync();
        if (F && lane < gpw && i0 + lane < n_nu) {
            double sum = 0.0;
            for (int t = 0; t < n_theta; ++t) sum = add_rn(sum, sX[lane * G + t]);
            double* dst = F + i0 + lane;
            *dst = accumulate ? add_rn(*dst, sum) : sum;
        }
        wave_sync();
    } else {
#pragma unroll
        for (int k = 0; k < P; ++k)
            if (valid && I_nus && on[k]) I_nus[(size_t)i * theta_stride + th[k]] = 0.0;
        if (valid && g == 0 && F && !accumulate) F[i] = 0.0;
    }
    // rolling state: optical depth of the current gap per angle, source at its two ends, sqrt(alpha) at its far end
    // (the ray-length table — 9 KB at 56 depths x 20 angles — is read from global memory, i.e. the L1: a lane needs ONE entry
    // per gap, requested a gap ahead; staged in LDS it cost every block 9 KB, and with them two of seven workgroups per CU)
    double tau0[P], rd_next[P];
    const double* rdp[P];
    const double2 p0 = sP[gi], p1 = sP[gi + 1];
    double a1 = p1.y;
    {
        const double mean0 = p0.y * a1;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            rdp[k] = ray_dist + th[k];
            tau0[k] = mul_rn(mean0, *rdp[k]);
            rdp[k] += n_gap > 1 ? theta_stride : 0;
            rd_next[k] = *rdp[k];  // gap 1
        }
    }
    double s1 = p1.x, d10 = p0.x - s1;
    const float inv_gpw = 1.0f / (float)gpw;

    for (int gap0 = 0; gap0 < n_gap; gap0 += kBatch) {
        const int nb = min(kBatch, n_gap - gap0);
        for (int b = 0; b < nb; ++b) {
            const int gap = gap0 + b;
            if (gap < n_gap - 1) {  // :208-249
                const double2 p2 = sP[gi + gap + 2];
                const double s2 = p2.x, a2 = p2.y;
                const double mean1 = a1 * a2, d21 = s2 - s1;
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    const double t1 = mul_rn(mean1, rd_next[k]);
                    rdp[k] += gap + 2 < n_gap ? theta_stride : 0;
                    rd_next[k] = *rdp[k];  // gap + 2, for the next trip
                    double c, e;
                    rt_coef<false>(tau0[k], t1, d10, d21, s1, c, e, kc);
                    const double inew = fma(c, inten[k], e);
                    inten[k] = inew;
                    tau0[k] = t1;
                    if (valid && I_nus && on[k]) I_nus[((size_t)(gap + 1) * n_nu + i) * theta_stride + th[k]] = inew;
                    if (active) sX[(b * gpw + grp) * G + g] = inew * wt[k];
                }
                d10 = -d21, s1 = s2, a1 = a2;
            } else {  // the final gap (:253-266)
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    double c, e;
                    rt_coef<true>(tau0[k], 0.0, d10, 0.0, s1, c, e, kc);
                    const double inew = fma(c, inten[k], e);
                    inten[k] = inew;
                    if (valid && I_nus && on[k]) I_nus[((size_t)(gap + 1) * n_nu + i) * theta_stride + th[k]] = inew;
                    if (active) sX[(b * gpw + grp) * G + g] = inew * wt[k];
                }
            }
        }
        wave_sync();
        if (F) {
            // flux of the nb gaps: lanes <-> (gap, frequency, half of the angles); each half is summed in ascending theta
            // (the reference's order, :324-338) and the lower half is added to the upper one
            const int half = (n_theta + 1) >> 1;
            for (int p = lane; p < 2 * nb * gpw; p += 64) {
                const int h = p & 1, q = p >> 1;
                const int b = (int)(((float)q + 0.5f) * inv_gpw), gq = q - b * gpw;  // q / gpw without an integer division (q < 2^20: exact)
                const double* c = sX + (b * gpw + gq) * G + (h ? half : 0);
                const int cnt = h ? n_theta - half : half;
                double sum = 0.0;
                int t = 0;
                for (; t + 5 <= cnt; t += 5) {  // five terms a trip (their loads in flight together), added in ascending order
                    const double c0 = c[t], c1 = c[t + 1], c2 = c[t + 2], c3 = c[t + 3], c4 = c[t + 4];
                    sum = add_rn(add_rn(add_rn(add_rn(add_rn(sum, c0), c1), c2), c3), c4);
                }
                for (; t < cnt; ++t) sum = add_rn(sum, c[t]);
                const double other = __shfl_xor(sum, 1);  // 2 nb gpw is even: the partner lane is in the loop too
                const int64_t iq = i0 + gq;
                if (h == 0 && iq < n_nu) {
                    const double tot = add_rn(sum, other);
                    double* dst = F + (size_t)(gap0 + b + 1) * fld + iq;
                    *dst = accumulate ? add_rn(*dst, tot) : tot;
                }
            }
        }
        wave_sync();
    }
}

// The emergent intensity of every ray (include/stardis_hip.h, sdx_emergent_intensity_dev): k_raytrace's walk — the same lane <->
// (frequency, angle) mapping, the same RtColumns staging of (S, sqrt(alpha)) from a FINISHED total_alphas plane, the inward sweep where
// asked for, rt_coef<false> per inner gap and rt_coef<true> for the last, each on the operands k_raytrace forms, in its order — that keeps
// the last row alone: no flux, no weights, no I_nus volume.  What a lane holds after the last gap is row N_d - 1 of k_raytrace's I_nus bit
// for bit.  The output is theta-major, I_out[theta][ild] (a ring's spectrum contiguous for k_disk_integrate): the wave parks its
// gpw x G values in the flux region of its LDS share and writes them out angle by angle, consecutive lanes consecutive frequencies.
__global__ __launch_bounds__(kRtBlock) void k_emergent_intensity(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                               const double* __restrict__ nus, const double* __restrict__ temps,
                                                               const double* __restrict__ ray_dist, const double* __restrict__ alphas,
                                                               int64_t ald, const double* __restrict__ source, int64_t sld, int inward,
                                                               double* __restrict__ I_out, int64_t ild, int gpw)
{
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane / G, g = lane - grp * G;
    const int64_t i0 = ((int64_t)blockIdx.x * (kRtBlock / 64) + wave) * gpw;  // first frequency of this wave
    const int64_t i = i0 + grp;
    const bool active = grp < gpw;
    const int64_t ic = i < n_nu ? i : n_nu - 1;
    const int n_gap = n_depth - 1;
    const int col = n_depth;
    const RtColumns lay(G, n_depth, gpw);
    double* wbase = smem + (size_t)wave * lay.wave_doubles();
    double2* sP = (double2*)(wbase + lay.pairs());  // (source function, sqrt(alpha)) [gpw][col]
    double* sX = wbase + lay.flux();                // the emergent intensities [gpw][G] (the first of the kRtBatch flux slots)
    const double nu = nus[ic];
    if (active) {
        for (int d = g; d < n_depth; d += G)
            sP[grp * col + d] = double2{source ? source[(size_t)d * sld + ic] : planck_staged(nu, temps[d]), sqrt(alphas[(size_t)d * ald + ic])};
    }
    wave_sync();
    const RtConst kc = rt_const_literals();  // (literals, as in k_raytrace: the gap loop is rolled)

    const int gi = (active ? grp : 0) * col;  // idle lanes shadow group 0 and never store
    const int th = min(g, n_theta - 1);
    double inten = 0.0;  // np.zeros (:134)
    if (inward) {        // the surface-to-centre sweep of k_raytrace (:141-198)
        for (int gap = n_gap - 1; gap >= 0; --gap) {
            const int gm = gap > 0 ? gap - 1 : n_gap - 1;
            const int dm = gap > 0 ? gap - 1 : n_depth - 1;
            const double2 q0 = sP[gi + gap + 1], q1 = sP[gi + gap], q2 = sP[gi + dm];
            const double s0 = q0.x, s1 = q1.x, s2 = q2.x;
            const double mg = q1.y * q0.y, mm = sP[gi + gm].y * sP[gi + gm + 1].y;
            const double tg = mul_rn(mg, ray_dist[(size_t)gap * theta_stride + th]), tm = mul_rn(mm, ray_dist[(size_t)gm * theta_stride + th]);
            double c, e;
            rt_coef<false>(tg, tm, s0 - s1, s2 - s1, s1, c, e, kc);
            inten = tm == 0.0 ? inten : fma(c, inten, e);
        }
    }
    const double2 p0 = sP[gi], p1 = sP[gi + 1];
    double a1 = p1.y;
    const double* rdp = ray_dist + th;
    double tau0 = mul_rn(p0.y * a1, *rdp);
    rdp += n_gap > 1 ? theta_stride : 0;
    double rd_next = *rdp;  // gap 1
    double s1 = p1.x, d10 = p0.x - s1;
    for (int gap = 0; gap < n_gap; ++gap) {
        double c, e;
        if (gap < n_gap - 1) {  // :208-249
            const double2 p2 = sP[gi + gap + 2];
            const double s2 = p2.x, a2 = p2.y;
            const double mean1 = a1 * a2, d21 = s2 - s1;
            const double t1 = mul_rn(mean1, rd_next);
            rdp += gap + 2 < n_gap ? theta_stride : 0;
            rd_next = *rdp;  // gap + 2, for the next trip
            rt_coef<false>(tau0, t1, d10, d21, s1, c, e, kc);
            inten = fma(c, inten, e);
            tau0 = t1;
            d10 = -d21, s1 = s2, a1 = a2;
        } else {  // the final gap (:253-266)
            rt_coef<true>(tau0, 0.0, d10, 0.0, s1, c, e, kc);
            inten = fma(c, inten, e);
        }
    }
    if (active) sX[grp * G + g] = inten;
    wave_sync();
    // theta-major: entry p <-> (angle p / gpw, frequency p % gpw) of the wave; gpw n_theta <= 64 entries, so t < n_theta and f < gpw
    const float inv_gpw = 1.0f / (float)gpw;
    for (int p = lane; p < n_theta * gpw; p += 64) {
        const int t = (int)(((float)p + 0.5f) * inv_gpw), f = p - t * gpw;  // p / gpw without an integer division (p < 2^20: exact)
        if (i0 + f < n_nu) I_out[(size_t)t * ild + i0 + f] = sX[f * G + t];
    }
}

// The formal solution of the fp32-mixed TOLERANCE path (mixed_precision = 1; plane-parallel, one angle per lane, flux only): the
// layout of k_raytrace — lane <-> (frequency, angle), columns staged per wave — with the recurrence in fp32 (rt_coef32:
// hardware exp2 / rcp, ~27 instructions per step at twice the fp64 issue rate against ~54).  sqrt(alpha), the source function, its
// differences between adjacent points (formed as differences: planck32_pair) and the ray lengths are staged as floats (the totals
// are formed in fp64 and rounded once); F_nu is written as doubles.
// Against the fp64 kernels: < 1e-5 of the flux on the full-size workloads (tests/test_gpu_configs.py, stated tolerance 1e-4).
__global__ __launch_bounds__(kRtBlock) void k_raytrace_f32(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                           const double* __restrict__ nus, const double* __restrict__ temps,
                                                           const double* __restrict__ ray_dist, const double* __restrict__ wts,
                                                           const double* __restrict__ alphas, int64_t ald, double* __restrict__ F,
                                                           int64_t fld, int gpw, FusedTotal ft)
{
    constexpr int kBatch = kRt32Batch;
    extern __shared__ double smem[];
    float* fmem = (float*)smem;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane / G, g = lane - grp * G;
    const int64_t i0 = ((int64_t)blockIdx.x * (kRtBlock / 64) + wave) * gpw;
    const int64_t i = i0 + grp;
    const bool active = grp < gpw;
    const bool valid = active && i < n_nu;
    const int64_t ic = i < n_nu ? i : n_nu - 1;
    const int n_gap = n_depth - 1, col = n_depth;
    const RtF32Columns lay(n_theta, G, n_depth, gpw);
    float* sRD = fmem + lay.ray_table();                 // ray_dist [n_gap][n_theta], shared by the block
    float* sK = fmem + lay.inv_kt();                     // 1 / (k T_d) [col], shared by the block
    float* sR = fmem + lay.dtemp();                      // (T_d - T_{d+1}) / T_{d+1} [col]: the difference formed in fp64
    // per wave: what a step of the recurrence needs of its NEXT point as ONE 16-byte LDS read — sP[k] = (sqrt(alpha_{k+1}), S_{k+1},
    // S_k - S_{k+1}, -) for k < n_gap, the difference formed as a difference (planck32_pair), not from the two rounded values; the
    // first point's (sqrt(alpha_0), S_0) in the spare slot k = n_gap
    float* wbase = fmem + lay.shared_floats() + (size_t)wave * lay.wave_floats();
    float4* sP = (float4*)(wbase + lay.points());        // [gpw][col]
    float* sX = wbase + lay.flux();                      // flux terms [kBatch][gpw][G]
    const double nu = nus[ic];
    for (int k = threadIdx.x; k < n_gap * n_theta; k += kRtBlock) {
        const int gp = k / n_theta, t = k - gp * n_theta;
        sRD[k] = (float)ray_dist[(size_t)gp * theta_stride + t];
    }
    for (int k = threadIdx.x; k < n_depth; k += kRtBlock) {
        const double t = temps[k], tn = temps[min(k + 1, n_depth - 1)];
        sK[k] = __builtin_amdgcn_rcpf((float)mul_rn(kKB, t));
        sR[k] = (float)sub_rn(t, tn) * __builtin_amdgcn_rcpf((float)tn);
    }
    __syncthreads();
    if (active) {
        const float hn = (float)mul_rn(kH, nu);
        const float pre = (float)(mul_rn(mul_rn(2.0, kH), mul_rn(mul_rn(nu, nu), nu)) * (1.0 / (kC * kC)));
        for (int d = g; d < n_depth; d += G) {
            double a;
            if (ft.cont) {
                a = ft.cont[(size_t)d * ft.cld + ic];
                if (ft.planes) {
                    double line = ft.planes[(size_t)d * ft.pld + ic];
                    for (int sp = 1; sp < ft.n_planes; ++sp) line = add_rn(line, ft.planes[((size_t)sp * n_depth + d) * ft.pld + ic]);
                    a = add_rn(a, line);
                    if (valid && ft.line_out) ft.line_out[(size_t)d * ft.out_ld + i] = line;
                }
                for (int x = 0; x < ft.n_extra; ++x) a = add_rn(a, ft.extra[x][(size_t)d * ft.eld + ic]);
                if (valid && ft.total_out) ft.total_out[(size_t)d * ft.out_ld + i] = a;
            } else {
                a = alphas[(size_t)d * ald + ic];
            }
            const float sa = __builtin_sqrtf((float)a);
            const int dn = min(d + 1, n_depth - 1);
            float sv, dv;
            if (ft.source) {
                const double s0 = ft.source[(size_t)d * ft.sld + ic];
                sv = (float)s0, dv = (float)sub_rn(s0, ft.source[(size_t)dn * ft.sld + ic]);
            } else {
                planck32_pair(hn, pre, sK[d], sK[dn], sR[d], sv, dv);
            }
            float* const mine = (float*)(sP + grp * col + (d > 0 ? d - 1 : n_gap));
            mine[0] = sa, mine[1] = sv;
            ((float*)(sP + grp * col + d))[2] = dv;  // (slot n_gap: the last point's 0, never read)
        }
    }
    __syncthreads();
    const int gi = (active ? grp : 0) * col;
    const int th = min(g, n_theta - 1);
    const float wt = g < n_theta ? (float)wts[th] : 0.f;
    if (valid && g == 0) F[i] = 0.0;
    float inten = 0.f;
    const float4 p0 = sP[gi];
    float a1 = p0.x;
    float t0 = (sP[gi + n_gap].x * a1) * sRD[th];
    float s1 = p0.y, d10 = p0.z;
    const float inv_gpw = 1.0f / (float)gpw;
    for (int gap0 = 0; gap0 < n_gap; gap0 += kBatch) {
        const int nb = min(kBatch, n_gap - gap0);
        for (int b = 0; b < nb; ++b) {
            const int gap = gap0 + b;
            const bool last = gap == n_gap - 1;
            const int nx = last ? gap : gap + 1;
            const float4 p = sP[gi + nx];
            const float s2 = p.y, a2 = p.x;
            const float t1 = (a1 * a2) * sRD[nx * n_theta + th];
            const float d21 = last ? 0.f : -p.z;
            float c, e;
            rt_coef32(t0, t1, d10, d21, s1, last, c, e);
            inten = fmaf(c, inten, e);
            if (active) sX[(b * gpw + grp) * G + g] = inten * wt;
            t0 = t1, d10 = -d21, s1 = s2, a1 = a2;
        }
        wave_sync();
        {
            const int half = (n_theta + 1) >> 1;
            for (int p = lane; p < 2 * nb * gpw; p += 64) {
                const int h = p & 1, q = p >> 1;
                const int b = (int)(((float)q + 0.5f) * inv_gpw), gq = q - b * gpw;
                const float* cc = sX + (b * gpw + gq) * G + (h ? half : 0);
                const int cnt = h ? n_theta - half : half;
                float sum = 0.f;
                int t = 0;
                for (; t + 5 <= cnt; t += 5) {
                    const float c0 = cc[t], c1 = cc[t + 1], c2 = cc[t + 2], c3 = cc[t + 3], c4 = cc[t + 4];
                    sum = ((((sum + c0) + c1) + c2) + c3) + c4;
                }
                for (; t < cnt; ++t) sum += cc[t];
                const float other = __shfl_xor(sum, 1);
                const int64_t iq = i0 + gq;
                if (h == 0 && iq < n_nu) F[(size_t)(gap0 + b + 1) * fld + iq] = (double)(sum + other);
            }
        }
        wave_sync();
    }
}

// Formal solution with the GAPS OF A RAY SPLIT OVER THE WAVES OF A WORKGROUP (plane-parallel geometry, one angle per lane).
// k_raytrace above is bounded by latency, not throughput: a wave walks all N_d - 1 gaps of its rays one after the other —
// ~5000 dependent-issue instructions — and a grid of a few thousand frequencies offers only 2-3 such waves per SIMD.  But a
// step of the recurrence is AFFINE in the incoming intensity, I' = c I + e with c = 1 - w0, and everything expensive
// (exp(-tau), the weights, the second-order source terms: ~55 of ~60 instructions) is in c and e, which do not depend on I.
// So the NS waves of a workgroup take the same rays (lane <-> (frequency, angle), as above) and one SEGMENT of L = ceil
// (n_gap / NS) gaps each:
//   1  every wave forms (c, e) of its gaps — kept in registers — and composes them, (A, B) <- (c A, c B + e);
//   2  the segment maps meet in LDS; wave s folds the maps of the segments below it: its incoming intensity;
//   3  it replays its gaps, I <- c I + e (one FMA each), and writes I w_theta to LDS; the flux of its own gaps is summed
//      over theta by the wave itself, in the order of k_raytrace (two ascending halves).
// Eight times the waves, each an eighth as long.  Staging (ray table and its reciprocals, log alpha, Planck source, geometric means) is done once
// per workgroup by all its threads; the flux terms reuse that LDS after the barrier of step 2.
// The intensity differs from k_raytrace's by the rounding of the composition (a few ulp; the tolerance is 1e-10).
template <int NS, int LMAX>
__global__ __launch_bounds__(64 * NS) __attribute__((amdgpu_waves_per_eu(NS >= 8 ? 6 : 4, 8))) void k_raytrace_seg(
    int n_depth, int64_t n_nu, int n_theta, int theta_stride, const double* __restrict__ nus, const double* __restrict__ temps,
    const double* __restrict__ ray_dist, const double* __restrict__ wts, const double* __restrict__ alphas,
    int64_t ald, double* __restrict__ F, int64_t fld, double* __restrict__ I_nus, int gpw, int g_recip, unsigned n_wg, unsigned per_xcd,
    FusedTotal ft)
{
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63;
    const int seg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: gap indices and their branches stay scalar
    const int G = n_theta;
    const int grp = lane_div(lane, g_recip), g = lane - grp * G;
    // XCD-aware order: a workgroup reads and writes only gpw (= 3) adjacent columns of every plane row, less than half a 64-byte
    // sector — the workgroups that share a sector must share an L2, or every XCD fetches and writes back its own copy of it
    // (measured: 30 MB fetched, 13 MB written for 10 + 7 MB).  Workgroups b, b + 8, ... run on one XCD: they take one
    // contiguous eighth of the frequencies (the work per frequency is uniform here).  n_wg = ceil(n_nu / gpw) and per_xcd =
    // ceil(n_wg / 8) are launch constants and come from the host: formed here, two 64-bit divisions ran in every wave.  The grid is
    // 8 per_xcd workgroups, so the index fits 32 bits.
    const unsigned wg = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if ((blockIdx.x >> 3) >= per_xcd || wg >= n_wg) return;  // (the whole workgroup: no barrier is left waiting)
    const int64_t i0 = (int64_t)wg * gpw;
    const int64_t i = i0 + grp;
    const bool active = grp < gpw;
    const bool valid = active && i < n_nu;
    const int n_gap = n_depth - 1, col = n_depth;
    const RtSegments lay(NS, LMAX, n_theta, n_depth);
    const int rstride = lay.rstride();         // odd row stride: the angles of a wave read distinct banks
    double* sAB = smem + lay.maps();           // [NS][64][2] segment maps
    double* sRT = smem + lay.ray_table();      // ray_dist TRANSPOSED [n_theta][rstride]: a lane's gaps are consecutive (immediate offsets)
    // (source function, sqrt(alpha)) [gpw][col], a point's pair ONE 16-byte LDS read; the geometric-mean opacity of a gap (:121) is
    // the product of its two ends' square roots
    double2* sP = (double2*)(smem + lay.pairs());
    double* sFx = smem + lay.flux();           // after the barrier of step 2: flux terms [NS][LMAX][gpw][G]

    // staging without a division per item: lane <-> (one of 64 / n_theta gaps, angle) once; then a wave takes one frequency's
    // column (lane <-> depth) — waves 0 .. gpw-1 sqrt(alpha), the next gpw the source function
    {
        const int per = 64 / G;  // gaps per wave and trip
        if (grp < per)
            for (int gp = seg * per + grp; gp < n_gap; gp += NS * per) sRT[g * rstride + gp] = ray_dist[(size_t)gp * theta_stride + g];
    }
    for (int part = seg; part < 2 * gpw; part += NS) {
        const bool source = part >= gpw;
        const int gq = source ? part - gpw : part;
        const int64_t iq = i0 + gq;
        const bool vq = iq < n_nu;
        const int64_t ic = vq ? iq : n_nu - 1;
        if (source) {
            const double nu = nus[ic];
            for (int d = lane; d < n_depth; d += 64) sP[gq * col + d].x = ft.source ? ft.source[(size_t)d * ft.sld + ic] : planck_staged(nu, temps[d]);
            continue;
        }
        for (int d = lane; d < n_depth; d += 64) {
            double a;
            if (ft.cont) {
                a = ft.cont[(size_t)d * ft.cld + ic];
                if (ft.planes) {
                    double line = ft.planes[(size_t)d * ft.pld + ic];
                    for (int sp = 1; sp < ft.n_planes; ++sp) line = add_rn(line, ft.planes[((size_t)sp * n_depth + d) * ft.pld + ic]);
                    a = add_rn(a, line);
                    if (vq && ft.line_out) ft.line_out[(size_t)d * ft.out_ld + iq] = line;
                }
                for (int x = 0; x < ft.n_extra; ++x) a = add_rn(a, ft.extra[x][(size_t)d * ft.eld + ic]);
                if (vq && ft.total_out) ft.total_out[(size_t)d * ft.out_ld + iq] = a;
            } else {
                a = alphas[(size_t)d * ald + ic];
            }
            sP[gq * col + d].y = sqrt(a);
        }
    }
    __syncthreads();

    // step 1: the coefficients of this wave's gaps [g_lo, g_lo + count).  The segments are aligned to the END of the ray — the first
    // wave takes the short one — and a wave's gaps to the end of its LMAX register slots (slot j <-> gap g_lo + j - j0): the final
    // gap, the one step with a formula of its own (:253-266), is then always slot LMAX - 1 of the last wave, a static place
    const int L = lay.segment();
    const int g_end = n_gap - (NS - 1 - seg) * L;
    const int g_lo = max(0, g_end - L);
    const int count = max(0, g_end - g_lo);
    const int j0 = LMAX - count;
    const int gi = (active ? grp : 0) * col;  // idle lanes shadow group 0 and never store
    const int th = min(g, n_theta - 1);
    const double wt = wts[th];
    double c[LMAX], e[LMAX];
    double A = 1.0, B = 0.0;
    // the unrolled pass carries no per-lane exception handling: a lane with anything unusual (a transparent gap, a denominator
    // outside the normal range) only raises the wave's flag, and the wave then walks its segment once more, the flagged lanes'
    // steps in the reference's own form
    unsigned long long redo = 0;
    const int gc = count > 0 ? g_lo : 0;
    const RtConst kc = rt_const_resident();  // the step's literals, in scalar registers from here on (sdx_math.h)
    // (A straight-line copy of this pass and of the replay for the waves whose segment fills all LMAX slots — no `j >= j0` test per
    // slot — was built and measured: 34.7 us against 35.0 at S-c2, inside the spread of either, for a third more code; the compiler
    // also sank every slot's tail behind the last one, 48 spilled VGPRs, until each slot's (c, e) was pinned.  Removed.)
    {
        const double2* pP = sP + gi + gc - j0;
        const double* pR = sRT + th * rstride + gc - j0;
        const double2 q0 = pP[j0], q1 = pP[j0 + 1];
        double a1 = q1.y, s1 = q1.x;
        double d10 = q0.x - s1;
        double t0 = mul_rn(q0.y * a1, pR[j0]);
#pragma unroll
        for (int j = 0; j < LMAX; ++j) {
            c[j] = 1.0, e[j] = 0.0;
            if (j >= j0) {
                if (j < LMAX - 1 || seg < NS - 1) {  // :208-249
                    const double2 q2 = pP[j + 2];
                    const double s2 = q2.x, a2 = q2.y;
                    const double t1 = mul_rn(a1 * a2, pR[j + 1]);
                    const double d21 = s2 - s1;
                    redo |= rt_coef_fast<false>(t0, t1, d10, d21, s1, c[j], e[j], kc);
                    t0 = t1, d10 = -d21, s1 = s2, a1 = a2;
                } else {  // the final gap (:253-266)
                    redo |= rt_coef_fast<true>(t0, 0.0, d10, 0.0, s1, c[j], e[j], kc);
                }
                A *= c[j];
                B = fma(c[j], B, e[j]);
            }
        }
    }
    if (redo) {  // rare: a rolled loop, the coefficients find their registers through a (scalar) switch
        A = 1.0, B = 0.0;
        for (int j = j0; j < LMAX; ++j) {
            const int gap = gc + j - j0;
            const double s0 = sP[gi + gap].x, s1 = sP[gi + gap + 1].x;
            const double t0 = mul_rn(sP[gi + gap].y * sP[gi + gap + 1].y, sRT[th * rstride + gap]);
            double cj = 1.0, ej = 0.0;  // (the lanes that did not raise the flag keep the fast pass's pair)
#pragma unroll
            for (int k = 0; k < LMAX; ++k)
                if (k == j) cj = c[k], ej = e[k];
            if (gap < n_gap - 1) {
                const double t1 = mul_rn(sP[gi + gap + 1].y * sP[gi + gap + 2].y, sRT[th * rstride + gap + 1]);
                if (rt_coef_is_unusual<false>(t0, t1)) rt_coef_reference<false>(t0, t1, s0 - s1, sP[gi + gap + 2].x - s1, s1, cj, ej);
            } else {
                if (rt_coef_is_unusual<true>(t0, 0.0)) rt_coef_reference<true>(t0, 0.0, s0 - s1, 0.0, s1, cj, ej);
            }
            A *= cj;
            B = fma(cj, B, ej);
#pragma unroll
            for (int k = 0; k < LMAX; ++k)
                if (k == j) c[k] = cj, e[k] = ej;
        }
    }
    sAB[(seg * 64 + lane) * 2] = A;
    sAB[(seg * 64 + lane) * 2 + 1] = B;
    __syncthreads();
    // step 2: the intensity entering this segment (0 at the innermost point, np.zeros :134)
    double inten = 0.0;
    for (int k = 0; k < seg; ++k) inten = fma(sAB[(k * 64 + lane) * 2], inten, sAB[(k * 64 + lane) * 2 + 1]);
    if (seg == 0) {
        if (valid && I_nus) I_nus[(size_t)i * theta_stride + th] = 0.0;
        if (valid && g == 0 && F) F[i] = 0.0;
    }
    // step 3: replay, flux terms to LDS (the staging arrays are dead since the barrier)
    double* fx = sFx + (size_t)seg * LMAX * gpw * G + (active ? grp * G + g : 0);
    // (one pointer stepped per gap: left as an index expression, the 64-bit address of the optional intensity output is
    // formed for every gap whether or not it is requested — ten instructions next to one FMA)
    double* ip = valid && I_nus ? I_nus + ((size_t)(g_lo + 1) * n_nu + i) * theta_stride + th : nullptr;
    const size_t istep = (size_t)n_nu * theta_stride;
#pragma unroll
    for (int j = 0; j < LMAX; ++j) {
        if (j >= j0) {
            inten = fma(c[j], inten, e[j]);
            if (ip) *ip = inten, ip += istep;
            if (active) fx[(j - j0) * gpw * G] = inten * wt;
        }
    }
    fx = sFx + (size_t)seg * LMAX * gpw * G;
    wave_sync();
    if (F) {
        const int half = (n_theta + 1) >> 1;
        for (int p = lane; p < 2 * count * gpw; p += 64) {
            const int h = p & 1, q = p >> 1;  // q = b * gpw + gq
            const int b = (int)(((float)q + 0.5f) * (1.0f / (float)gpw)), gq = q - b * gpw;  // q < 64 LMAX: exact
            const double* cc = fx + q * G + (h ? half : 0);
            const int cnt = h ? n_theta - half : half;
            double sum = 0.0;
            for (int t = 0; t < cnt; ++t) sum = add_rn(sum, cc[t]);
            const double other = __shfl_xor(sum, 1);
            const int64_t iq = i0 + gq;
            if (h == 0 && iq < n_nu) F[(size_t)(g_lo + b + 1) * fld + iq] = add_rn(sum, other);
        }
    }
}

// k_raytrace_seg in the ONE SHAPE the fused synthesis step launches it in: a fused total (continuum + N_PLANES partial line planes,
// N_PLANES = 0 for a zero-line run and for the continuum-only second launch), the Planck source, flux only.  The same algorithm and
// the same floating-point operations in the same order — segment alignment, rt_coef_fast / rt_coef_reference on resident constants,
// the composition, the fold, the two ascending halves of the flux, total = cont + (p0 + p1 (+ p2)) — so the same bits; what differs
// is the fixed cost a wave pays around its LMAX gaps:
//   prologue  every launch constant the general kernel forms per wave comes from the host (SegStepGeom); no address of an output the
//             shape lacks; the Planck literals live only in the waves that stage;
//   staging   items are (depth, column) with the column fastest, dense over the lanes: a wave's loads and its total_out stores cover
//             whole runs of a row (the general kernel gives a column to a wave: three waves touch the same sectors of every row), all
//             plane loads of a point are in flight before the first add, the Planck value — no load of a plane behind it — is formed
//             under their latency, and a point's (source, sqrt(alpha)) pair is ONE 16-byte LDS write.  The ray table goes to the waves
//             in descending order, so that the waves without columns take its extra trip;
//   replay    no test for the optional intensity output;
//   flux      (gap, frequency) of a lane from the host's reciprocal of gpw; at 20 angles (geo.fx_pairs) a lane reads its half of the
//             angles as five 16-byte words, all in flight before the first add; the two lanes of a pair exchange their sums inside
//             the quad; F's row stride is 32 bits.  The same adds in the same order.  (Unpredicated replay stores, the segment maps
//             read ahead of the fold and the ray table loaded ahead of the staging were built and measured: nothing, or 0.3 us of 30
//             each — profiles/EXPERIMENTS.md.)
struct SegStepGeom {
    int gpw, g_recip;         // frequencies per workgroup 64 / n_theta; lane_recip(n_theta)
    int per;                  // 64 / n_theta: gaps of the ray table per wave and trip
    int L;                    // RtSegments::segment()
    int rstride;              // RtSegments::rstride()
    int sp_off;               // doubles from the ray table to the (source, sqrt(alpha)) pairs: RtSegments::pairs_from_table()
    unsigned gpw_magic;       // small_div_magic(gpw)
    unsigned n_wg, per_xcd;   // as k_raytrace_seg
    int fx_pairs;             // kStepFluxPairs where a half of the flux sum is that many aligned 16-byte reads and a wave's items fit
                              // its lanes (seg_step_flux_pairs); 0: the general form
    unsigned fld;             // the row stride of F (the host launches this kernel only where it fits 32 bits)
};
// The flux sum's 128-bit form: n_theta = 20 (two halves of ten angles: five 16-byte reads each).  Every run of a half then starts at
// an even double — n_theta, the half and with them a gap's and a wave's share of the terms are even, and the flux terms start where
// the ray table does (RtSegments::flux(): even) — and the 2 LMAX gpw (gap, frequency, half) items of a wave are at most its 64 lanes.
constexpr int kStepFluxPairs = 5;
inline int seg_step_flux_pairs(const RtSegments& s)
{
    const int half = (s.n_theta + 1) >> 1;
    return s.n_theta % 4 == 0 && half == 2 * kStepFluxPairs && s.flux() % 2 == 0 && 2 * s.LMAX * s.gpw() <= 64 ? kStepFluxPairs : 0;
}
// lanes 2k and 2k + 1 exchange v (what __shfl_xor(v, 1) moves, as two DPP moves inside the quad instead of a trip through LDS)
__device__ __forceinline__ double swap_lane_pairs(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0xB1, 0xF, 0xF, true);  // quad_perm: [1, 0, 3, 2]
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0xB1, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
template <int NS, int LMAX, int N_PLANES, bool KEEP_TOTAL>
__global__ __launch_bounds__(64 * NS) __attribute__((amdgpu_waves_per_eu(NS >= 8 ? 6 : 4, 8))) void k_raytrace_seg_step(
    int n_depth, int64_t n_nu, int n_theta, int theta_stride, const double* __restrict__ nus, const double* __restrict__ temps,
    const double* __restrict__ ray_dist, const double* __restrict__ wts, const double* __restrict__ cont, int64_t cld,
    const double* __restrict__ planes, int64_t pld, double* __restrict__ total_out, int64_t out_ld, double* __restrict__ F, SegStepGeom geo)
{
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63;
    const int seg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = n_theta, gpw = geo.gpw;
    const int grp = lane_div(lane, geo.g_recip), g = lane - grp * G;
    const unsigned wg = (blockIdx.x & 7) * geo.per_xcd + (blockIdx.x >> 3);  // XCD-aware order, as k_raytrace_seg
    if ((blockIdx.x >> 3) >= geo.per_xcd || wg >= geo.n_wg) return;
    const int64_t i0 = (int64_t)wg * gpw;
    const bool active = grp < gpw;
    const int n_gap = n_depth - 1, col = n_depth;
    const int rstride = geo.rstride;
    double* sAB = smem;                        // [NS][64][2] segment maps (the layout is RtSegments, its run-time values in geo)
    double* sRT = smem + RtSegments(NS, LMAX, n_theta, n_depth).ray_table();  // ray_dist transposed [n_theta][rstride]
    double2* sP = (double2*)(sRT + geo.sp_off);  // (source function, sqrt(alpha)) [gpw][col]
    double* sFx = sRT;                         // after the barrier of step 2: flux terms [NS][LMAX][gpw][G]

    if (grp < geo.per)
        for (int gp = (NS - 1 - seg) * geo.per + grp; gp < n_gap; gp += NS * geo.per) sRT[g * rstride + gp] = ray_dist[gp * theta_stride + g];
    const int n_items = n_depth * gpw;
    if (seg * 64 < n_items) {  // (wave-uniform: a wave without items forms no Planck constant)
        for (int k = threadIdx.x; k < n_items; k += 64 * NS) {
            const int d = small_div(k, geo.gpw_magic), gq = k - d * gpw;
            const int64_t iq = i0 + gq;
            const bool vq = iq < n_nu;
            const int64_t ic = vq ? iq : n_nu - 1;
            const double c0 = cont[(size_t)d * cld + ic];
            double pl[N_PLANES > 0 ? N_PLANES : 1];
#pragma unroll
            for (int sp = 0; sp < N_PLANES; ++sp) pl[sp] = planes[((size_t)sp * n_depth + d) * pld + ic];
            const double src = planck_staged(nus[ic], temps[d]);
            double a = c0;
            if (N_PLANES > 0) {
                double line = pl[0];
#pragma unroll
                for (int sp = 1; sp < N_PLANES; ++sp) line = add_rn(line, pl[sp]);
                a = add_rn(a, line);
            }
            if (KEEP_TOTAL && vq) total_out[(size_t)d * out_ld + iq] = a;
            sP[gq * col + d] = double2{src, sqrt(a)};
        }
    }
    __syncthreads();

    // step 1, as k_raytrace_seg: segments aligned to the end of the ray, a wave's gaps to the end of its LMAX register slots
    const int L = geo.L;
    const int g_end = n_gap - (NS - 1 - seg) * L;
    const int g_lo = max(0, g_end - L);
    const int count = max(0, g_end - g_lo);
    const int j0 = LMAX - count;
    const int gi = (active ? grp : 0) * col;  // idle lanes shadow group 0 and never store
    const int th = min(g, n_theta - 1);
    const double wt = wts[th];
    double c[LMAX], e[LMAX];
    double A = 1.0, B = 0.0;
    unsigned long long redo = 0;
    const int gc = count > 0 ? g_lo : 0;
    const RtConst kc = rt_const_resident();
    {
        const double2* pP = sP + gi + gc - j0;
        const double* pR = sRT + th * rstride + gc - j0;
        const double2 q0 = pP[j0], q1 = pP[j0 + 1];
        double a1 = q1.y, s1 = q1.x;
        double d10 = q0.x - s1;
        double t0 = mul_rn(q0.y * a1, pR[j0]);
#pragma unroll
        for (int j = 0; j < LMAX; ++j) {
            c[j] = 1.0, e[j] = 0.0;
            if (j >= j0) {
                if (j < LMAX - 1 || seg < NS - 1) {  // :208-249
                    const double2 q2 = pP[j + 2];
                    const double s2 = q2.x, a2 = q2.y;
                    const double t1 = mul_rn(a1 * a2, pR[j + 1]);
                    const double d21 = s2 - s1;
                    redo |= rt_coef_fast<false>(t0, t1, d10, d21, s1, c[j], e[j], kc);
                    t0 = t1, d10 = -d21, s1 = s2, a1 = a2;
                } else {  // the final gap (:253-266)
                    redo |= rt_coef_fast<true>(t0, 0.0, d10, 0.0, s1, c[j], e[j], kc);
                }
                A *= c[j];
                B = fma(c[j], B, e[j]);
            }
        }
    }
    if (redo) {  // rare: the segment once more, the flagged lanes' steps in the reference's own form
        A = 1.0, B = 0.0;
        for (int j = j0; j < LMAX; ++j) {
            const int gap = gc + j - j0;
            const double s0 = sP[gi + gap].x, s1 = sP[gi + gap + 1].x;
            const double t0 = mul_rn(sP[gi + gap].y * sP[gi + gap + 1].y, sRT[th * rstride + gap]);
            double cj = 1.0, ej = 0.0;  // (the lanes that did not raise the flag keep the fast pass's pair)
#pragma unroll
            for (int k = 0; k < LMAX; ++k)
                if (k == j) cj = c[k], ej = e[k];
            if (gap < n_gap - 1) {
                const double t1 = mul_rn(sP[gi + gap + 1].y * sP[gi + gap + 2].y, sRT[th * rstride + gap + 1]);
                if (rt_coef_is_unusual<false>(t0, t1)) rt_coef_reference<false>(t0, t1, s0 - s1, sP[gi + gap + 2].x - s1, s1, cj, ej);
            } else {
                if (rt_coef_is_unusual<true>(t0, 0.0)) rt_coef_reference<true>(t0, 0.0, s0 - s1, 0.0, s1, cj, ej);
            }
            A *= cj;
            B = fma(cj, B, ej);
#pragma unroll
            for (int k = 0; k < LMAX; ++k)
                if (k == j) c[k] = cj, e[k] = ej;
        }
    }
    sAB[(seg * 64 + lane) * 2] = A;
    sAB[(seg * 64 + lane) * 2 + 1] = B;
    __syncthreads();
    // step 2: the intensity entering this segment
    double inten = 0.0;
    for (int k = 0; k < seg; ++k) inten = fma(sAB[(k * 64 + lane) * 2], inten, sAB[(k * 64 + lane) * 2 + 1]);
    if (seg == 0 && active && g == 0 && i0 + grp < n_nu) F[i0 + grp] = 0.0;
    // step 3: replay, flux terms to LDS
    double* fx = sFx + seg * LMAX * gpw * G + (active ? grp * G + g : 0);
#pragma unroll
    for (int j = 0; j < LMAX; ++j) {
        if (j >= j0) {
            inten = fma(c[j], inten, e[j]);
            if (active) fx[(j - j0) * gpw * G] = inten * wt;
        }
    }
    fx = sFx + seg * LMAX * gpw * G;
    wave_sync();
    // the flux: lane p sums one half of the angles of (gap b, frequency gq), ascending; the halves meet in one add
    if (geo.fx_pairs == kStepFluxPairs) {
        // the 128-bit form: a half is kStepFluxPairs 16-byte reads, all in flight before the first add — the same adds —, and a wave's
        // items fit its lanes.  4 kStepFluxPairs angles, hence kW frequencies per workgroup, are constants here: lane p's run starts
        // (q n_theta + h n_theta / 2 =) p halves into the wave's terms
        constexpr int kW = 64 / (4 * kStepFluxPairs);
        if (lane < 2 * count * kW) {
            const int h = lane & 1, q = lane >> 1;  // q = b * kW + gq
            const int b = q / kW, gq = q - b * kW;
            const double2* cc = (const double2*)(fx + lane * (2 * kStepFluxPairs));
            double2 v[kStepFluxPairs];
#pragma unroll
            for (int t = 0; t < kStepFluxPairs; ++t) v[t] = cc[t];
            double sum = 0.0;
#pragma unroll
            for (int t = 0; t < kStepFluxPairs; ++t) sum = add_rn(add_rn(sum, v[t].x), v[t].y);
            const double other = swap_lane_pairs(sum);
            const int64_t iq = i0 + gq;
            if (h == 0 && iq < n_nu) F[(size_t)(unsigned)(g_lo + b + 1) * geo.fld + iq] = add_rn(sum, other);
        }
        return;
    }
    const int half = (n_theta + 1) >> 1;
    for (int p = lane; p < 2 * count * gpw; p += 64) {
        const int h = p & 1, q = p >> 1;  // q = b * gpw + gq
        const int b = small_div(q, geo.gpw_magic), gq = q - b * gpw;
        const double* cc = fx + q * G + h * half;
        const int cnt = half - (h & n_theta & 1);  // (the second half of an odd count is one angle shorter)
        double sum = 0.0;
#pragma unroll 1
        for (int t = 0; t < cnt; ++t) sum = add_rn(sum, cc[t]);
        const double other = swap_lane_pairs(sum);
        const int64_t iq = i0 + gq;
        if (h == 0 && iq < n_nu) F[(size_t)(unsigned)(g_lo + b + 1) * geo.fld + iq] = add_rn(sum, other);
    }
}

// ------------------------------------------------------------------------------------------------
// The formal solution with the CONTINUUM FLUX beside the total one (sdx_synthesis_options.F_nu_continuum): F_nu of the continuum
// plane alone — what radiation_field_solvers/base.py:271-346 gives for the total_alphas of a run with the lines disabled (the
// reference's `alpha_line_at_nu = 0` entry adds nothing, opacities/base.py:24-28) — from the same staging.  Requires a fused total
// (ft.cont): the continuum column is read there anyway.
//
// k_raytrace_cont: the layout of k_raytrace with sqrt(alpha_cont) staged per depth point beside the (S, sqrt(alpha)) pair, and
// per lane TWO independent recurrences — total and continuum — on the same ray lengths, the same source values and the same rt_coef
// arithmetic (the same operations as k_raytrace on a zero-line total, so the continuum flux is that run's F_nu bit for bit).  The
// k_raytrace chain is latency-bound (one wave walks all N_d - 1 dependent gaps); the second chain gives the scheduler independent work
// to interleave.  Both flux sums use k_raytrace's order (two ascending halves over theta); the spherical inward sweep runs for both.
__global__ __launch_bounds__(kRtBlock) void k_raytrace_cont(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                          const double* __restrict__ nus, const double* __restrict__ temps,
                                                          const double* __restrict__ ray_dist, const double* __restrict__ wts,
                                                          double* __restrict__ F, int64_t fld, double* __restrict__ Fc, int64_t fcld,
                                                          double* __restrict__ I_nus, int inward, int gpw, FusedTotal ft)
{
    constexpr int P = 1, kBatch = kRtBatch;  // P: angles per lane (why the one-trip loops over k stay: the note above k_raytrace_basic)
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane / G, g = lane - grp * G;
    const int64_t i0 = ((int64_t)blockIdx.x * (kRtBlock / 64) + wave) * gpw;
    const int64_t i = i0 + grp;
    const bool active = grp < gpw;
    const bool valid = active && i < n_nu;
    const int64_t ic = i < n_nu ? i : n_nu - 1;
    const int n_gap = n_depth - 1;
    const int col = n_depth;
    // must match RtContColumns (sdx_rt_layout.h), which the host sizes the launch by (taken from the struct the instructions change)
    double* wbase = smem + (size_t)wave * ((3 * gpw * col + 2 * kBatch * gpw * G + 1) & ~1);  // (even: 16-byte aligned pairs)
    double2* sP = (double2*)wbase;            // (source function, sqrt(alpha total)) [gpw][col]
    double* sC = wbase + 2 * gpw * col;       // sqrt(alpha continuum)             [gpw][col]
    double* sX = sC + gpw * col;              // flux terms, total                 [kBatch][gpw][G]
    double* sXc = sX + kBatch * gpw * G;      // flux terms, continuum             [kBatch][gpw][G]
    const double nu = nus[ic];

    if (active) {
        for (int d = g; d < n_depth; d += G) {
            const double ac = ft.cont[(size_t)d * ft.cld + ic];
            double a = ac;
            if (ft.planes) {
                double line = ft.planes[(size_t)d * ft.pld + ic];
                for (int sp = 1; sp < ft.n_planes; ++sp) line = add_rn(line, ft.planes[((size_t)sp * n_depth + d) * ft.pld + ic]);
                a = add_rn(a, line);
                if (valid && ft.line_out) ft.line_out[(size_t)d * ft.out_ld + i] = line;
            }
            for (int x = 0; x < ft.n_extra; ++x) a = add_rn(a, ft.extra[x][(size_t)d * ft.eld + ic]);
            if (valid && ft.total_out) ft.total_out[(size_t)d * ft.out_ld + i] = a;
            sP[grp * col + d] = double2{ft.source ? ft.source[(size_t)d * ft.sld + ic] : planck_staged(nu, temps[d]), sqrt(a)};
            sC[grp * col + d] = sqrt(ac);
        }
    }
    wave_sync();
    const RtConst kc = rt_const_literals();  // (literals, as in k_raytrace)

    const int gi = (active ? grp : 0) * col;
    double inten[P], intc[P], wt[P];
    int th[P];
    bool on[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        th[k] = min(g, n_theta - 1);
        on[k] = g < n_theta;
        inten[k] = 0.0, intc[k] = 0.0;
        wt[k] = on[k] ? wts[th[k]] : 0.0;
    }
    if (inward) {  // the surface-to-centre sweep of k_raytrace, for both chains
        for (int gap = n_gap - 1; gap >= 0; --gap) {
            const int gm = gap > 0 ? gap - 1 : n_gap - 1;
            const int dm = gap > 0 ? gap - 1 : n_depth - 1;
            const double2 q0 = sP[gi + gap + 1], q1 = sP[gi + gap], q2 = sP[gi + dm];
            const double s0 = q0.x, s1 = q1.x, s2 = q2.x;
            const double mg = q1.y * q0.y, mm = sP[gi + gm].y * sP[gi + gm + 1].y;
            const double mgc = sC[gi + gap] * sC[gi + gap + 1], mmc = sC[gi + gm] * sC[gi + gm + 1];
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const double rg = ray_dist[(size_t)gap * theta_stride + th[k]], rm = ray_dist[(size_t)gm * theta_stride + th[k]];
                const double tg = mul_rn(mg, rg), tm = mul_rn(mm, rm);
                const double tgc = mul_rn(mgc, rg), tmc = mul_rn(mmc, rm);
                double c, e, cc, ec;
                rt_coef<false>(tg, tm, s0 - s1, s2 - s1, s1, c, e, kc);
                rt_coef<false>(tgc, tmc, s0 - s1, s2 - s1, s1, cc, ec, kc);
                inten[k] = tm == 0.0 ? inten[k] : fma(c, inten[k], e);
                intc[k] = tmc == 0.0 ? intc[k] : fma(cc, intc[k], ec);
            }
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if (valid && I_nus && on[k]) I_nus[(size_t)i * theta_stride + th[k]] = inten[k];
            if (active) sX[grp * G + g] = inten[k] * wt[k], sXc[grp * G + g] = intc[k] * wt[k];
        }
        wave_sync();
        if (lane < gpw && i0 + lane < n_nu) {
            double sum = 0.0, sumc = 0.0;
            for (int t = 0; t < n_theta; ++t) sum = add_rn(sum, sX[lane * G + t]), sumc = add_rn(sumc, sXc[lane * G + t]);
            F[i0 + lane] = sum;
            Fc[i0 + lane] = sumc;
        }
        wave_sync();
    } else {
#pragma unroll
        for (int k = 0; k < P; ++k)
            if (valid && I_nus && on[k]) I_nus[(size_t)i * theta_stride + th[k]] = 0.0;
        if (valid && g == 0) F[i] = 0.0, Fc[i] = 0.0;
    }
    double tau0[P], tauc0[P], rd_next[P];
    const double* rdp[P];
    const double2 p0 = sP[gi], p1 = sP[gi + 1];
    double a1 = p1.y, ac1 = sC[gi + 1];
    {
        const double mean0 = p0.y * a1, meanc0 = sC[gi] * ac1;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            rdp[k] = ray_dist + th[k];
            const double r0 = *rdp[k];
            tau0[k] = mul_rn(mean0, r0);
            tauc0[k] = mul_rn(meanc0, r0);
            rdp[k] += n_gap > 1 ? theta_stride : 0;
            rd_next[k] = *rdp[k];
        }
    }
    double s1 = p1.x, d10 = p0.x - s1;
    const float inv_gpw = 1.0f / (float)gpw;

    for (int gap0 = 0; gap0 < n_gap; gap0 += kBatch) {
        const int nb = min(kBatch, n_gap - gap0);
        for (int b = 0; b < nb; ++b) {
            const int gap = gap0 + b;
            if (gap < n_gap - 1) {
                const double2 p2 = sP[gi + gap + 2];
                const double s2 = p2.x, a2 = p2.y, ac2 = sC[gi + gap + 2];
                const double mean1 = a1 * a2, meanc1 = ac1 * ac2, d21 = s2 - s1;
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    const double rd = rd_next[k];
                    const double t1 = mul_rn(mean1, rd), tc1 = mul_rn(meanc1, rd);
                    rdp[k] += gap + 2 < n_gap ? theta_stride : 0;
                    rd_next[k] = *rdp[k];
                    double c, e, cc, ec;
                    rt_coef<false>(tau0[k], t1, d10, d21, s1, c, e, kc);
                    rt_coef<false>(tauc0[k], tc1, d10, d21, s1, cc, ec, kc);
                    const double inew = fma(c, inten[k], e), icnew = fma(cc, intc[k], ec);
                    inten[k] = inew, intc[k] = icnew;
                    tau0[k] = t1, tauc0[k] = tc1;
                    if (valid && I_nus && on[k]) I_nus[((size_t)(gap + 1) * n_nu + i) * theta_stride + th[k]] = inew;
                    if (active) sX[(b * gpw + grp) * G + g] = inew * wt[k], sXc[(b * gpw + grp) * G + g] = icnew * wt[k];
                }
                d10 = -d21, s1 = s2, a1 = a2, ac1 = ac2;
            } else {
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    double c, e, cc, ec;
                    rt_coef<true>(tau0[k], 0.0, d10, 0.0, s1, c, e, kc);
                    rt_coef<true>(tauc0[k], 0.0, d10, 0.0, s1, cc, ec, kc);
                    const double inew = fma(c, inten[k], e), icnew = fma(cc, intc[k], ec);
                    inten[k] = inew, intc[k] = icnew;
                    if (valid && I_nus && on[k]) I_nus[((size_t)(gap + 1) * n_nu + i) * theta_stride + th[k]] = inew;
                    if (active) sX[(b * gpw + grp) * G + g] = inew * wt[k], sXc[(b * gpw + grp) * G + g] = icnew * wt[k];
                }
            }
        }
        wave_sync();
        {
            const int half = (n_theta + 1) >> 1;
            for (int p = lane; p < 2 * nb * gpw; p += 64) {
                const int h = p & 1, q = p >> 1;
                const int b = (int)(((float)q + 0.5f) * inv_gpw), gq = q - b * gpw;
                const int off = (b * gpw + gq) * G + (h ? half : 0);
                const double* c = sX + off;
                const double* cc = sXc + off;
                const int cnt = h ? n_theta - half : half;
                double sum = 0.0, sumc = 0.0;
                int t = 0;
                for (; t + 5 <= cnt; t += 5) {
                    const double c0 = c[t], c1 = c[t + 1], c2 = c[t + 2], c3 = c[t + 3], c4 = c[t + 4];
                    const double e0 = cc[t], e1 = cc[t + 1], e2 = cc[t + 2], e3 = cc[t + 3], e4 = cc[t + 4];
                    sum = add_rn(add_rn(add_rn(add_rn(add_rn(sum, c0), c1), c2), c3), c4);
                    sumc = add_rn(add_rn(add_rn(add_rn(add_rn(sumc, e0), e1), e2), e3), e4);
                }
                for (; t < cnt; ++t) sum = add_rn(sum, c[t]), sumc = add_rn(sumc, cc[t]);
                const double other = __shfl_xor(sum, 1), otherc = __shfl_xor(sumc, 1);
                const int64_t iq = i0 + gq;
                if (h == 0 && iq < n_nu) {
                    F[(size_t)(gap0 + b + 1) * fld + iq] = add_rn(sum, other);
                    Fc[(size_t)(gap0 + b + 1) * fcld + iq] = add_rn(sumc, otherc);
                }
            }
        }
        wave_sync();
    }
}

// ------------------------------------------------------------------------------------------------
// Flux contribution function: WHERE the emergent flux is formed.  The formal solution is, per ray and gap, the affine map
// I[g+1] = c[g] I[g] + e[g] (rt_coef; radiation_field_solvers/base.py:200-266) and every ray starts at I[0] = 0 (:134), so the emergent
// intensity is exactly sum_g T[g+1] e[g], T[k] = prod_{j >= k} c[j] the transmission from row k to the surface (T[N_d - 1] = 1).  Summed
// over the angles with the flux weights (:324-338), the terms are what the layer below row k adds to F_nu[N_d - 1]:
//     C[0] = 0,   C[k] = sum_theta w_theta (T[k] e[k-1]),   sum_k C[k] = F_nu[N_d - 1] up to rounding.
// Nothing is modelled anew: (c, e) come from the device functions k_raytrace calls — rt_coef<false> for the inner gaps, rt_coef<true> for the
// last one, the tau == 0 -> (1, 0) rule and the rare-lane fallback included — on the same tau = (sqrt(alpha[g]) sqrt(alpha[g+1])) ray_dist.
//
// The layout of k_raytrace: lane <-> (frequency, angle), a group of G lanes per frequency, (S, sqrt(alpha)) staged per wave in LDS as one
// 16-byte pair per point, from a FINISHED total_alphas plane.  Each lane walks its ray from the surface INWARDS — the rolling state of
// k_raytrace mirrored: the optical depth of the gap and of the one above it, the source at the gap's upper end and the two differences, one
// 16-byte LDS read per step for the point below — carrying only the running product T: the (c, e) of different gaps do not depend on each
// other, so this is not the 55-step dependent chain of the forward recurrence.  T e w_theta goes to the wave's LDS; every kBatch gaps
// the wave sums each (gap, frequency) over theta in k_raytrace's order (two ascending halves, the lower added to the upper) and writes row
// gap + 1 of C.  T underflows to 0 in deep layers: C is 0 there, no special case.  Plane-parallel only (the inward sweep of spherical
// geometry makes I[0] != 0), all angles in one launch.
__global__ __launch_bounds__(kRtBlock) void k_contribution(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                         const double* __restrict__ nus, const double* __restrict__ temps,
                                                         const double* __restrict__ ray_dist, const double* __restrict__ wts,
                                                         const double* __restrict__ alphas, int64_t ald, const double* __restrict__ source,
                                                         int64_t sld, double* __restrict__ C, int64_t cld, int gpw)
{
    constexpr int P = 1, kBatch = kRtBatch;  // P: angles per lane (why the one-trip loops over k stay: the note above k_raytrace_basic)
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane / G, g = lane - grp * G;
    const int64_t i0 = ((int64_t)blockIdx.x * (kRtBlock / 64) + wave) * gpw;  // first frequency of this wave
    const int64_t i = i0 + grp;
    const bool active = grp < gpw;
    const bool valid = active && i < n_nu;
    const int64_t ic = i < n_nu ? i : n_nu - 1;
    const int n_gap = n_depth - 1;
    const int col = n_depth;  // LDS row stride per group
    const RtColumns lay(G, n_depth, gpw);
    double* wbase = smem + (size_t)wave * lay.wave_doubles();
    double2* sP = (double2*)(wbase + lay.pairs());  // (source function, sqrt(alpha)) [gpw][col]
    double* sX = wbase + lay.flux();                // flux terms T e w_theta [kBatch][gpw][G]
    const double nu = nus[ic];

    if (active) {
        for (int d = g; d < n_depth; d += G)
            sP[grp * col + d] = double2{source ? source[(size_t)d * sld + ic] : planck_staged(nu, temps[d]), sqrt(alphas[(size_t)d * ald + ic])};
    }
    if (valid && g == 0) C[i] = 0.0;  // nothing lies below row 0
    wave_sync();
    const RtConst kc = rt_const_literals();  // (literals, as in k_raytrace: the gap loop is rolled)

    const int gi = (active ? grp : 0) * col;  // idle lanes shadow group 0 and never store
    double wt[P], trans[P], tau0[P], tau1[P], rd_next[P];
    const double* rdp[P];
    int th[P];
    // rolling state, for the gap being visited: its optical depth tau0 and that of the gap above tau1 per angle; the source at its upper
    // end s1, at its lower end s0, the differences d10 = S[gap] - S[gap+1] and d21 = S[gap+2] - S[gap+1]; sqrt(alpha) at its lower end
    const double2 pt = sP[gi + n_gap], pb = sP[gi + n_gap - 1];
    double s1 = pt.x, s0 = pb.x, a0 = pb.y;
    double d10 = s0 - s1, d21 = 0.0;
    {
        const double mean = a0 * pt.y;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            th[k] = min(g, n_theta - 1);
            wt[k] = g < n_theta ? wts[th[k]] : 0.0;
            trans[k] = 1.0;  // T[N_d - 1]
            rdp[k] = ray_dist + (size_t)(n_gap - 1) * theta_stride + th[k];
            tau0[k] = mul_rn(mean, *rdp[k]);
            tau1[k] = 0.0;
            rdp[k] -= n_gap > 1 ? theta_stride : 0;
            rd_next[k] = *rdp[k];  // gap n_gap - 2
        }
    }
    const float inv_gpw = 1.0f / (float)gpw;

    for (int gtop = n_gap - 1; gtop >= 0; gtop -= kBatch) {
        const int nb = min(kBatch, gtop + 1);
        for (int b = 0; b < nb; ++b) {
            const int gap = gtop - b;
            const double2 pm = sP[gi + max(gap - 1, 0)];  // the point below this gap: what the NEXT step needs, one 16-byte read
            const double mean_next = pm.y * a0;
#pragma unroll
            for (int k = 0; k < P; ++k) {
                double c, e;
                if (gap == n_gap - 1) rt_coef<true>(tau0[k], 0.0, d10, 0.0, s1, c, e, kc);  // the final gap (:253-266), visited first
                else rt_coef<false>(tau0[k], tau1[k], d10, d21, s1, c, e, kc);               // :208-249
                if (active) sX[(b * gpw + grp) * G + g] = (trans[k] * e) * wt[k];
                trans[k] *= c;  // T[gap]
                tau1[k] = tau0[k];
                tau0[k] = mul_rn(mean_next, rd_next[k]);
                rdp[k] -= gap >= 2 ? theta_stride : 0;
                rd_next[k] = *rdp[k];  // gap - 2, for the next trip
            }
            d21 = -d10, s1 = s0, s0 = pm.x, a0 = pm.y;
            d10 = s0 - s1;
        }
        wave_sync();
        {
            // the nb rows of this batch: lanes <-> (gap, frequency, half of the angles), each half summed in ascending theta and the lower
            // half added to the upper one (k_raytrace's flux sum)
            const int half = (n_theta + 1) >> 1;
            for (int p = lane; p < 2 * nb * gpw; p += 64) {
                const int h = p & 1, q = p >> 1;
                const int b = (int)(((float)q + 0.5f) * inv_gpw), gq = q - b * gpw;  // q / gpw without an integer division (q < 2^20: exact)
                const double* t = sX + (b * gpw + gq) * G + (h ? half : 0);
                const int cnt = h ? n_theta - half : half;
                double sum = 0.0;
                for (int j = 0; j < cnt; ++j) sum = add_rn(sum, t[j]);
                const double other = __shfl_xor(sum, 1);  // 2 nb gpw is even: the partner lane is in the loop too
                const int64_t iq = i0 + gq;
                if (h == 0 && iq < n_nu) C[(size_t)(gtop - b + 1) * cld + iq] = add_rn(sum, other);
            }
        }
        wave_sync();
    }
}

// Formation mean of a per-depth quantity x (geometric depth, temperature, a reference log tau): the contribution-weighted mean of its
// layer values m_k = (x[k-1] + x[k]) 0.5,  <x> = (sum_{k>=1} C[k] m_k) / (sum_{k>=1} C[k]).  One lane per frequency, both sums over ascending
// k, every operation one correctly rounded fp64 operation; a zero denominator gives what IEEE gives.
__global__ __launch_bounds__(kBlock) void k_formation_mean(int n_depth, int64_t n_nu, const double* __restrict__ C, int64_t cld,
                                                           const double* __restrict__ x, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_nu) return;
    double num = 0.0, den = 0.0;
    for (int k = 1; k < n_depth; ++k) {
        const double c = C[(size_t)k * cld + i];
        num = add_rn(num, mul_rn(c, mul_rn(add_rn(x[k - 1], x[k]), 0.5)));
        den = add_rn(den, c);
    }
    out[i] = num / den;
}

// ------------------------------------------------------------------------------------------------
// Response functions: HOW the emergent flux changes — its exact derivative with respect to the opacity and to the source function at
// every depth point (include/stardis_hip.h, sdx_response_dev, states the formulas).  The chain of affine steps I[g+1] = c[g] I[g] + e[g]
// differentiates into
//     G[j] = dI_emergent / dt[j] = T[j+1] (-p0[j] I[j] + de[j]/dt0) + T[j] de[j-1]/dt1
// which needs the intensity ENTERING gap j from below and the transmission from its upper end to the surface: two walks.  The first
// is k_raytrace's forward recurrence (rt_coef, the kernels' own (c, e)) and stashes I[j] per (ray, gap) in the wave's LDS; the second is
// k_contribution's walk from the surface inwards with the running product T and rt_coef_derivative per gap.  T[j+1] I[j] is formed
// from its two factors, never as the emergent intensity minus a suffix sum (that cancels completely in deep layers).
// Row k of either output collects from the gaps k, k-1 and k-2:
//     R_alpha[k]  = sum_theta w_theta (t[k-1] G[k-1] + t[k] G[k]) / 2      (G[k-1] needs gap k-2)
//     R_source[k] = sum_theta w_theta (T[k+1] a[k] + T[k] q[k-1] + T[k-1] r[k-2])
// so the walk visits gap k-2 and then emits row k, two rows behind the gap; what does not exist (a gap below 0 or above N_d-2) is 0.
// The layout is k_contribution's — lane <-> (frequency, angle), (S, sqrt(alpha)) pairs staged per wave from a FINISHED total_alphas
// plane, the terms of kRtBatch rows summed over theta through LDS in the flux's order — in a workgroup of one wave (RtResponse).
// Either output may be NULL: its terms are neither formed nor stored.
// The body with a compile-time flag, k_response (kAngles false: the code as it always was, wld unused) and k_response_angles below.
// kAngles (sdx_response_angles_dev): wts is a plane cot[theta][wld] and a ray's terms are weighted with ITS OWN
// frequency's cot[theta][nu] where the flux's w_theta stands otherwise — the response of sum_theta cot[theta][nu] I_theta(nu), the cotangent
// of the emergent intensities.  Nothing else differs: the same walks, the same LDS layout, the same theta sum; cot[theta][nu] = w_theta
// gives k_response's bits.
template <bool kAngles>
__device__ __forceinline__ void response_body(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                              const double* __restrict__ nus, const double* __restrict__ temps,
                                              const double* __restrict__ ray_dist, const double* __restrict__ wts, int64_t wld,
                                              const double* __restrict__ alphas, int64_t ald, const double* __restrict__ source,
                                              int64_t sld, double* __restrict__ Ra, int64_t rald, double* __restrict__ Rs,
                                              int64_t rsld, int gpw)
{
    constexpr int kBatch = kRtBatch;
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane / G, g = lane - grp * G;
    const int64_t i0 = ((int64_t)blockIdx.x * kRespWaves + wave) * gpw;  // first frequency of this wave
    const int64_t i = i0 + grp;
    const bool active = grp < gpw;
    const int64_t ic = i < n_nu ? i : n_nu - 1;
    const int n_gap = n_depth - 1;
    const int col = n_depth;
    const RtResponse lay(G, n_depth, gpw);
    const int n_slot = lay.slots();
    double* wbase = smem + (size_t)wave * lay.wave_doubles();
    double2* sP = (double2*)(wbase + lay.pairs());  // (source function, sqrt(alpha)) [gpw][col]
    double* sI = wbase + lay.stash();               // the intensity entering gap j, [n_gap][n_slot]
    double* sA = wbase + lay.terms_alpha();         // terms of R_alpha  [kBatch][gpw][G]
    double* sS = wbase + lay.terms_source();        // terms of R_source [kBatch][gpw][G]
    const double nu = nus[ic];

    if (active) {
        for (int d = g; d < n_depth; d += G)
            sP[grp * col + d] = double2{source ? source[(size_t)d * sld + ic] : planck_staged(nu, temps[d]), sqrt(alphas[(size_t)d * ald + ic])};
    }
    wave_sync();
    const RtConst kc = rt_const_literals();

    const int gi = (active ? grp : 0) * col;            // idle lanes shadow group 0 and never store
    const int slot = (active ? grp : 0) * G + g;        // (their slot is group 0's: a valid read)
    const int th = min(g, n_theta - 1);
    const double wt = g < n_theta ? (kAngles ? wts[(size_t)th * wld + ic] : wts[th]) : 0.0;
    const double* rd = ray_dist + th;                   // rd[gap * theta_stride]

    // ---- walk 1, from the bottom up: I[j], the intensity entering gap j (I[0] = 0, :134) ----
    {
        double2 pa = sP[gi], pb = sP[gi + 1];
        double t0 = mul_rn(pa.y * pb.y, rd[0]);
        double inten = 0.0;
        for (int j = 0; j < n_gap; ++j) {
            const bool last = j == n_gap - 1;
            const double2 pc = sP[gi + min(j + 2, n_gap)];
            const double t1 = last ? 0.0 : mul_rn(pb.y * pc.y, rd[(size_t)(j + 1) * theta_stride]);
            if (active) sI[j * n_slot + slot] = inten;
            double c, e;
            if (last) rt_coef<true>(t0, 0.0, pa.x - pb.x, 0.0, pb.x, c, e, kc);
            else rt_coef<false>(t0, t1, pa.x - pb.x, pc.x - pb.x, pb.x, c, e, kc);
            inten = fma(c, inten, e);
            pa = pb, pb = pc, t0 = t1;
        }
    }
    wave_sync();

    // ---- walk 2, from the surface inwards ----
    // of the gap last visited (m + 1) and the one before (m + 2), for the row being emitted (m + 2):
    double trans = 1.0;                  // T[m+1] for the gap m about to be visited
    double t_up = 0.0;                   // t[m+1]
    double x0_up = 0.0;                  // T[m+2] (-p0 I + de/dt0) of gap m+1
    double tg_up = 0.0;                  // t[m+2] G[m+2]
    double ta_up = 0.0, ta_up2 = 0.0;    // T[m+2] a[m+1], T[m+3] a[m+2]
    double tq_up = 0.0;                  // T[m+2] q[m+1]
    double2 pB = sP[gi + n_gap], pC = pB;  // the points m+1 and m+2
    double x0 = 0.0, x1 = 0.0, ta = 0.0, tq = 0.0, tr = 0.0, tm = 0.0;
    // one visit: gap m from the points (m, m+1, m+2) -> x0, x1, ta, tq, tr, tm; zeros below the first gap
    auto visit = [&](int m) {
        if (m < 0) {
            x0 = x1 = ta = tq = tr = tm = 0.0;
            return;
        }
        const double2 pA = sP[gi + m];
        tm = mul_rn(pA.y * pB.y, rd[(size_t)m * theta_stride]);
        const double inten = sI[m * n_slot + slot];
        const RtStepDerivative d = m == n_gap - 1 ? rt_coef_derivative<true>(tm, 0.0, pA.x - pB.x, 0.0, pB.x)
                                                  : rt_coef_derivative<false>(tm, t_up, pA.x - pB.x, pC.x - pB.x, pB.x);
        x0 = trans * (d.de_dt0 - d.p0 * inten);
        x1 = trans * d.de_dt1;
        ta = trans * d.a, tq = trans * d.q, tr = trans * d.r;
        trans *= d.c;  // T[m]
        pC = pB, pB = pA;
    };
    visit(n_gap - 1);  // the final gap: no row is complete yet
    t_up = tm, x0_up = x0, ta_up = ta, tq_up = tq;
    const float inv_gpw = 1.0f / (float)gpw;

    for (int ktop = n_depth - 1; ktop >= 0; ktop -= kBatch) {
        const int nb = min(kBatch, ktop + 1);
        for (int b = 0; b < nb; ++b) {
            const int k = ktop - b;
            visit(k - 2);
            const double g_up = x0_up + x1;       // G[k-1]
            const double tg = t_up * g_up;        // t[k-1] G[k-1]
            if (active) {
                if (Ra) sA[(b * gpw + grp) * G + g] = (0.5 * (tg + tg_up)) * wt;
                if (Rs) sS[(b * gpw + grp) * G + g] = ((ta_up2 + tq_up) + tr) * wt;
            }
            tg_up = tg, x0_up = x0, t_up = tm;
            ta_up2 = ta_up, ta_up = ta, tq_up = tq;
        }
        wave_sync();
        {
            // the nb rows of this batch, each output in turn: lanes <-> (row, frequency, half of the angles), each half summed in
            // ascending theta and the lower half added to the upper one (k_raytrace's flux sum)
            const int half = (n_theta + 1) >> 1;
            for (int o = 0; o < 2; ++o) {
                double* out = o ? Rs : Ra;
                if (!out) continue;
                const double* terms = o ? sS : sA;
                const int64_t ld = o ? rsld : rald;
                for (int p = lane; p < 2 * nb * gpw; p += 64) {
                    const int h = p & 1, q = p >> 1;
                    const int b = (int)(((float)q + 0.5f) * inv_gpw), gq = q - b * gpw;  // q / gpw without an integer division (q < 2^20: exact)
                    const double* t = terms + (b * gpw + gq) * G + (h ? half : 0);
                    const int cnt = h ? n_theta - half : half;
                    double sum = 0.0;
                    for (int j = 0; j < cnt; ++j) sum = add_rn(sum, t[j]);
                    const double other = __shfl_xor(sum, 1);  // 2 nb gpw is even: the partner lane is in the loop too
                    const int64_t iq = i0 + gq;
                    if (h == 0 && iq < n_nu) out[(size_t)(ktop - b) * ld + iq] = add_rn(sum, other);
                }
            }
        }
        wave_sync();
    }
}

__global__ __launch_bounds__(kRespBlock) void k_response(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                       const double* __restrict__ nus, const double* __restrict__ temps,
                                                       const double* __restrict__ ray_dist, const double* __restrict__ wts,
                                                       const double* __restrict__ alphas, int64_t ald, const double* __restrict__ source,
                                                       int64_t sld, double* __restrict__ Ra, int64_t rald, double* __restrict__ Rs,
                                                       int64_t rsld, int gpw)
{
    response_body<false>(n_depth, n_nu, n_theta, theta_stride, G, nus, temps, ray_dist, wts, 0, alphas, ald, source, sld, Ra, rald, Rs, rsld, gpw);
}
__global__ __launch_bounds__(kRespBlock) void k_response_angles(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                              const double* __restrict__ nus, const double* __restrict__ temps,
                                                              const double* __restrict__ ray_dist, const double* __restrict__ cot, int64_t cld,
                                                              const double* __restrict__ alphas, int64_t ald,
                                                              const double* __restrict__ source, int64_t sld, double* __restrict__ Ra,
                                                              int64_t rald, double* __restrict__ Rs, int64_t rsld, int gpw)
{
    response_body<true>(n_depth, n_nu, n_theta, theta_stride, G, nus, temps, ray_dist, cot, cld, alphas, ald, source, sld, Ra, rald, Rs, rsld, gpw);
}

// ------------------------------------------------------------------------------------------------
// Mean intensity of the formal solution and the scattering source function S = (1 - albedo) B + albedo J[S] (include/stardis_hip.h,
// sdx_mean_intensity_dev and sdx_scatter_source_dev, state the definition).  Coherent scattering leaves the frequencies independent:
// a column's whole iteration — the iterate, its thermal term, albedo, accelerating diagonal and mean intensity — lives in its wave's
// LDS (RtLambda) and no wave ever waits for another.
// The layout is k_contribution's and k_response's: lane <-> (frequency, angle), (S, sqrt(alpha)) pairs staged per wave from a FINISHED
// total_alphas plane, the terms of kRtBatch rows summed over theta through LDS in the flux's order.  One APPLICATION is two sweeps of
// the kernels' own step (rt_coef, tau = (sqrt(alpha[g]) sqrt(alpha[g+1])) ray_dist[g]) over the same column, written once: sweep 0 runs
// from row 0 upwards and starts at S[0], sweep 1 from row N_d - 1 downwards and starts at 0 — behind, arrival and ahead are the points
// (j, j+1, j+2) of the one and (g+1, g, g-1) of the other, the step that arrives at the sweep's last row is rt_coef<true>.  Each sweep
// leaves sum_theta m_theta (value at the row) in the wave's column, the second added to the first.  With kDiag the value is not the
// intensity but the coefficient q of the arrival point's source value in the step's e (rt_coef_derivative), 1 at the first row of the
// upward sweep: the diagonal of the operator, which depends on the optical depths alone.
// kIterate: Jacobi with that diagonal as the local operator.  All lanes of a wave sweep together for as long as one of its columns
// is live (a ballot), but a column that has stopped is never written again, so its bits do not depend on what shares its wave; the
// update of a column reads only what the two sweeps left, after both have finished.  The trip count is bounded by max_iter.
struct LambdaIteration {
    const double* scatter;  // alpha_scatter [n_depth][scatter_ld]; scatter_ld == 0: [n_depth], one value per depth point
    int64_t scatter_ld;
    double tol;
    int max_iter;
    double* S;  // [n_depth][S_ld]
    int64_t S_ld;
    int* iterations;  // per column, each may be NULL
    int* status;
    double* change;
};
// kNg: Ng acceleration of that iteration (include/stardis_hip.h, sdx_scatter_source_ng_dev, states the rule).  The updates are the plain
// ones; an update also writes the iterate it replaces into a ring of three columns (RtLambdaNg), and after it a column that is due
// replaces its iterate by the unweighted second-order extrapolation of its last four.  The five sums are per column: each lane sums
// its depths g, g + G, ... in ascending order, the G partials pass through the terms region and are added in ascending lane order, every
// operation rounded once — the order depends on (n_depth, G) alone.  Whether to extrapolate, whether the result is finite and what
// the safeguard decides are per-column decisions under the wave-uniform trip: ballots, no LDS flags, and a stopped column is never
// written.  The safeguard's state (reference change, strikes) lives in registers, the same in every lane of a column.
struct LambdaIterationNg : LambdaIteration {
    int ng_start, ng_period;
    int* accelerations;  // per column, may be NULL
};
constexpr int kNgStrikes = 2;  // extrapolations in a row without a gain before a column continues plain
constexpr double kDoubleMax = 0x1.fffffffffffffp+1023;
template <bool kIterate, bool kNg>
__device__ __forceinline__ void lambda_body(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G, const double* __restrict__ nus,
                                            const double* __restrict__ temps, const double* __restrict__ ray_dist,
                                            const double* __restrict__ mean_wts, const double* __restrict__ alphas, int64_t ald,
                                            const double* __restrict__ source, int64_t sld, double* __restrict__ J, int64_t jld,
                                            double* __restrict__ Ldiag, int64_t lld, int gpw, int waves,
                                            const std::conditional_t<kNg, LambdaIterationNg, LambdaIteration>& it)
{
    static_assert(kIterate || !kNg, "only the iteration is accelerated");
    constexpr int kBatch = kRtBatch;
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane / G, g = lane - grp * G;
    const int64_t i0 = ((int64_t)blockIdx.x * waves + wave) * gpw;  // first frequency of this wave
    const int64_t i = i0 + grp;
    const bool active = grp < gpw;
    const bool valid = active && i < n_nu;
    const int64_t ic = i < n_nu ? i : n_nu - 1;
    const int n_gap = n_depth - 1;
    const int col = n_depth;
    const std::conditional_t<kNg, RtLambdaNg, RtLambda> lay(G, n_depth, gpw);
    double* wbase = smem + (size_t)wave * lay.wave_doubles();
    double2* sP = (double2*)(wbase + lay.pairs());  // (source function — the iterate —, sqrt(alpha)) [gpw][col]
    double* sT = wbase + lay.thermal();             // (1 - albedo) B [gpw][col]
    double* sW = wbase + lay.albedo();              // albedo [gpw][col]
    double* sD = wbase + lay.diag();                // L, then 1 / (1 - albedo clamp(L)) [gpw][col]
    double* sJ = wbase + lay.mean();                // J; between the sweeps and the update, the change of the iterate [gpw][col]
    double* sX = wbase + lay.terms();               // terms of a batch of rows [kBatch][gpw][G]; the maxima of the stopping rule [2][gpw][G]
    const double nu = nus[ic];
    const int cbase = (active ? grp : 0) * col;     // idle lanes shadow group 0 and never store

    if (active) {
        for (int d = g; d < n_depth; d += G) {
            const double a = alphas[(size_t)d * ald + ic];
            const double b = source ? source[(size_t)d * sld + ic] : planck_staged(nu, temps[d]);
            sP[cbase + d] = double2{b, sqrt(a)};  // S^0 = B
            if constexpr (kIterate) {
                double w = a == 0.0 ? 0.0 : it.scatter[it.scatter_ld ? (size_t)d * it.scatter_ld + ic : (size_t)d] / a;
                w = w > 0.0 ? (w < 1.0 ? w : 1.0) : 0.0;  // clamped to [0, 1]; NaN -> 0
                sT[cbase + d] = mul_rn(sub_rn(1.0, w), b);
                sW[cbase + d] = w;
            }
        }
    }
    wave_sync();
    const RtConst kc = rt_const_literals();  // (literals, as in k_raytrace: the step loops are rolled)
    const int th = min(g, n_theta - 1);
    const double wt = g < n_theta ? mean_wts[th] : 0.0;
    const double* rd = ray_dist + th;  // rd[gap * theta_stride]
    const float inv_gpw = 1.0f / (float)gpw;
    const int half = (n_theta + 1) >> 1;

    // the nb rows first, first + step, ... of a batch: lanes <-> (row, frequency, half of the angles), each half summed in ascending theta
    // and the lower half added to the upper one (k_raytrace's flux sum) -> dst[frequency][row], written or added to
    auto reduce = [&](int nb, int first, int step, bool add, double* dst) {
        for (int p = lane; p < 2 * nb * gpw; p += 64) {
            const int h = p & 1, q = p >> 1;
            const int b = (int)(((float)q + 0.5f) * inv_gpw), gq = q - b * gpw;  // q / gpw without an integer division (q < 2^20: exact)
            const double* t = sX + (b * gpw + gq) * G + (h ? half : 0);
            const int cnt = h ? n_theta - half : half;
            double sum = 0.0;
            for (int j = 0; j < cnt; ++j) sum = add_rn(sum, t[j]);
            const double other = __shfl_xor(sum, 1);  // 2 nb gpw is even: the partner lane is in the loop too
            if (h == 0) {
                double* o = dst + gq * col + first + b * step;
                const double tot = add_rn(sum, other);
                *o = add ? add_rn(*o, tot) : tot;
            }
        }
    };
    // one application of the operator (or, kDiag, its diagonal) to the wave's columns -> dst [gpw][col]
    auto apply = [&](auto diag_tag, double* dst) {
        constexpr bool kDiag = decltype(diag_tag)::value;
        for (int dir = 0; dir < 2; ++dir) {
            const int sgn = dir ? -1 : 1, start = dir ? n_gap : 0;
            double2 pa = sP[cbase + start], pb = sP[cbase + start + sgn];  // the points behind and at the arrival of step 0
            double t0 = mul_rn(pa.y * pb.y, rd[(size_t)(dir ? n_gap - 1 : 0) * theta_stride]);
            double val = dir ? 0.0 : (kDiag ? 1.0 : pa.x);  // U[0] = S[0]: a thermalised lower boundary; D[N_d-1] = 0
            if (active) sX[grp * G + g] = val * wt;
            wave_sync();
            reduce(1, start, sgn, dir != 0, dst);
            wave_sync();
            for (int s0 = 0; s0 < n_gap; s0 += kBatch) {
                const int nb = min(kBatch, n_gap - s0);
                for (int b = 0; b < nb; ++b) {
                    const int s = s0 + b;
                    const bool last = s == n_gap - 1;
                    const int pt = start + sgn * (s + 1);                      // the arrival point
                    const double2 pc = sP[cbase + (last ? pt : pt + sgn)];     // the point ahead
                    const double t1 = last ? 0.0 : mul_rn(pb.y * pc.y, rd[(size_t)(dir ? pt - 1 : pt) * theta_stride]);
                    if constexpr (kDiag) {
                        val = last ? rt_coef_derivative<true>(t0, 0.0, 0.0, 0.0, 0.0).q : rt_coef_derivative<false>(t0, t1, 0.0, 0.0, 0.0).q;
                    } else {
                        double c, e;
                        if (last) rt_coef<true>(t0, 0.0, pa.x - pb.x, 0.0, pb.x, c, e, kc);
                        else rt_coef<false>(t0, t1, pa.x - pb.x, pc.x - pb.x, pb.x, c, e, kc);
                        val = fma(c, val, e);
                    }
                    if (active) sX[(b * gpw + grp) * G + g] = val * wt;
                    pa = pb, pb = pc, t0 = t1;
                }
                wave_sync();
                reduce(nb, start + sgn * (s0 + 1), sgn, dir != 0, dst);
                wave_sync();
            }
        }
    };
    auto store_column = [&](const double* colv, double* out, int64_t ld) {
        if (valid)
            for (int d = g; d < n_depth; d += G) out[(size_t)d * ld + i] = colv[cbase + d];
    };

    if constexpr (!kIterate) {
        if (J) {
            apply(std::false_type{}, sJ);
            store_column(sJ, J, jld);
        }
        if (Ldiag) {
            apply(std::true_type{}, sD);
            store_column(sD, Ldiag, lld);
        }
    } else {
        apply(std::true_type{}, sD);
        if (active) {
            for (int d = g; d < n_depth; d += G) {
                const double l = sD[cbase + d];
                const double lh = l > 0.0 ? (l < 1.0 ? l : 1.0) : 0.0;  // clamp(L, 0, 1): changes the rate, never the fixed point
                sD[cbase + d] = 1.0 / sub_rn(1.0, mul_rn(sW[cbase + d], lh));
            }
        }
        wave_sync();
        bool live = valid;
        int iters = 0, status = 1;
        double change = 0.0;
        // kNg, per column: iterates of history (the current one included), updates since the last extrapolation, whether the column
        // is still accelerated and awaits the safeguard's judgement, its strikes, the reference change, the extrapolations applied
        [[maybe_unused]] int held = 1, since = 0, strikes = 0, accs = 0;
        [[maybe_unused]] bool ng_on = true, probation = false;
        [[maybe_unused]] double reference = 0.0;
        if constexpr (kNg) since = it.ng_period;
        for (int n = 1;; ++n) {
            const bool more = n <= it.max_iter && __builtin_amdgcn_ballot_w64(live) != 0;  // wave-uniform
            if (!more && !J) break;
            apply(std::false_type{}, sJ);  // J[S^n]; in the trip after the last update, the J of what is returned
            if (!more) break;
            double md = 0.0, ms = 0.0;
            if (active) {
                for (int d = g; d < n_depth; d += G) {
                    const double s = sP[cbase + d].x;
                    const double r = sub_rn(add_rn(sT[cbase + d], mul_rn(sW[cbase + d], sJ[cbase + d])), s);
                    const double ds = mul_rn(r, sD[cbase + d]);
                    sJ[cbase + d] = ds;
                    double ad = fabs(ds);
                    if (!(ad <= kDoubleMax)) ad = __builtin_huge_val();  // not finite: the column stops (status 2)
                    const double as = fabs(add_rn(s, ds));
                    md = ad > md ? ad : md;
                    ms = as > ms ? as : ms;
                }
                sX[grp * G + g] = md;
                sX[(gpw + grp) * G + g] = ms;
            }
            wave_sync();
            double cd = 0.0, cs = 0.0;  // the column's max |dS| and max |S^(n+1)|: maxima, so the order of the lanes does not matter
            {
                const int xb = (active ? grp : 0) * G;
                for (int t = 0; t < G; ++t) {
                    const double vd = sX[xb + t], vs = sX[gpw * G + xb + t];
                    cd = vd > cd ? vd : cd;
                    cs = vs > cs ? vs : cs;
                }
            }
            wave_sync();
            if (live) {
                iters = n, change = cd;
                if (!(cd <= kDoubleMax)) {
                    status = 2, live = false;  // S stays at the last finite iterate
                } else {
                    if constexpr (kNg) {
                        double* ring = wbase + lay.history(n % 3);  // the iterate this update replaces: x1 of the next extrapolation
                        for (int d = g; d < n_depth; d += G) {
                            const double s = sP[cbase + d].x;
                            ring[cbase + d] = s;
                            sP[cbase + d].x = add_rn(s, sJ[cbase + d]);
                        }
                        ++held, ++since;
                    } else {
                        for (int d = g; d < n_depth; d += G) sP[cbase + d].x = add_rn(sP[cbase + d].x, sJ[cbase + d]);
                    }
                    if (cd <= mul_rn(it.tol, cs)) status = 0, live = false;
                }
            }
            if constexpr (kNg) {
                double* sF = wbase + lay.history(3);  // the iterate the last judged-from extrapolation replaced
                // the safeguard: a whole period after an extrapolation, the change against the one before it
                if (live && ng_on && probation && since >= it.ng_period) {
                    if (cd < reference) {
                        strikes = 0;
                    } else if (++strikes >= kNgStrikes) {
                        for (int d = g; d < n_depth; d += G) sP[cbase + d].x = sF[cbase + d];
                        ng_on = false;
                    }
                }
                if (since >= it.ng_period) probation = false;
                const bool want = live && ng_on && n >= it.ng_start && n < it.max_iter && since >= it.ng_period && held >= 4;
                if (__builtin_amdgcn_ballot_w64(want) != 0) {  // wave-uniform
                    const double* h1 = wbase + lay.history(n % 3);
                    const double* h2 = wbase + lay.history((n + 2) % 3);
                    const double* h3 = wbase + lay.history((n + 1) % 3);
                    if (want) {
                        double a1 = 0.0, b1 = 0.0, c1 = 0.0, b2 = 0.0, c2 = 0.0;
                        for (int d = g; d < n_depth; d += G) {
                            const double x0 = sP[cbase + d].x, x1 = h1[cbase + d], x2 = h2[cbase + d], x3 = h3[cbase + d];
                            const double q1 = add_rn(sub_rn(x0, mul_rn(2.0, x1)), x2);
                            const double q2 = add_rn(sub_rn(sub_rn(x0, x1), x2), x3);
                            const double q3 = sub_rn(x0, x1);
                            a1 = add_rn(a1, mul_rn(q1, q1));
                            b1 = add_rn(b1, mul_rn(q1, q2));
                            c1 = add_rn(c1, mul_rn(q1, q3));
                            b2 = add_rn(b2, mul_rn(q2, q2));
                            c2 = add_rn(c2, mul_rn(q2, q3));
                        }
                        const int xs = grp * G + g, stride = gpw * G;
                        sX[xs] = a1, sX[stride + xs] = b1, sX[2 * stride + xs] = c1, sX[3 * stride + xs] = b2, sX[4 * stride + xs] = c2;
                    }
                    wave_sync();
                    bool bad = false;
                    if (want) {
                        const int xb = grp * G, stride = gpw * G;
                        double A1 = 0.0, B1 = 0.0, C1 = 0.0, B2 = 0.0, C2 = 0.0;
                        for (int t = 0; t < G; ++t) {
                            A1 = add_rn(A1, sX[xb + t]);
                            B1 = add_rn(B1, sX[stride + xb + t]);
                            C1 = add_rn(C1, sX[2 * stride + xb + t]);
                            B2 = add_rn(B2, sX[3 * stride + xb + t]);
                            C2 = add_rn(C2, sX[4 * stride + xb + t]);
                        }
                        const double det = sub_rn(mul_rn(A1, B2), mul_rn(B1, B1));
                        const double a = sub_rn(mul_rn(C1, B2), mul_rn(C2, B1)) / det;
                        const double b = sub_rn(mul_rn(C2, A1), mul_rn(C1, B1)) / det;
                        const double k0 = sub_rn(sub_rn(1.0, a), b);
                        for (int d = g; d < n_depth; d += G) {
                            const double e = add_rn(add_rn(mul_rn(k0, sP[cbase + d].x), mul_rn(a, h1[cbase + d])), mul_rn(b, h2[cbase + d]));
                            sJ[cbase + d] = e;  // (the change of the iterate has been consumed)
                            bad = bad || !(fabs(e) <= kDoubleMax);
                        }
                    }
                    // a column's lanes are grp G .. grp G + G - 1: one non-finite component anywhere skips the column's extrapolation
                    const uint64_t bad_lanes = __builtin_amdgcn_ballot_w64(bad);
                    const uint64_t mine = (G == 64 ? ~0ull : ((1ull << G) - 1)) << (active ? grp * G : 0);
                    if (want && !(bad_lanes & mine)) {
                        const bool fresh = strikes == 0;
                        for (int d = g; d < n_depth; d += G) {
                            if (fresh) sF[cbase + d] = sP[cbase + d].x;
                            sP[cbase + d].x = sJ[cbase + d];
                        }
                        if (fresh) reference = cd;
                        held = 1, since = 0, probation = true, ++accs;
                    }
                }
            }
            wave_sync();
        }
        if (valid) {
            for (int d = g; d < n_depth; d += G) it.S[(size_t)d * it.S_ld + i] = sP[cbase + d].x;
            if (g == 0) {
                if (it.iterations) it.iterations[i] = iters;
                if (it.status) it.status[i] = status;
                if (it.change) it.change[i] = change;
                if constexpr (kNg)
                    if (it.accelerations) it.accelerations[i] = accs;
            }
        }
        if (J) store_column(sJ, J, jld);
    }
}

template <bool kIterate>
__global__ __launch_bounds__(kRtBlock) void k_lambda(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                   const double* __restrict__ nus, const double* __restrict__ temps,
                                                   const double* __restrict__ ray_dist, const double* __restrict__ mean_wts,
                                                   const double* __restrict__ alphas, int64_t ald, const double* __restrict__ source,
                                                   int64_t sld, double* __restrict__ J, int64_t jld, double* __restrict__ Ldiag, int64_t lld,
                                                   int gpw, int waves, LambdaIteration it)
{
    lambda_body<kIterate, false>(n_depth, n_nu, n_theta, theta_stride, G, nus, temps, ray_dist, mean_wts, alphas, ald, source, sld, J, jld, Ldiag, lld, gpw, waves, it);
}
// k_lambda<true> with Ng acceleration (a kernel name of its own: the plain family keeps its two instantiations and their figures)
__global__ __launch_bounds__(kRtBlock) void k_lambda_ng(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                      const double* __restrict__ nus, const double* __restrict__ temps,
                                                      const double* __restrict__ ray_dist, const double* __restrict__ mean_wts,
                                                      const double* __restrict__ alphas, int64_t ald, const double* __restrict__ source,
                                                      int64_t sld, double* __restrict__ J, int64_t jld, int gpw, int waves, LambdaIterationNg it)
{
    lambda_body<true, true>(n_depth, n_nu, n_theta, theta_stride, G, nus, temps, ray_dist, mean_wts, alphas, ald, source, sld, J, jld, nullptr, 0, gpw, waves, it);
}

// ------------------------------------------------------------------------------------------------
// The adjoint of the mean-intensity operator and of the scattering solve (include/stardis_hip.h, sdx_mean_intensity_adjoint_dev and
// sdx_scatter_response_dev, state the definitions).  k_lambda's mapping — lane <-> (frequency, angle), a wave's columns in its own LDS
// (RtLambdaAdjoint), no wave waits for another, no atomics — and k_response's two-walk scheme, once per sweep of the operator:
//   transposed application   a lane walks AGAINST the sweep with the adjoint of the value, vbar[s] = m z[p_s] + c[s] vbar[s+1], and the
//                            row at sweep position j collects (a[j] vbar[j+1] + q[j-1] vbar[j]) + r[j-2] vbar[j-1] — the walk visits
//                            step j-2 and then emits row j, two rows behind the step, as k_response does; the row the upward sweep
//                            starts from also takes vbar[0].  (c, a, q, r) are the forward step's OWN: e is linear in the three
//                            source values, so rt_coef on unit differences returns them, and what is transposed is the operator
//                            k_lambda applies, to rounding (rt_coef_derivative's forms of the same coefficients are more accurate
//                            near tau = 5e-4 than the step is, and z . J[x] = (Lambda^T z) . x would hold to 1e-8 only).  They
//                            depend on the optical depths alone, so the solve's loop needs no stash.
//   differentiated           the forward sweep (k_lambda's, rt_coef) stashes the value entering every step per ray; the reverse walk forms
//   application              tbar[j] = vbar[j+1] (de/dt0[j] - p0[j] val[j]) + vbar[j] de/dt1[j-1] and the row takes (t[j-1] tbar[j-1] +
//                            t[j] tbar[j]) / 2.  One stash serves both sweeps in turn.
// The rows of a batch are summed over theta through LDS in the flux's order; the downward sweep's sums are added to the upward one's.
// kSolve: y = c + Lambda^T (W y) by Jacobi with the forward kernel's local operator 1 / (1 - albedo clamp(L)), L formed as k_lambda
// forms it; the stopping rule, the three statuses, the refused non-finite update and the frozen column are k_lambda<true>'s, line by
// line.  Then, where an opacity derivative is asked for, the differentiated application at z = W y (which also leaves J of S), and the
// combination of the outputs per depth point.
struct LambdaAdjointSolve {
    const double* scatter;  // alpha_scatter [n_depth][scatter_ld]; scatter_ld == 0: [n_depth]
    int64_t scatter_ld;
    const double* thermal;  // B [n_depth][thermal_ld]; NULL: Planck
    int64_t thermal_ld;
    const double* cotangent;  // [n_depth][cotangent_ld]
    int64_t cotangent_ld;
    const double* direct;  // [n_depth][direct_ld]; NULL: 0
    int64_t direct_ld;
    double tol;
    int max_iter;
    double* y;  // outputs [n_depth][ld], each may be NULL
    int64_t y_ld;
    double* R_thermal;
    int64_t R_thermal_ld;
    double* R_absorption;
    int64_t R_absorption_ld;
    double* R_scatter;
    int64_t R_scatter_ld;
    int* iterations;  // per column, each may be NULL
    int* status;
    double* change;
};
template <bool kSolve>
__global__ __launch_bounds__(kRtBlock) void k_lambda_adjoint(int n_depth, int64_t n_nu, int n_theta, int theta_stride, int G,
                                                           const double* __restrict__ nus, const double* __restrict__ temps,
                                                           const double* __restrict__ ray_dist, const double* __restrict__ mean_wts,
                                                           const double* __restrict__ alphas, int64_t ald, const double* __restrict__ source,
                                                           int64_t sld, const double* __restrict__ z, int64_t zld, double* __restrict__ Lt,
                                                           int64_t ltld, double* __restrict__ Gout, int64_t gld, int gpw, int waves,
                                                           LambdaAdjointSolve it)
{
    constexpr int kBatch = kRtBatch;
    extern __shared__ double smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane / G, g = lane - grp * G;
    const int64_t i0 = ((int64_t)blockIdx.x * waves + wave) * gpw;  // first frequency of this wave
    const int64_t i = i0 + grp;
    const bool active = grp < gpw;
    const bool valid = active && i < n_nu;
    const int64_t ic = i < n_nu ? i : n_nu - 1;
    const int n_gap = n_depth - 1;
    const int col = n_depth;
    const RtLambdaAdjoint lay(G, n_depth, gpw);
    const int n_slot = lay.slots();
    double* wbase = smem + (size_t)wave * lay.wave_doubles();
    double2* sP = (double2*)(wbase + lay.pairs());  // (source function S, sqrt(alpha)) [gpw][col]
    double* sZ = wbase + lay.z();                   // what Lambda^T is applied to [gpw][col]
    double* sR = wbase + lay.result();              // Lambda^T z
    double* sY = wbase + lay.iterate();             // y
    double* sC = wbase + lay.cotangent();           // c
    double* sW = wbase + lay.albedo();              // albedo
    double* sD = wbase + lay.diag();                // L, then 1 / (1 - albedo clamp(L))
    double* sJ = wbase + lay.mean();                // J of S
    double* sG = wbase + lay.gradient();            // d(z^T J[S]) / d ln alpha
    double* sI = wbase + lay.stash();               // the value entering step s, [n_gap][n_slot]
    double* sX = wbase + lay.terms();               // terms of a batch of rows [kBatch][gpw][G]; the maxima of the stopping rule [2][gpw][G]
    const double nu = nus[ic];
    const int cbase = (active ? grp : 0) * col;     // idle lanes shadow group 0 and never store
    const int slot = (active ? grp : 0) * G + g;

    if (active) {
        for (int d = g; d < n_depth; d += G) {
            const double a = alphas[(size_t)d * ald + ic];
            sP[cbase + d] = double2{source ? source[(size_t)d * sld + ic] : planck_staged(nu, temps[d]), sqrt(a)};
            if constexpr (kSolve) {
                double w = a == 0.0 ? 0.0 : it.scatter[it.scatter_ld ? (size_t)d * it.scatter_ld + ic : (size_t)d] / a;
                w = w > 0.0 ? (w < 1.0 ? w : 1.0) : 0.0;  // clamped to [0, 1]; NaN -> 0
                const double c = it.cotangent[(size_t)d * it.cotangent_ld + ic];
                sW[cbase + d] = w;
                sC[cbase + d] = c;
                sY[cbase + d] = c;  // y^0 = c
            } else {
                sZ[cbase + d] = z[(size_t)d * zld + ic];
            }
        }
    }
    wave_sync();
    const RtConst kc = rt_const_literals();
    const int th = min(g, n_theta - 1);
    const double wt = g < n_theta ? mean_wts[th] : 0.0;
    const double* rd = ray_dist + th;  // rd[gap * theta_stride]
    const float inv_gpw = 1.0f / (float)gpw;
    const int half = (n_theta + 1) >> 1;

    // k_lambda's: the nb rows first, first + step, ... of a batch, each half of the angles summed in ascending theta and the lower half
    // added to the upper one -> dst[frequency][row], written or added to
    auto reduce = [&](int nb, int first, int step, bool add, double* dst) {
        for (int p = lane; p < 2 * nb * gpw; p += 64) {
            const int h = p & 1, q = p >> 1;
            const int b = (int)(((float)q + 0.5f) * inv_gpw), gq = q - b * gpw;  // q / gpw without an integer division (q < 2^20: exact)
            const double* t = sX + (b * gpw + gq) * G + (h ? half : 0);
            const int cnt = h ? n_theta - half : half;
            double sum = 0.0;
            for (int j = 0; j < cnt; ++j) sum = add_rn(sum, t[j]);
            const double other = __shfl_xor(sum, 1);  // 2 nb gpw is even: the partner lane is in the loop too
            if (h == 0) {
                double* o = dst + gq * col + first + b * step;
                const double tot = add_rn(sum, other);
                *o = add ? add_rn(*o, tot) : tot;
            }
        }
    };
    // k_lambda's sweep dir over the wave's columns.  kDiag: the diagonal -> dst.  Otherwise the values of S: the value entering every
    // step goes to the stash, and with dst the mean intensity is summed (dir 0 written, dir 1 added).
    auto forward = [&](auto diag_tag, int dir, double* dst) {
        constexpr bool kDiag = decltype(diag_tag)::value;
        const int sgn = dir ? -1 : 1, start = dir ? n_gap : 0;
        double2 pa = sP[cbase + start], pb = sP[cbase + start + sgn];  // the points behind and at the arrival of step 0
        double t0 = mul_rn(pa.y * pb.y, rd[(size_t)(dir ? n_gap - 1 : 0) * theta_stride]);
        double val = dir ? 0.0 : (kDiag ? 1.0 : pa.x);  // U[0] = S[0]: a thermalised lower boundary; D[N_d-1] = 0
        if (dst) {
            if (active) sX[grp * G + g] = val * wt;
            wave_sync();
            reduce(1, start, sgn, dir != 0, dst);
            wave_sync();
        }
        for (int s0 = 0; s0 < n_gap; s0 += kBatch) {
            const int nb = min(kBatch, n_gap - s0);
            for (int b = 0; b < nb; ++b) {
                const int s = s0 + b;
                const bool last = s == n_gap - 1;
                const int pt = start + sgn * (s + 1);                      // the arrival point
                const double2 pc = sP[cbase + (last ? pt : pt + sgn)];     // the point ahead
                const double t1 = last ? 0.0 : mul_rn(pb.y * pc.y, rd[(size_t)(dir ? pt - 1 : pt) * theta_stride]);
                if constexpr (kDiag) {
                    val = last ? rt_coef_derivative<true>(t0, 0.0, 0.0, 0.0, 0.0).q : rt_coef_derivative<false>(t0, t1, 0.0, 0.0, 0.0).q;
                } else {
                    if (active) sI[s * n_slot + slot] = val;
                    double c, e;
                    if (last) rt_coef<true>(t0, 0.0, pa.x - pb.x, 0.0, pb.x, c, e, kc);
                    else rt_coef<false>(t0, t1, pa.x - pb.x, pc.x - pb.x, pb.x, c, e, kc);
                    val = fma(c, val, e);
                }
                if (dst && active) sX[(b * gpw + grp) * G + g] = val * wt;
                pa = pb, pb = pc, t0 = t1;
            }
            if (dst) {
                wave_sync();
                reduce(nb, start + sgn * (s0 + 1), sgn, dir != 0, dst);
                wave_sync();
            }
        }
    };
    // the walk against sweep dir with the plane zc.  kGrad: the opacity derivative of z^T J[S] from the stash of forward(dir) -> dst;
    // otherwise Lambda^T z -> dst.  dir 0 writes, dir 1 adds.
    auto backward = [&](auto grad_tag, int dir, const double* zc, double* dst) {
        constexpr bool kGrad = decltype(grad_tag)::value;
        const int sgn = dir ? -1 : 1, start = dir ? n_gap : 0;
        double vbar = mul_rn(wt, zc[cbase + start + sgn * n_gap]);  // of the value at the sweep's last row
        double t_up = 0.0;                   // tau of step m+1
        double x0_up = 0.0;                  // vbar[m+2] (de/dt0 - p0 val) of step m+1
        double tg_up = 0.0;                  // t[m+2] tbar[m+2]
        double ta_up = 0.0, ta_up2 = 0.0;    // vbar[m+2] a[m+1], vbar[m+3] a[m+2]
        double tq_up = 0.0;                  // vbar[m+2] q[m+1]
        double2 pB = sP[cbase + start + sgn * n_gap], pC = pB;  // the arrival point of step m and the point ahead
        double x0 = 0.0, x1 = 0.0, ta = 0.0, tq = 0.0, tr = 0.0, tm = 0.0;
        // one visit: step m from the points (m, m+1, m+2) of the sweep -> x0, x1 or ta, tq, tr, and tm; zeros below the first step
        auto visit = [&](int m) {
            if (m < 0) {
                x0 = x1 = ta = tq = tr = tm = 0.0;
                return;
            }
            const double2 pA = sP[cbase + start + sgn * m];
            tm = mul_rn(pA.y * pB.y, rd[(size_t)(dir ? n_gap - 1 - m : m) * theta_stride]);
            double c;
            if constexpr (kGrad) {
                const RtStepDerivative d = m == n_gap - 1 ? rt_coef_derivative<true>(tm, 0.0, pA.x - pB.x, 0.0, pB.x)
                                                          : rt_coef_derivative<false>(tm, t_up, pA.x - pB.x, pC.x - pB.x, pB.x);
                const double val = sI[m * n_slot + slot];
                x0 = mul_rn(vbar, sub_rn(d.de_dt0, mul_rn(d.p0, val)));
                x1 = mul_rn(vbar, d.de_dt1);
                c = d.c;
            } else {
                // e is linear in (S[behind] - S[arrival], S[ahead] - S[arrival], S[arrival]): the step on unit differences gives a, r and q
                double a, q, r = 0.0;
                if (m == n_gap - 1) {
                    rt_coef<true>(tm, 0.0, 1.0, 0.0, 0.0, c, a, kc);
                    rt_coef<true>(tm, 0.0, -1.0, 0.0, 1.0, c, q, kc);
                } else {
                    rt_coef<false>(tm, t_up, 1.0, 0.0, 0.0, c, a, kc);
                    rt_coef<false>(tm, t_up, 0.0, 1.0, 0.0, c, r, kc);
                    rt_coef<false>(tm, t_up, -1.0, -1.0, 1.0, c, q, kc);
                }
                ta = mul_rn(vbar, a), tq = mul_rn(vbar, q), tr = mul_rn(vbar, r);
            }
            vbar = add_rn(mul_rn(wt, zc[cbase + start + sgn * m]), mul_rn(c, vbar));
            pC = pB, pB = pA;
        };
        visit(n_gap - 1);  // the sweep's last step: no row is complete yet
        t_up = tm, x0_up = x0, ta_up = ta, tq_up = tq;
        for (int ktop = n_depth - 1; ktop >= 0; ktop -= kBatch) {
            const int nb = min(kBatch, ktop + 1);
            for (int b = 0; b < nb; ++b) {
                const int k = ktop - b;  // the row's position in the sweep
                visit(k - 2);
                double term;
                if constexpr (kGrad) {
                    const double tg = mul_rn(t_up, add_rn(x0_up, x1));  // t[k-1] tbar[k-1]
                    term = mul_rn(0.5, add_rn(tg, tg_up));
                    tg_up = tg, x0_up = x0;
                } else {
                    term = add_rn(add_rn(ta_up2, tq_up), tr);
                    if (k == 0 && dir == 0) term = add_rn(term, vbar);  // U[0] = S[0]
                    ta_up2 = ta_up, ta_up = ta, tq_up = tq;
                }
                t_up = tm;
                if (active) sX[(b * gpw + grp) * G + g] = g < n_theta ? term : 0.0;
            }
            wave_sync();
            reduce(nb, start + sgn * ktop, -sgn, dir != 0, dst);
            wave_sync();
        }
    };
    auto store_column = [&](const double* colv, double* out, int64_t ld) {
        if (valid)
            for (int d = g; d < n_depth; d += G) out[(size_t)d * ld + i] = colv[cbase + d];
    };

    if constexpr (!kSolve) {
        if (Lt) {
            backward(std::false_type{}, 0, sZ, sR);
            backward(std::false_type{}, 1, sZ, sR);
            store_column(sR, Lt, ltld);
        }
        if (Gout) {
            for (int dir = 0; dir < 2; ++dir) {
                forward(std::false_type{}, dir, (double*)nullptr);
                wave_sync();
                backward(std::true_type{}, dir, sZ, sG);
            }
            store_column(sG, Gout, gld);
        }
    } else {
        forward(std::true_type{}, 0, sD);
        forward(std::true_type{}, 1, sD);
        if (active) {
            for (int d = g; d < n_depth; d += G) {
                const double l = sD[cbase + d];
                const double lh = l > 0.0 ? (l < 1.0 ? l : 1.0) : 0.0;  // clamp(L, 0, 1)
                sD[cbase + d] = 1.0 / sub_rn(1.0, mul_rn(sW[cbase + d], lh));
                sZ[cbase + d] = mul_rn(sW[cbase + d], sY[cbase + d]);
            }
        }
        wave_sync();
        bool live = valid;
        int iters = 0, status = 1;
        double change = 0.0;
        for (int n = 1;; ++n) {
            const bool more = n <= it.max_iter && __builtin_amdgcn_ballot_w64(live) != 0;  // wave-uniform
            if (!more) break;
            backward(std::false_type{}, 0, sZ, sR);  // Lambda^T (W y^n)
            backward(std::false_type{}, 1, sZ, sR);
            double md = 0.0, ms = 0.0;
            if (active) {
                for (int d = g; d < n_depth; d += G) {
                    const double y = sY[cbase + d];
                    const double r = sub_rn(add_rn(sC[cbase + d], sR[cbase + d]), y);
                    const double dy = mul_rn(r, sD[cbase + d]);
                    sR[cbase + d] = dy;
                    double ad = fabs(dy);
                    if (!(ad <= kDoubleMax)) ad = __builtin_huge_val();  // not finite: the column stops (status 2)
                    const double as = fabs(add_rn(y, dy));
                    md = ad > md ? ad : md;
                    ms = as > ms ? as : ms;
                }
                sX[grp * G + g] = md;
                sX[(gpw + grp) * G + g] = ms;
            }
            wave_sync();
            double cd = 0.0, cs = 0.0;  // the column's max |dy| and max |y^(n+1)|
            {
                const int xb = (active ? grp : 0) * G;
                for (int t = 0; t < G; ++t) {
                    const double vd = sX[xb + t], vs = sX[gpw * G + xb + t];
                    cd = vd > cd ? vd : cd;
                    cs = vs > cs ? vs : cs;
                }
            }
            wave_sync();
            if (live) {
                iters = n, change = cd;
                if (!(cd <= kDoubleMax)) {
                    status = 2, live = false;  // y stays at the last finite iterate
                } else {
                    for (int d = g; d < n_depth; d += G) {
                        const double y = add_rn(sY[cbase + d], sR[cbase + d]);
                        sY[cbase + d] = y;
                        sZ[cbase + d] = mul_rn(sW[cbase + d], y);
                    }
                    if (cd <= mul_rn(it.tol, cs)) status = 0, live = false;
                }
            }
            wave_sync();
        }
        const bool want_grad = it.R_absorption || it.R_scatter;
        if (want_grad) {
            for (int dir = 0; dir < 2; ++dir) {
                forward(std::false_type{}, dir, sJ);
                backward(std::true_type{}, dir, sZ, sG);
            }
        }
        if (valid) {
            for (int d = g; d < n_depth; d += G) {
                const double y = sY[cbase + d], w = sW[cbase + d];
                const size_t row = (size_t)d;
                if (it.y) it.y[row * it.y_ld + i] = y;
                if (it.R_thermal) it.R_thermal[row * it.R_thermal_ld + i] = mul_rn(sub_rn(1.0, w), y);
                if (want_grad) {
                    const double b = it.thermal ? it.thermal[row * it.thermal_ld + i] : planck_staged(nu, temps[d]);
                    const double A = add_rn(it.direct ? it.direct[row * it.direct_ld + i] : 0.0, sG[cbase + d]);
                    const double H = mul_rn(y, sub_rn(sJ[cbase + d], b));
                    if (it.R_absorption) it.R_absorption[row * it.R_absorption_ld + i] = sub_rn(A, mul_rn(w, H));
                    if (it.R_scatter) it.R_scatter[row * it.R_scatter_ld + i] = add_rn(mul_rn(w, A), mul_rn(mul_rn(w, sub_rn(1.0, w)), H));
                }
            }
            if (g == 0) {
                if (it.iterations) it.iterations[i] = iters;
                if (it.status) it.status[i] = status;
                if (it.change) it.change[i] = change;
            }
        }
    }
}

// The response to a scale factor on ONE part of the opacity: out[nu] = sum_k R_alpha[k][nu] (part[k][nu] / total[k][nu]), the
// derivative of the emergent flux with respect to the logarithm of that factor (d ln alpha[k] = part[k] / total[k] d ln factor).  One lane per
// frequency, ascending k, every operation one correctly rounded fp64 operation; a zero in total gives what IEEE gives.
__global__ __launch_bounds__(kBlock) void k_response_project(int n_depth, int64_t n_nu, const double* __restrict__ R, int64_t rld,
                                                             const double* __restrict__ part, int64_t pld, const double* __restrict__ total,
                                                             int64_t tld, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_nu) return;
    double acc = 0.0;
    for (int k = 0; k < n_depth; ++k)
        acc = add_rn(acc, mul_rn(R[(size_t)k * rld + i], part[(size_t)k * pld + i] / total[(size_t)k * tld + i]));
    out[i] = acc;
}

// ------------------------------------------------------------------------------------------------
// scipy.ndimage.convolve1d(in, w) with the default mode='reflect' (d c b a | a b c d | d c b a), odd kernel, origin 0:
// what rotation_broadening applies to the spectrum (broadening.py:869-871).  scipy's summation order is kept:
// for a symmetric kernel  out = in[0] w[c], then pairs (in[-j] + in[+j]) w[c-j] from the OUTERMOST inwards;
// otherwise the last tap first, then the ascending-offset sum with the reversed kernel.
__device__ __forceinline__ int64_t reflect_index(int64_t i, int64_t n)
{
    const int64_t p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - 1 - i : i;
}
__global__ __launch_bounds__(kBlock) void k_convolve1d_reflect(int64_t n, const double* __restrict__ in, int m,
                                                               const double* __restrict__ w, int symmetric,
                                                               double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int h = m / 2;
    double acc;
    if (symmetric) {
        acc = mul_rn(in[i], w[h]);
        for (int j = h; j >= 1; --j) acc = add_rn(acc, mul_rn(add_rn(in[reflect_index(i - j, n)], in[reflect_index(i + j, n)]), w[h - j]));
    } else {
        acc = mul_rn(in[reflect_index(i + h, n)], w[0]);  // scipy starts from the last tap, then ascends
        for (int jj = -h; jj < h; ++jj) acc = add_rn(acc, mul_rn(in[reflect_index(i + jj, n)], w[h - jj]));
    }
    out[i] = acc;
}

// ------------------------------------------------------------------------------------------------
// The instrument model (include/stardis_hip.h, sdx_observe_dev): Doppler shift, a Gaussian line-spread function whose width is
// given per pixel, and integration over the detector's pixels, in one launch:
//     x_i = lambdas[i] D,   h_i = the trapezoid weight of x_i,   r_ij = the Gaussian of width sigma[j] around x_i integrated over pixel j,
//     out[j] = (sum_i r_ij h_i flux[i]) / (sum_i r_ij h_i g_i)  over the points with edges[j] - 8 sigma[j] <= x_i <= edges[j+1] + 8 sigma[j]
// (g = 1, or the reference spectrum); NaN where the grid does not cover that window.  fp64, every operation one rounded operation.
//
// One wave per pixel; the pixels go in groups of kObsGroup.  A group whose windows are short — none is expected to hold more than
// kObsShort points at the grid's MEAN spacing, (x_{n-1} - x_0) / (n - 1): an estimate, taken before anything is searched — is done by its
// FIRST wave, eight lanes per pixel, and the other waves leave at once: an undersampled line-spread function has one to five points per
// window, and a wave per pixel would keep five lanes of 64 busy.  Otherwise every wave does its own pixel with 64 lanes.  The estimate
// only chooses the mapping; either mapping serves any window.  A pixel's W lanes find its window [i0, i1) together (obs_windows), its
// points are dealt to them round-robin from i0, each lane adds its own in ascending order, and a butterfly over the W lanes (offsets
// W/2 ... 1) adds the partials: the order of the sums follows from the arrays alone, not from the launch or the device.
//
// Whatever the arrays hold (NaN, unordered values, sigma <= 0): a search reads only indices inside its bracket [lo, hi) within [0, n)
// and shrinks the bracket at least W + 1 times per round, a window is [i0, i1) with 0 <= i0 <= i1 <= n, and a lane makes at most
// (i1 - i0) / W + 1 trips.
constexpr int kObsGroup = 8;
constexpr int kObsShort = 32;
constexpr double kCKms = 299792.458;

// One round of a (W + 1)-ary search for the first index in [lo, hi) at which a predicate that holds on a prefix fails: lane t of the
// pixel's W probes p = lo + (t + 1) chunk - 1, chunk = ceil((hi - lo) / (W + 1)).
struct ObsBracket {
    int64_t lo, hi;
};
__device__ __forceinline__ int64_t obs_probe(const ObsBracket& b, int W, int t, int64_t& chunk)
{
    const int64_t len = b.hi - b.lo;
    chunk = W == 64 ? (len + 64) / 65 : (len + 8) / 9;
    const int64_t p = b.lo + (t + 1) * chunk - 1;
    return len > 0 && p < b.hi ? p : -1;  // (-1: nothing to read)
}
// ... c of the W probes held: the index lies behind probe c - 1 and not behind probe c.  The probes that exist are a prefix of the lanes
// and only they can hold, so lo + c chunk <= hi whatever the data; the bracket shrinks to at most chunk - 1 or len / (W + 1) indices.
__device__ __forceinline__ void obs_narrow(ObsBracket& b, int W, int c, int64_t chunk)
{
    if (b.hi <= b.lo) return;
    b.lo += c * chunk;
    const int64_t pc = b.lo + chunk - 1;  // probe c
    if (c < W && pc < b.hi) b.hi = pc;
}
// The window of a pixel, by its W lanes (W = 64: the wave; W = 8: each of the wave's eight segments its own pixel): i0 = the first index
// with x >= lo, i1 = the first with x > hi, searched side by side (one round = one load per lane and bound).  Every lane of the wave
// calls this; a pixel that is not searched (`on` false) reads nothing.  The two bounds may be searched in two arrays of n values (the
// forward kernel passes the grid twice; the adjoint's gather passes its two scans, with D = 1, which rounds nothing).
__device__ __forceinline__ void obs_windows(const double* lam_a, const double* lam_b, int64_t n, double D, double lo, double hi, bool on, int W,
                                            int lane, int64_t& i0, int64_t& i1)
{
    const int t = W == 64 ? lane : lane & 7, shift = W == 64 ? 0 : lane & ~7;
    const unsigned long long seg = W == 64 ? ~0ull : 0xffull;
    ObsBracket a{0, on ? n : 0}, b{0, on ? n : 0};
    while (__any(a.hi > a.lo || b.hi > b.lo)) {
        int64_t ca, cb;
        const int64_t pa = obs_probe(a, W, t, ca), pb = obs_probe(b, W, t, cb);
        const double xa = pa >= 0 ? mul_rn(lam_a[pa], D) : 0.0, xb = pb >= 0 ? mul_rn(lam_b[pb], D) : 0.0;
        const unsigned long long ma = __ballot(pa >= 0 && xa < lo), mb = __ballot(pb >= 0 && xb <= hi);
        obs_narrow(a, W, __popcll((ma >> shift) & seg), ca);
        obs_narrow(b, W, __popcll((mb >> shift) & seg), cb);
    }
    i0 = a.lo;
    i1 = max(a.lo, b.lo);
}

// the Gaussian around x integrated from e0 to e1; s2 = sigma sqrt(2).  Both tails through erfc, which keeps their relative accuracy.
__device__ __forceinline__ double obs_response(double e0, double e1, double x, double s2)
{
    const double a = sub_rn(e0, x) / s2, b = sub_rn(e1, x) / s2;
    const bool above = a > 0.0;
    if (above || b < 0.0) {
        const double p = above ? a : -b, q = above ? b : -a;
        return mul_rn(0.5, sub_rn(erfc(p), erfc(q)));
    }
    return mul_rn(0.5, sub_rn(erf(b), erf(a)));
}

// The two partials of obs_response that the instrument's tangent needs, with a' = (e0 - x) / sigma, b' = (e1 - x) / sigma and phi the unit
// normal density:  rx = dr/dx = (phi(a') - phi(b')) / sigma,   rs = dr/d ln sigma = a' phi(a') - b' phi(b').  In the kernel's a = a' / sqrt 2,
// b = b' / sqrt 2:  phi(a') - phi(b') = G / sqrt(2 pi),  G = e^(-a^2) - e^(-b^2).  G cancels for a pixel much narrower than sigma and where
// both edges lie in one tail, so it is formed from the exponential of the NEARER edge (the smaller |.|) and expm1 of -(|a^2 - b^2|),
// a^2 - b^2 = (a - b)(a + b) with a - b from e0 - e1 and a + b from (e0 - x) + (e1 - x): each a difference of neighbours, then one
// division.  rs sqrt(pi) = a e^(-a^2) - b e^(-b^2) = near G + (a - b) e^(-far^2): the product rule over the same two differences.
__device__ __forceinline__ void obs_response_grad(double e0, double e1, double x, double s2, double& rx, double& rs)
{
    const double da = sub_rn(e0, x), db = sub_rn(e1, x);
    const double m = sub_rn(e0, e1) / s2, p = add_rn(da, db) / s2;  // a - b, a + b
    const bool first = p >= 0.0;                                    // |a| <= |b|
    const double near = (first ? da : db) / s2, far = (first ? db : da) / s2;
    const double d = mul_rn(m, p);  // a^2 - b^2: <= 0 where `first`
    const double en = exp(-mul_rn(near, near)), ef = exp(-mul_rn(far, far));
    const double g = mul_rn(en, expm1(first ? d : -d));  // e^(-far^2) - e^(-near^2)
    const double G = first ? -g : g;
    rx = mul_rn(G, kInvSqrtPi) / s2;
    rs = mul_rn(add_rn(mul_rn(near, G), mul_rn(m, ef)), kInvSqrtPi);
}

// The pixel(s) of a wave in k_observe's mapping and the window each searched: what obs_pixel_sums and k_observe_tangent share.
// false: the wave has no pixel and leaves.
struct ObsWindow {
    int64_t pj;  // the lane's pixel (may lie behind n_pix in the last group: nothing is searched, nothing may be written)
    int W, t;    // the pixel's lanes and the lane's index among them
    bool covered;
    double D, e0, e1, s2;
    int64_t i0, i1;
};
__device__ __forceinline__ bool obs_pixel_window(int64_t n, const double* __restrict__ lam, int64_t n_pix, const double* __restrict__ edges,
                                                 const double* __restrict__ sigma, const double* __restrict__ doppler, ObsWindow& q)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t first = wave - wave % kObsGroup;  // the group's first pixel
    if (first >= n_pix) return false;
    const double D = doppler ? *doppler : 1.0;
    const double x_first = mul_rn(lam[0], D), x_last = mul_rn(lam[n - 1], D);

    // the group's mapping, from pixel first + lane / 8 in every lane
    int64_t pj = first + (lane >> 3);
    double e0 = 0.0, e1 = 0.0, s = 0.0;
    if (pj < n_pix) e0 = edges[pj], e1 = edges[pj + 1], s = sigma[pj];
    const double expected = (e1 - e0 + 16.0 * s) * (double)(n - 1) / (x_last - x_first);  // points in the window at the mean spacing
    int W = 8;
    if (__all(!(expected > (double)kObsShort))) {
        if (wave != first) return false;
    } else {
        if (wave >= n_pix) return false;
        pj = wave, W = 64;
        e0 = edges[pj], e1 = edges[pj + 1], s = sigma[pj];
    }
    const int t = W == 64 ? lane : lane & 7;

    const double reach = mul_rn(8.0, s), lo = sub_rn(e0, reach), hi = add_rn(e1, reach), s2 = mul_rn(s, 1.4142135623730951);
    const bool covered = pj < n_pix && lo >= x_first && hi <= x_last;
    int64_t i0, i1;
    obs_windows(lam, lam, n, D, lo, hi, covered, W, lane, i0, i1);
    q = ObsWindow{pj, W, t, covered, D, e0, e1, s2, i0, i1};
    return true;
}
// point i of the window: x = its shifted wavelength, h = its trapezoid weight, -> r, the pixel's response to it (w_ij = r h)
__device__ __forceinline__ double obs_point(int64_t n, const double* __restrict__ lam, int64_t i, const ObsWindow& q, double& x, double& h)
{
    x = mul_rn(lam[i], q.D);
    const double below = mul_rn(lam[i > 0 ? i - 1 : 0], q.D), above = mul_rn(lam[i < n - 1 ? i + 1 : n - 1], q.D);
    h = mul_rn(sub_rn(above, below), 0.5);
    return obs_response(q.e0, q.e1, x, q.s2);
}

// What a wave of k_observe's mapping sums for its pixel(s): num = sum_i w_ij flux[i] (flux = nullptr: not formed) and den = sum_i w_ij g_i
// over the window, closed by the butterfly, in every lane of the pixel.  false: the wave has no pixel and leaves.
struct ObsPixel {
    int64_t pj;  // the lane's pixel (may lie behind n_pix in the last group: nothing is searched, nothing may be written)
    int t;       // the lane's index among the pixel's W lanes
    bool covered;
    double num, den;
};
__device__ __forceinline__ bool obs_pixel_sums(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                               const double* __restrict__ ref, int64_t n_pix, const double* __restrict__ edges,
                                               const double* __restrict__ sigma, const double* __restrict__ doppler, ObsPixel& p)
{
    ObsWindow q;
    if (!obs_pixel_window(n, lam, n_pix, edges, sigma, doppler, q)) return false;
    double num = 0.0, den = 0.0;
    for (int64_t i = q.i0 + q.t; i < q.i1; i += q.W) {
        double x, h;
        const double r = obs_point(n, lam, i, q, x, h);
        const double w = mul_rn(r, h);
        if (flux) num = add_rn(num, mul_rn(w, flux[i]));
        den = add_rn(den, ref ? mul_rn(w, ref[i]) : w);
    }
    for (int off = q.W >> 1; off > 0; off >>= 1) num = add_rn(num, __shfl_xor(num, off)), den = add_rn(den, __shfl_xor(den, off));
    p = ObsPixel{q.pj, q.t, q.covered, num, den};
    return true;
}

__global__ __launch_bounds__(kBlock) void k_observe(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                                    const double* __restrict__ ref, int64_t n_pix, const double* __restrict__ edges,
                                                    const double* __restrict__ sigma, const double* __restrict__ doppler,
                                                    double* __restrict__ out)
{
    ObsPixel p;
    if (!obs_pixel_sums(n, lam, flux, ref, n_pix, edges, sigma, doppler, p)) return;
    if (p.t == 0 && p.pj < n_pix) out[p.pj] = p.covered ? p.num / p.den : __longlong_as_double(0x7ff8000000000000LL);
}

// ------------------------------------------------------------------------------------------------
// The tangent of the instrument model (include/stardis_hip.h, sdx_observe_tangent_dev): k_observe's pass over k_observe's windows
// (obs_pixel_window, obs_point: the same mapping, search, covered, weights and order of the sums, so `out` is k_observe's bit for bit),
// which also forms, per pixel, with w_ij = r_ij h_i,
//     d w / d ln D     = (x_i dr/dx + r) h_i       (h_i scales with D),        d w / d ln sigma_j = (dr/d ln sigma) h_i      (obs_response_grad),
//     dout_p = (sum_i d_p w_ij flux_i - out_j sum_i d_p w_ij g_i) / den_j      for p = ln D and p = ln sigma,
//     dout_velocity = dout_lnD (D^2 + 1)^2 / (4 D^2 c)  per km/s  (d ln D / dv of D = sqrt((1 + beta) / (1 - beta)), from the D in device memory),
//     dout_flux = (sum_i w_ij dflux_i - out_j sum_i w_ij dref_i) / den_j        (the tangent of the quotient; dref = nullptr: no second term).
// The windows and `covered` are FIXED: a point entering a window brings 1e-15 of the sum.  An uncovered pixel is NaN in every output.  The
// parameter sums are formed only where dout_velocity or dout_lsf is asked for, the tangent sums only with dflux.  No floating-point
// atomics; a butterfly closes every sum.
//
// Whatever the arrays hold (NaN, unordered values, sigma <= 0): the search and the loop are k_observe's own — indices inside a bracket
// within [0, n), a window [i0, i1) with 0 <= i0 <= i1 <= n, at most (i1 - i0) / W + 1 trips per lane — and the loop reads lam at i - 1, i,
// i + 1 clamped to [0, n) and flux, ref, dflux, dref at i alone; a lane writes only at its own pixel pj < n_pix.
__global__ __launch_bounds__(kBlock) void k_observe_tangent(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                                            const double* __restrict__ ref, int64_t n_pix, const double* __restrict__ edges,
                                                            const double* __restrict__ sigma, const double* __restrict__ doppler,
                                                            const double* __restrict__ dflux, const double* __restrict__ dref,
                                                            double* __restrict__ out, double* __restrict__ dout_v, double* __restrict__ dout_s,
                                                            double* __restrict__ dout_f)
{
    ObsWindow q;
    if (!obs_pixel_window(n, lam, n_pix, edges, sigma, doppler, q)) return;
    const bool params = dout_v != nullptr || dout_s != nullptr;
    double num = 0.0, den = 0.0, nD = 0.0, dD = 0.0, nS = 0.0, dS = 0.0, tF = 0.0, tG = 0.0;
    for (int64_t i = q.i0 + q.t; i < q.i1; i += q.W) {
        double x, h;
        const double r = obs_point(n, lam, i, q, x, h);
        const double w = mul_rn(r, h), f = flux[i], g = ref ? ref[i] : 1.0;
        num = add_rn(num, mul_rn(w, f));
        den = add_rn(den, ref ? mul_rn(w, g) : w);
        if (params) {
            double rx, rs;
            obs_response_grad(q.e0, q.e1, x, q.s2, rx, rs);
            const double wD = mul_rn(add_rn(mul_rn(x, rx), r), h), wS = mul_rn(rs, h);
            nD = add_rn(nD, mul_rn(wD, f)), dD = add_rn(dD, ref ? mul_rn(wD, g) : wD);
            nS = add_rn(nS, mul_rn(wS, f)), dS = add_rn(dS, ref ? mul_rn(wS, g) : wS);
        }
        if (dflux) tF = add_rn(tF, mul_rn(w, dflux[i]));
        if (dref) tG = add_rn(tG, mul_rn(w, dref[i]));
    }
    for (int off = q.W >> 1; off > 0; off >>= 1) {
        num = add_rn(num, __shfl_xor(num, off)), den = add_rn(den, __shfl_xor(den, off));
        if (params) {
            nD = add_rn(nD, __shfl_xor(nD, off)), dD = add_rn(dD, __shfl_xor(dD, off));
            nS = add_rn(nS, __shfl_xor(nS, off)), dS = add_rn(dS, __shfl_xor(dS, off));
        }
        if (dflux) tF = add_rn(tF, __shfl_xor(tF, off));
        if (dref) tG = add_rn(tG, __shfl_xor(tG, off));
    }
    if (q.t != 0 || q.pj >= n_pix) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double o = num / den;
    if (out) out[q.pj] = q.covered ? o : nan;
    if (dout_v) {
        const double D2 = mul_rn(q.D, q.D), up = add_rn(D2, 1.0);
        const double per_kms = mul_rn(up, up) / mul_rn(mul_rn(4.0, D2), kCKms);  // d ln D / dv
        dout_v[q.pj] = q.covered ? mul_rn(sub_rn(nD, mul_rn(o, dD)) / den, per_kms) : nan;
    }
    if (dout_s) dout_s[q.pj] = q.covered ? sub_rn(nS, mul_rn(o, dS)) / den : nan;
    if (dout_f) dout_f[q.pj] = q.covered ? (dref ? sub_rn(tF, mul_rn(o, tG)) : tF) / den : nan;
}

// obs_response and obs_response_grad element-wise, as k_observe_tangent's loop calls them (s2 = sigma sqrt 2 rounded as there):
// r, dr/dx and dr/d ln sigma per point (tests/test_gpu_observe_tangent.py judges them point by point)
__global__ __launch_bounds__(kBlock) void k_observe_response_grad(int64_t n, const double* __restrict__ e0, const double* __restrict__ e1,
                                                                  const double* __restrict__ x, const double* __restrict__ sigma,
                                                                  double* __restrict__ out_r, double* __restrict__ out_rx,
                                                                  double* __restrict__ out_rs)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double s2 = mul_rn(sigma[i], 1.4142135623730951);
    double rx, rs;
    obs_response_grad(e0[i], e1[i], x[i], s2, rx, rs);
    out_r[i] = obs_response(e0[i], e1[i], x[i], s2);
    out_rx[i] = rx;
    out_rs[i] = rs;
}

// ------------------------------------------------------------------------------------------------
// The adjoint of the instrument model (include/stardis_hip.h, sdx_observe_adjoint_dev): a vector c over the pixels pulled back to the
// grid points,
//     a_j = covered_j ? c_j / den_j : 0,   b_j = -out_j a_j,
//     w_flux[i] = sum over the covered j with lo_j <= x_i <= hi_j of  w_ij a_j,     w_ref[i] = the same sum of  w_ij b_j,
// w_ij = r_ij h_i the weight of k_observe's loop, bit for bit.  Four launches:
//   k_observe_adjoint_pixels  k_observe's own mapping and sums (obs_pixel_sums) -> a, and b with a reference;
//   k_observe_adjoint_tiles,  PH_j = max_{j' <= j} hi_j' and SL_j = min_{j' >= j} lo_j', in tiles of kObsScanTile pixels: the tiles'
//   k_observe_adjoint_scan    own max and min first, then every tile scans itself behind those of the tiles before it (one block
//                             walking 1e5 pixels took three times the forward kernel's time: EXPERIMENTS).  sigma is per pixel, so
//                             lo and hi need not ascend with j and the pixels that hold a point need not be consecutive; PH and SL do
//                             ascend, max and min round nothing, and PH_j >= hi_j, SL_j <= lo_j: every pixel that holds x lies in
//                             [jA, jB), jA = the first j with PH_j >= x, jB = one past the last with SL_j <= x;
//   k_observe_adjoint         the gather: W lanes per grid point, the points in groups of kObsGroup.  A group none of whose points is
//                             expected to lie in more than kObsShort pixels — 1 + 16 sigma / (the MEAN pixel width), sigma that of the
//                             pixel the point would fall in were all pixels of the mean width: an estimate, taken before anything is
//                             searched — is done by its FIRST wave, eight lanes per point (the forward kernel's reasoning: an
//                             instrument sampled at two pixels per FWHM has a point in ~15 pixels, and a wave per point would keep 15
//                             lanes of 64 busy); otherwise every wave does its own point with 64 lanes.  The estimate only chooses
//                             the mapping; either serves any point.  The point's lanes search jA and jB together (obs_windows on PH
//                             and SL), the candidates are dealt to them round-robin from jA, each is tested with the forward's own
//                             predicate (covered_j && lo_j <= x_i <= hi_j, the same roundings), each lane adds its terms in
//                             ascending j and a butterfly over the W lanes (offsets W/2 ... 1) adds the partials.
// No floating-point atomics; the order of every sum follows from the arrays alone.  A point in no covered window is exactly 0.
//
// Whatever the arrays hold (NaN, unordered values, sigma <= 0): the per-pixel pass has k_observe's bounds; a scan thread reads its own
// pixel, if that lies inside [0, n_pix), and the partials of the n_tiles = ceil(n_pix / kObsScanTile) tiles; the searches read PH and
// SL only inside their brackets within [0, n_pix) and shrink them at least W + 1 times per round, so 0 <= jA <= jB <= n_pix; a lane
// makes at most (jB - jA) / W + 1 trips and reads edges[j], edges[j + 1], sigma[j], a[j], b[j] for jA <= j < jB alone; the estimate's
// pixel index is clamped to [0, n_pix) (a NaN compares false and gives 0).
constexpr int kObsScanTile = kBlock;  // positions per block of the two scan launches: one per thread

__global__ __launch_bounds__(kBlock) void k_observe_adjoint_pixels(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                                                   const double* __restrict__ ref, int64_t n_pix,
                                                                   const double* __restrict__ edges, const double* __restrict__ sigma,
                                                                   const double* __restrict__ doppler, const double* __restrict__ c,
                                                                   double* __restrict__ a, double* __restrict__ b)
{
    ObsPixel p;
    if (!obs_pixel_sums(n, lam, ref ? flux : nullptr, ref, n_pix, edges, sigma, doppler, p)) return;
    if (p.t != 0 || p.pj >= n_pix) return;
    const double aj = p.covered ? c[p.pj] / p.den : 0.0;  // (c of an uncovered pixel is never used)
    a[p.pj] = aj;
    if (ref) b[p.pj] = p.covered ? mul_rn(-(p.num / p.den), aj) : 0.0;
}

// One scan position: position p of direction `up` is pixel p and carries hi_p; of the other, pixel n_pix - 1 - p and lo of that pixel.
// A position behind the last pixel carries the identity of the direction's max or min.
struct ObsScan {
    bool up;
    __device__ __forceinline__ double none() const { return __longlong_as_double(up ? 0xfff0000000000000LL : 0x7ff0000000000000LL); }
    __device__ __forceinline__ double pick(double r, double v) const { return up ? (v > r ? v : r) : (v < r ? v : r); }
    __device__ __forceinline__ double value(int64_t p, int64_t n_pix, const double* __restrict__ edges, const double* __restrict__ sigma) const
    {
        if (p >= n_pix) return none();
        const int64_t j = up ? p : n_pix - 1 - p;
        const double reach = mul_rn(8.0, sigma[j]);
        return up ? add_rn(edges[j + 1], reach) : sub_rn(edges[j], reach);
    }
    // the block's max or min, in every thread (lds: one double per wave; max and min round nothing, so the order is free)
    __device__ __forceinline__ double block(double v, double* lds) const
    {
        for (int off = 32; off > 0; off >>= 1) v = pick(v, __shfl_xor(v, off));
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        double r = lds[0];
        for (int w = 1; w < kBlock / 64; ++w) r = pick(r, lds[w]);
        __syncthreads();
        return r;
    }
};

// tiles[dir n_tiles + k]: the max of hi (dir 0) or the min of lo (dir 1) over the kObsScanTile positions of tile k
__global__ __launch_bounds__(kBlock) void k_observe_adjoint_tiles(int64_t n_pix, const double* __restrict__ edges, const double* __restrict__ sigma,
                                                                  int64_t n_tiles, double* __restrict__ tiles)
{
    __shared__ double lds[kBlock / 64];
    const ObsScan sc{blockIdx.y == 0};
    const double r = sc.block(sc.value((int64_t)blockIdx.x * kObsScanTile + threadIdx.x, n_pix, edges, sigma), lds);
    if (threadIdx.x == 0) tiles[blockIdx.y * n_tiles + blockIdx.x] = r;
}

// PH (blockIdx.y = 0) and SL (1): a block takes the partials of the tiles before its own, then scans its own tile (within the wave by
// shuffles, the waves before it through LDS)
__global__ __launch_bounds__(kBlock) void k_observe_adjoint_scan(int64_t n_pix, const double* __restrict__ edges, const double* __restrict__ sigma,
                                                                 int64_t n_tiles, const double* __restrict__ tiles, double* __restrict__ PH,
                                                                 double* __restrict__ SL)
{
    __shared__ double lds[kBlock / 64], totals[kBlock / 64];
    const ObsScan sc{blockIdx.y == 0};
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double carry = sc.none();
    for (int64_t k = t; k < (int64_t)blockIdx.x; k += kBlock) carry = sc.pick(carry, tiles[blockIdx.y * n_tiles + k]);
    carry = sc.block(carry, lds);
    const int64_t p = (int64_t)blockIdx.x * kObsScanTile + t;
    double v = sc.value(p, n_pix, edges, sigma);
    for (int off = 1; off < 64; off <<= 1) {
        const double before = __shfl_up(v, off);
        if (lane >= off) v = sc.pick(v, before);
    }
    if (lane == 63) totals[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) carry = sc.pick(carry, totals[w]);
    if (p < n_pix) (sc.up ? PH : SL)[sc.up ? p : n_pix - 1 - p] = sc.pick(carry, v);
}

__global__ __launch_bounds__(kBlock) void k_observe_adjoint(int64_t n, const double* __restrict__ lam, int64_t n_pix,
                                                            const double* __restrict__ edges, const double* __restrict__ sigma,
                                                            const double* __restrict__ doppler, const double* __restrict__ a,
                                                            const double* __restrict__ b, const double* __restrict__ PH,
                                                            const double* __restrict__ SL, const double* __restrict__ nus,
                                                            double* __restrict__ w_flux, double* __restrict__ w_ref)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t first = wave - wave % kObsGroup;  // the group's first point
    if (first >= n) return;
    const double D = doppler ? *doppler : 1.0;
    const double x_first = mul_rn(lam[0], D), x_last = mul_rn(lam[n - 1], D);

    // the group's mapping, from point first + lane / 8 in every lane
    int64_t pi = first + (lane >> 3);
    const double e_first = edges[0], width = (edges[n_pix] - e_first) / (double)n_pix;  // the mean pixel width
    double expected = 0.0;
    if (pi < n) {
        const double q = (mul_rn(lam[pi], D) - e_first) / width;
        const int64_t jq = q > 0.0 ? (q < (double)n_pix ? (int64_t)q : n_pix - 1) : 0;
        expected = (width + 16.0 * sigma[jq]) / width;  // pixels that hold the point
    }
    int W = 8;
    if (__all(!(expected > (double)kObsShort))) {
        if (wave != first) return;
    } else {
        if (wave >= n) return;
        pi = wave, W = 64;
    }
    const int t = W == 64 ? lane : lane & 7;
    const bool on = pi < n;
    const int64_t i = on ? pi : n - 1;

    const double x = mul_rn(lam[i], D);
    const double below = mul_rn(lam[i > 0 ? i - 1 : 0], D), above = mul_rn(lam[i < n - 1 ? i + 1 : n - 1], D);
    const double h = mul_rn(sub_rn(above, below), 0.5);
    int64_t jA, jB;
    obs_windows(PH, SL, n_pix, 1.0, x, x, on, W, lane, jA, jB);

    double wf = 0.0, wr = 0.0;
    for (int64_t j = jA + t; j < jB; j += W) {
        const double e0 = edges[j], e1 = edges[j + 1], s = sigma[j];
        const double reach = mul_rn(8.0, s), lo = sub_rn(e0, reach), hi = add_rn(e1, reach);
        if (!(lo >= x_first && hi <= x_last && lo <= x && x <= hi)) continue;
        const double w = mul_rn(obs_response(e0, e1, x, mul_rn(s, 1.4142135623730951)), h);
        wf = add_rn(wf, mul_rn(w, a[j]));
        if (b) wr = add_rn(wr, mul_rn(w, b[j]));
    }
    for (int off = W >> 1; off > 0; off >>= 1) wf = add_rn(wf, __shfl_xor(wf, off)), wr = add_rn(wr, __shfl_xor(wr, off));
    if (t != 0 || !on) return;
    // (the transpose of k_flux_nu_to_lambda, F_lambda = F_nu nu / lambda: the weights of F_lambda become weights of F_nu)
    w_flux[i] = nus ? mul_rn(wf, nus[i]) / lam[i] : wf;
    if (w_ref) w_ref[i] = nus ? mul_rn(wr, nus[i]) / lam[i] : wr;
}

// ------------------------------------------------------------------------------------------------
// Rotational broadening (include/stardis_hip.h, sdx_rotate_dev): Gray's profile for v sin i = V and linear limb darkening eps, in
// velocity space on any ascending grid, applied on the rest-frame grid in front of k_observe.  With beta = V / c, for point i
//     reach_i = lam_i beta,  lo_i = lam_i - reach_i,  hi_i = lam_i + reach_i,  y_ij = (lam_j - lam_i) / reach_i,  q_ij = 1 - y_ij^2,
//     j is included iff (lo_i <= lam_j <= hi_i and q_ij > 0) or j = i (q = 1),
//     K_ij = 2 (1 - eps) sqrt(q_ij) + (pi / 2) eps q_ij,   h_j = the trapezoid weight of lam_j (k_observe's, D = 1),   w_ij = K_ij h_j,
//     out_i = (sum_j w_ij flux_j) / (sum_j w_ij)   over the included j: a window that reaches past an end of the grid sums what exists.
// !(V > 0) copies.  rot_weight is the ONE place where reach, y, q, K and w are rounded and a pair is included or not: the forward
// kernel, the adjoint's denominators and the adjoint's gather call it, so all three hold the same weights bit for bit.
// k_rotate_tangent is the forward kernel's body with a compile-time flag (rotate_body<true>): rot_weight also hands out dw_ij = d w_ij /
// d eps = (-2 sqrt(q_ij) + (pi / 2) q_ij) h_j, and dout_i = (sum_j dw_ij flux_j - out_i sum_j dw_ij) / den_i from the same pass.  This
// sampled sum has no d / dV (dK / d ln V = y^2 (2 (1 - eps) / sqrt(q) + pi eps), and the sum has a square-root kink in V wherever a point
// enters a window); the cell-integrated profile below (k_rotate_integrated, sdx_rotate_integrated_dev) has a bounded one.
//
// k_observe's mapping: points in groups of kObsGroup, eight lanes per point where no point of the group expects more than kObsShort
// points in its window at the grid's MEAN spacing (2 beta lam_i (n - 1) / (lam_{n-1} - lam_0)), a wave per point otherwise; either
// serves any point.  The lanes search the window together (obs_windows, D = 1), take it round-robin, add in ascending j, and a
// butterfly closes the sums.
//
// The adjoint, for weights u over the broadened points: a_i = u_i / den_i (k_rotate_adjoint_den, rot_point_sums as the forward runs it),
// then w_j = sum over the i that include j of w_ij a_i (k_rotate_adjoint).  The i that can include j have lam_i within
// [lam_j / (1 + beta), lam_j / (1 - beta)]; that range is searched a few 1e-15 wide (beta >= 1: no upper bound) and every candidate is
// tested by rot_weight.  No floating-point atomics; the order of every sum follows from the arrays alone.
//
// Whatever the arrays hold (NaN, unordered values, any V and eps): a search reads only inside its bracket within [0, n) and shrinks it
// at least W + 1 times per round, a window is [i0, i1) with 0 <= i0 <= i1 <= n, a lane makes at most (i1 - i0) / W + 1 trips and reads
// lam, flux, ref or a at j - 1, j, j + 1 clamped to [0, n) alone.
constexpr double kHalfPi = 1.5707963267948966;

struct RotProfile {
    double beta, c_sqrt, c_q;  // V / c, 2 (1 - eps), (pi / 2) eps
    bool on;                   // V > 0
};
__device__ __forceinline__ RotProfile rot_profile(const double* __restrict__ rot)
{
    const double V = rot[0], eps = rot[1];
    return RotProfile{V / kCKms, mul_rn(2.0, sub_rn(1.0, eps)), mul_rn(kHalfPi, eps), V > 0.0};
}
// point i's weight for point j (self: j == i), h = the trapezoid weight of j; false: i does not include j.  dw (nullptr: not formed): d w /
// d eps = (-2 sqrt(q) + (pi / 2) q) h from the same sqrt(q) and q (K is linear in eps; bounded, unlike dK / dV with its 1 / sqrt(q))
__device__ __forceinline__ bool rot_weight(const RotProfile& r, double lam_i, double lam_j, bool self, double h, double& w, double* dw = nullptr)
{
    double q = 1.0;
    if (!self) {
        const double reach = mul_rn(lam_i, r.beta), lo = sub_rn(lam_i, reach), hi = add_rn(lam_i, reach);
        const double y = sub_rn(lam_j, lam_i) / reach;
        q = sub_rn(1.0, mul_rn(y, y));
        if (!(lo <= lam_j && lam_j <= hi && q > 0.0)) return false;
    }
    const double root = __dsqrt_rn(q);
    w = mul_rn(add_rn(mul_rn(r.c_sqrt, root), mul_rn(r.c_q, q)), h);
    if (dw) *dw = mul_rn(add_rn(mul_rn(-2.0, root), mul_rn(kHalfPi, q)), h);
    return true;
}
__device__ __forceinline__ double rot_trapezoid(const double* __restrict__ lam, int64_t n, int64_t j)
{
    return mul_rn(sub_rn(lam[j < n - 1 ? j + 1 : n - 1], lam[j > 0 ? j - 1 : 0]), 0.5);
}

// The mapping of the three kernels: the lane's point, its index among the point's W lanes.  false: the wave has no point and leaves.
struct RotLane {
    int64_t pi;  // the lane's point (may lie behind n in the last group: nothing is searched, nothing may be written)
    int W, t, lane;
    bool on;  // pi < n
};
// width: the window's whole width over lam_i (rotation: 2 beta; macroturbulence: 2 (6 beta)); on: the stage broadens at all
__device__ __forceinline__ bool rot_mapping(int64_t n, const double* __restrict__ lam, double width, bool on, RotLane& m)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t first = wave - wave % kObsGroup;  // the group's first point
    if (first >= n) return false;
    int64_t pi = first + (lane >> 3);
    double expected = 0.0;
    if (on && pi < n) expected = width * lam[pi] * (double)(n - 1) / (lam[n - 1] - lam[0]);  // points in the window at the mean spacing
    int W = 8;
    if (__all(!(expected > (double)kObsShort))) {
        if (wave != first) return false;
    } else {
        if (wave >= n) return false;
        pi = wave, W = 64;
    }
    m = RotLane{pi, W, W == 64 ? lane : lane & 7, lane, pi < n};
    return true;
}

// The range of lam_i whose window of relative reach b can hold lam_j: [lam_j / (1 + b), lam_j / (1 - b)], a few 1e-15 wide (b >= 1: no
// upper bound).  What the adjoints' gathers search; the stage's weight function then tests every candidate.
__device__ __forceinline__ void rot_candidates(double lj, double b, double& lo, double& hi)
{
    lo = mul_rn(lj / add_rn(1.0, b), 1.0 - 0x1p-48);
    hi = b < 1.0 ? mul_rn(lj / sub_rn(1.0, b), 1.0 + 0x1p-48) : __longlong_as_double(0x7ff0000000000000LL);
}

// What the point's lanes sum: num = sum_j w_ij flux[j], numr = sum_j w_ij ref[j] (nullptr: not formed), den = sum_j w_ij, closed by the
// butterfly, in every lane of the point; with dsums (three doubles; nullptr: not formed) the same three sums of dw_ij = d w_ij / d eps.
// Not called where !(V > 0).
__device__ __forceinline__ void rot_point_sums(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                               const double* __restrict__ ref, const RotProfile& r, const RotLane& m, double& num, double& numr,
                                               double& den, double* dsums = nullptr)
{
    const int64_t i = m.on ? m.pi : n - 1;
    const double li = lam[i];
    const double reach = mul_rn(li, r.beta);
    int64_t i0, i1;
    obs_windows(lam, lam, n, 1.0, sub_rn(li, reach), add_rn(li, reach), m.on, m.W, m.lane, i0, i1);
    num = 0.0, numr = 0.0, den = 0.0;
    double dnum = 0.0, dnumr = 0.0, dden = 0.0;
    for (int64_t j = i0 + m.t; j < i1; j += m.W) {
        double w, dw;
        if (!rot_weight(r, li, lam[j], j == i, rot_trapezoid(lam, n, j), w, dsums ? &dw : nullptr)) continue;
        if (flux) num = add_rn(num, mul_rn(w, flux[j]));
        if (ref) numr = add_rn(numr, mul_rn(w, ref[j]));
        den = add_rn(den, w);
        if (dsums) {
            if (flux) dnum = add_rn(dnum, mul_rn(dw, flux[j]));
            if (ref) dnumr = add_rn(dnumr, mul_rn(dw, ref[j]));
            dden = add_rn(dden, dw);
        }
    }
    for (int off = m.W >> 1; off > 0; off >>= 1)
        num = add_rn(num, __shfl_xor(num, off)), numr = add_rn(numr, __shfl_xor(numr, off)), den = add_rn(den, __shfl_xor(den, off));
    if (dsums) {
        for (int off = m.W >> 1; off > 0; off >>= 1)
            dnum = add_rn(dnum, __shfl_xor(dnum, off)), dnumr = add_rn(dnumr, __shfl_xor(dnumr, off)), dden = add_rn(dden, __shfl_xor(dden, off));
        dsums[0] = dnum, dsums[1] = dnumr, dsums[2] = dden;
    }
}

// k_rotate (kDeriv false: dout, dout_ref unused) and k_rotate_tangent (kDeriv true): with the derivative,
//     dout_i = (sum_j dw_ij flux_j - out_i sum_j dw_ij) / den_i = d out_i / d eps   (the windows do not depend on eps: exact),
// dout_ref likewise with ref and out_ref (nullptr: not written); !(V > 0): a copy, and zeros
template <bool kDeriv>
__device__ __forceinline__ void rotate_body(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                            const double* __restrict__ ref, const double* __restrict__ rot, double* __restrict__ out,
                                            double* __restrict__ out_ref, double* __restrict__ dout, double* __restrict__ dout_ref)
{
    const RotProfile r = rot_profile(rot);
    RotLane m;
    if (!rot_mapping(n, lam, 2.0 * r.beta, r.on, m)) return;
    if (!r.on) {  // (the group's first wave, eight lanes per point: a copy)
        if (m.t == 0 && m.on) {
            out[m.pi] = flux[m.pi];
            if (ref) out_ref[m.pi] = ref[m.pi];
            if (kDeriv) {
                dout[m.pi] = 0.0;
                if (dout_ref) dout_ref[m.pi] = 0.0;
            }
        }
        return;
    }
    double num, numr, den, d[3];
    rot_point_sums(n, lam, flux, ref, r, m, num, numr, den, kDeriv ? d : nullptr);
    if (m.t != 0 || !m.on) return;
    const double dnum = d[0], dnumr = d[1], dden = d[2];
    const double o = num / den;
    out[m.pi] = o;
    if (kDeriv) dout[m.pi] = sub_rn(dnum, mul_rn(o, dden)) / den;
    if (ref) {
        const double g = numr / den;
        out_ref[m.pi] = g;
        if (kDeriv && dout_ref) dout_ref[m.pi] = sub_rn(dnumr, mul_rn(g, dden)) / den;
    }
}
__global__ __launch_bounds__(kBlock) void k_rotate(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                                   const double* __restrict__ ref, const double* __restrict__ rot, double* __restrict__ out,
                                                   double* __restrict__ out_ref)
{
    rotate_body<false>(n, lam, flux, ref, rot, out, out_ref, nullptr, nullptr);
}
__global__ __launch_bounds__(kBlock) void k_rotate_tangent(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                                           const double* __restrict__ ref, const double* __restrict__ rot,
                                                           double* __restrict__ out, double* __restrict__ out_ref, double* __restrict__ dout,
                                                           double* __restrict__ dout_ref)
{
    rotate_body<true>(n, lam, flux, ref, rot, out, out_ref, dout, dout_ref);
}

// What a broadening stage provides to get its adjoint (stage_adjoint_den, stage_adjoint): a struct of static functions,
//     load(p): its profile from the device scalar(s), with .on (false: the stage copies);   width(r): the window's whole width over lam_i,
//     den(n, lam, r, m): den_i, through the stage's own *_point_sums, as the forward kernel runs it,
//     node(n, lam, j): what node j's weights share (formed once per node, not per candidate),
//     candidates(r, nd, lj, lo, hi): the range of lam_i that can include node j, a few 1e-15 wide,
//     weight(r, nd, n, i, j, lam_i, lj, w): point i's weight for node j; false: i does not include j.
struct RotSampledStage {
    struct Node {
        double h;  // the trapezoid weight of lam_j
    };
    static __device__ __forceinline__ RotProfile load(const double* __restrict__ rot) { return rot_profile(rot); }
    static __device__ __forceinline__ double width(const RotProfile& r) { return 2.0 * r.beta; }
    static __device__ __forceinline__ double den(int64_t n, const double* __restrict__ lam, const RotProfile& r, const RotLane& m)
    {
        double num, numr, den;
        rot_point_sums(n, lam, nullptr, nullptr, r, m, num, numr, den);
        return den;
    }
    static __device__ __forceinline__ Node node(int64_t n, const double* __restrict__ lam, int64_t j) { return Node{rot_trapezoid(lam, n, j)}; }
    // lam_i in [lam_j / (1 + beta), lam_j / (1 - beta)]; rot_weight decides
    static __device__ __forceinline__ void candidates(const RotProfile& r, const Node&, double lj, double& lo, double& hi)
    {
        rot_candidates(lj, r.beta, lo, hi);
    }
    static __device__ __forceinline__ bool weight(const RotProfile& r, const Node& nd, int64_t, int64_t i, int64_t j, double lam_i, double lj, double& w)
    {
        return rot_weight(r, lam_i, lj, i == j, nd.h, w);
    }
};

// The first launch of a stage's adjoint: a[i] = u[i] / den_i, a_ref[i] = u_ref[i] / den_i (u_ref = nullptr: none); a stage that is not
// on: den = 1
template <class Stage, class Profile>
__device__ __forceinline__ void stage_adjoint_den_of(int64_t n, const double* __restrict__ lam, const Profile& r,
                                                     const double* __restrict__ u, const double* __restrict__ u_ref, double* __restrict__ a,
                                                     double* __restrict__ a_ref)
{
    RotLane m;
    if (!rot_mapping(n, lam, Stage::width(r), r.on, m)) return;
    double den = 1.0;
    if (r.on) den = Stage::den(n, lam, r, m);
    if (m.t != 0 || !m.on) return;
    a[m.pi] = r.on ? u[m.pi] / den : u[m.pi];
    if (u_ref) a_ref[m.pi] = r.on ? u_ref[m.pi] / den : u_ref[m.pi];
}
template <class Stage>
__device__ __forceinline__ void stage_adjoint_den(int64_t n, const double* __restrict__ lam, const double* __restrict__ scalars,
                                                  const double* __restrict__ u, const double* __restrict__ u_ref, double* __restrict__ a,
                                                  double* __restrict__ a_ref)
{
    stage_adjoint_den_of<Stage>(n, lam, Stage::load(scalars), u, u_ref, a, a_ref);
}

// The second: w_j = sum over the candidates i that include node j of w_ij a_i, round-robin over the node's lanes in ascending i, closed
// by the butterfly; a stage that is not on copies a.  The accesses and trips are bounded as stated above k_rotate.
// (stage_out: what a stage does to a node's sum before the nu / lambda factor — nothing, but for a disk's ring, which applies its flux
// weight: the overload for DiskRing, declared with it further down, is the one an instantiation with that profile finds.  The *_of forms
// take the stage's profile already loaded — a disk has one per ring —, the forms without load it from the stage's device scalars.)
template <class Profile>
__device__ __forceinline__ double stage_out(const Profile&, double w)
{
    return w;
}
template <class Stage, class Profile>
__device__ __forceinline__ void stage_adjoint_of(int64_t n, const double* __restrict__ lam, const Profile& r,
                                                 const double* __restrict__ a, const double* __restrict__ a_ref, const double* __restrict__ nus,
                                                 double* __restrict__ w_out, double* __restrict__ w_ref)
{
    RotLane m;
    if (!rot_mapping(n, lam, Stage::width(r), r.on, m)) return;
    const int64_t j = m.on ? m.pi : n - 1;
    const double lj = lam[j];
    double wf = 0.0, wr = 0.0;
    if (r.on) {
        const typename Stage::Node nd = Stage::node(n, lam, j);
        double lo, hi;
        Stage::candidates(r, nd, lj, lo, hi);
        int64_t iA, iB;
        obs_windows(lam, lam, n, 1.0, lo, hi, m.on, m.W, m.lane, iA, iB);
        for (int64_t i = iA + m.t; i < iB; i += m.W) {
            double w;
            if (!Stage::weight(r, nd, n, i, j, lam[i], lj, w)) continue;
            wf = add_rn(wf, mul_rn(w, a[i]));
            if (a_ref) wr = add_rn(wr, mul_rn(w, a_ref[i]));
        }
        for (int off = m.W >> 1; off > 0; off >>= 1) wf = add_rn(wf, __shfl_xor(wf, off)), wr = add_rn(wr, __shfl_xor(wr, off));
    } else {
        wf = a[j];
        if (a_ref) wr = a_ref[j];
    }
    if (m.t != 0 || !m.on) return;
    wf = stage_out(r, wf), wr = stage_out(r, wr);
    // (the transpose of k_flux_nu_to_lambda, as k_observe_adjoint ends)
    w_out[j] = nus ? mul_rn(wf, nus[j]) / lj : wf;
    if (w_ref) w_ref[j] = nus ? mul_rn(wr, nus[j]) / lj : wr;
}
template <class Stage>
__device__ __forceinline__ void stage_adjoint(int64_t n, const double* __restrict__ lam, const double* __restrict__ scalars,
                                              const double* __restrict__ a, const double* __restrict__ a_ref, const double* __restrict__ nus,
                                              double* __restrict__ w_out, double* __restrict__ w_ref)
{
    stage_adjoint_of<Stage>(n, lam, Stage::load(scalars), a, a_ref, nus, w_out, w_ref);
}

__global__ __launch_bounds__(kBlock) void k_rotate_adjoint_den(int64_t n, const double* __restrict__ lam, const double* __restrict__ rot,
                                                               const double* __restrict__ u, const double* __restrict__ u_ref,
                                                               double* __restrict__ a, double* __restrict__ a_ref)
{
    stage_adjoint_den<RotSampledStage>(n, lam, rot, u, u_ref, a, a_ref);
}
__global__ __launch_bounds__(kBlock) void k_rotate_adjoint(int64_t n, const double* __restrict__ lam, const double* __restrict__ rot,
                                                           const double* __restrict__ a, const double* __restrict__ a_ref,
                                                           const double* __restrict__ nus, double* __restrict__ w_out,
                                                           double* __restrict__ w_ref)
{
    stage_adjoint<RotSampledStage>(n, lam, rot, a, a_ref, nus, w_out, w_ref);
}

// ------------------------------------------------------------------------------------------------
// The cell-integrated rotation profile (include/stardis_hip.h, sdx_rotate_integrated_dev): the flux is piecewise linear between the grid's
// nodes, as k_observe's trapezoid assumes, and Gray's profile K(y) = c_sqrt sqrt(q) + c_q q, q = 1 - y^2, is integrated against it exactly,
// cell by cell.  A second mode beside k_rotate, which stays what it is.  For point i, reach_i = lam_i beta, and cell g = [j, j + 1]:
//     y_j = (lam_j - lam_i) / reach_i  (y_i = 0),   c = clamp(y, -1, 1),   the cell counts iff c_{j+1} > c_j,
//     Delta = (lam_{j+1} - lam_j) / reach_i: the difference of the neighbours, then one division,
//     d = Delta where neither end is clamped, else c_{j+1} - c_j,
//     M0 = int_{c_j}^{c_{j+1}} K,   M1 = int y K,   r = (M1 - y_j M0) / Delta (node j + 1's share),   M0 - r (node j's),   t = M1 / Delta,
//     out_i = sum_g ((M0 - r) f_j + r f_{j+1}) / den_i,   den_i = sum_g M0   — ascending g, the two products of a cell added in this order,
//     d out_i / d ln V = (sum_g t (f_{j+1} - f_j) + e_0 f_0 - e_1 f_{n-1} - out_i (e_0 - e_1)) / den_i,
//         e_0 = y_0 K(y_0) if y_0 > -1, e_1 = y_{n-1} K(y_{n-1}) if y_{n-1} < 1, else 0: the end terms of a truncated window,
//     d out_i / d eps: the quotient rule over the same sums with K replaced by -2 sqrt(q) + (pi / 2) q.
// The derivative to V is exact, not "at fixed windows": over lambda the domain does not move, K(+-1) = 0 removes the Leibniz terms, and one
// integration by parts leaves int K y phi_j' with phi_j' piecewise constant.
//
// The moments of a cell are NOT differences of antiderivatives: a window of V = 100 km/s holds hundreds of cells, and a difference of
// asin loses what the cell is narrower than 1.  rot_half forms them for 0 <= p < s <= 1 (the other half by symmetry; a cell of a point's
// own row never spans 0, since y_i = 0 is a node) from d = s - p, u = 1 - y, q = u (1 + y), the angles theta = acos y:
//     sin dl = d (s + p) / (s sqrt(q_p) + p sqrt(q_s)),   cos dl = p s + sqrt(q_p q_s),   dl = theta_p - theta_s = atan2(sin dl, cos dl),
//     int sqrt(q)   = ((dl - sin dl) + sin dl (u_p + u_s p + sqrt(q_p q_s))) / 2      (the bracket: 1 - cos(theta_p + theta_s)),
//     int q         = d ((u_p + u_s) - (u_p^2 + u_p u_s + u_s^2) / 3),
//     int y sqrt(q) = d (s + p) (q_p + sqrt(q_p q_s) + q_s) / (3 (sqrt(q_p) + sqrt(q_s))),      int y q = d (s + p) (q_p + q_s) / 4,
// dl - sin dl from its series in dl^2 (twelve terms serve dl <= pi / 2).  Every sum is one of non-negative terms, so each moment keeps its
// relative accuracy for a cell of any width anywhere in [-1, 1].  r's numerator cancels by |y| / d for a narrow cell far from the centre:
// an error of an ulp of den_i per cell, which moves out_i by that times f_{j+1} - f_j.
//
// rot_cell is the ONE place where y, the clamp, the moments, r and t are rounded and a cell counts or not: the forward kernel, the
// adjoint's denominators and the adjoint's gather call it, so all three hold the same weights bit for bit.  Mapping, window search,
// round-robin, ascending order and butterfly are k_rotate's; the cells of point i are those of its window [i0, i1) and the partial cell
// on each side, g in [max(i0 - 1, 0), min(i1, n - 1)).  The adjoint: a_i = u_i / den_i (k_rotate_integrated_adjoint_den), then per node j
// w_j = sum_i (r of cell j - 1 + (M0 - r) of cell j) a_i over the candidates lam_i in [lam_{j-1} / (1 + beta), lam_{j+1} / (1 - beta)],
// searched a few 1e-15 wide; rot_cell decides.  No floating-point atomics.
//
// Whatever the arrays hold (NaN, unordered values, any V and eps): the searches are obs_windows' (inside [0, n), bounded by their
// brackets), a cell index g satisfies 0 <= g < n - 1 so that g + 1 <= n - 1, a lane makes at most (n - 1) / W + 1 trips, the gather reads
// lam at j - 1, j, j + 1 clamped to [0, n) and cells j - 1 >= 0 and j < n - 1 alone, and a point writes only its own element.
struct RotMoments {
    double s0, q0, s1, q1;  // int sqrt(q), int q, int y sqrt(q), int y q over the cell
};
__device__ __forceinline__ void rot_half(double p, double s, double d, RotMoments& m)
{
    const double up = sub_rn(1.0, p), us = sub_rn(1.0, s);
    const double qp = mul_rn(up, add_rn(1.0, p)), qs = mul_rn(us, add_rn(1.0, s));
    const double rp = __dsqrt_rn(qp), rs = __dsqrt_rn(qs), rr = mul_rn(rp, rs);
    const double dsum = mul_rn(d, add_rn(s, p));  // s^2 - p^2 = q_p - q_s
    const double sn = dsum / add_rn(mul_rn(s, rp), mul_rn(p, rs)), cs = add_rn(mul_rn(p, s), rr);
    const double dl = atan2(sn, cs), x = mul_rn(dl, dl);
    // (dl - sin dl) / dl^3 = 1 / 3! - x / 5! + x^2 / 7! - ...
    double h = 1.0 / 15511210043330985984000000.0;  // 25!
    h = sub_rn(1.0 / 25852016738884976640000.0, mul_rn(x, h));
    h = sub_rn(1.0 / 51090942171709440000.0, mul_rn(x, h));
    h = sub_rn(1.0 / 121645100408832000.0, mul_rn(x, h));
    h = sub_rn(1.0 / 355687428096000.0, mul_rn(x, h));
    h = sub_rn(1.0 / 1307674368000.0, mul_rn(x, h));
    h = sub_rn(1.0 / 6227020800.0, mul_rn(x, h));
    h = sub_rn(1.0 / 39916800.0, mul_rn(x, h));
    h = sub_rn(1.0 / 362880.0, mul_rn(x, h));
    h = sub_rn(1.0 / 5040.0, mul_rn(x, h));
    h = sub_rn(1.0 / 120.0, mul_rn(x, h));
    h = sub_rn(1.0 / 6.0, mul_rn(x, h));
    const double dms = mul_rn(mul_rn(dl, x), h);
    const double lift = add_rn(add_rn(up, mul_rn(us, p)), rr);
    m.s0 = mul_rn(0.5, add_rn(dms, mul_rn(sn, lift)));
    m.q0 = mul_rn(d, sub_rn(add_rn(up, us), add_rn(add_rn(mul_rn(up, up), mul_rn(up, us)), mul_rn(us, us)) / 3.0));
    m.s1 = mul_rn(dsum, add_rn(add_rn(qp, rr), qs)) / mul_rn(3.0, add_rn(rp, rs));
    m.q1 = mul_rn(mul_rn(dsum, add_rn(qp, qs)), 0.25);
}
// -1 <= a < b <= 1, d = b - a: what k_rotate_moments evaluates, and rot_cell for a cell in one half (its two first branches).  A cell that
// spans 0 is the sum of its halves for the even moments, and for the odd ones the cell between |a| and |b| with the sign of the longer half.
__device__ __forceinline__ void rot_moments(double a, double b, double d, RotMoments& m)
{
    if (a >= 0.0) {
        rot_half(a, b, d, m);
    } else if (b <= 0.0) {
        rot_half(-b, -a, d, m);
        m.s1 = -m.s1, m.q1 = -m.q1;
    } else {
        RotMoments lo, hi;
        rot_half(0.0, -a, -a, lo);
        rot_half(0.0, b, b, hi);
        m.s0 = add_rn(lo.s0, hi.s0), m.q0 = add_rn(lo.q0, hi.q0), m.s1 = 0.0, m.q1 = 0.0;
        const double na = -a;
        if (na != b) {
            RotMoments odd;
            rot_half(fmin(na, b), fmax(na, b), fabs(add_rn(a, b)), odd);
            m.s1 = b > na ? odd.s1 : -odd.s1, m.q1 = b > na ? odd.q1 : -odd.q1;
        }
    }
}

struct RotCell {
    double m0, r, t;  // int K over the cell, node j + 1's share of it, M1 / Delta
    double dm0, dr;   // d / d eps of m0 and r (kDeriv)
};
// point i's cell [a, b] = [j, j + 1] (self: 0 if a is the point itself, 1 if b is, else -1); false: the cell does not count
template <bool kDeriv>
__device__ __forceinline__ bool rot_cell(const RotProfile& r, double lam_i, double lam_a, double lam_b, int self, RotCell& c)
{
    const double reach = mul_rn(lam_i, r.beta);
    const double ya = self == 0 ? 0.0 : sub_rn(lam_a, lam_i) / reach, yb = self == 1 ? 0.0 : sub_rn(lam_b, lam_i) / reach;
    const double ca = fmin(fmax(ya, -1.0), 1.0), cb = fmin(fmax(yb, -1.0), 1.0);
    if (!(cb > ca)) return false;
    const double delta = sub_rn(lam_b, lam_a) / reach;
    RotMoments m;
    // (y_i = 0 is a node: on an ascending grid a cell of the point's own row lies in one half, and only there is the result meant)
    const double d = ca == ya && cb == yb ? delta : sub_rn(cb, ca);
    if (ca >= 0.0) {
        rot_half(ca, cb, d, m);
    } else {
        rot_half(fmax(-cb, 0.0), -ca, d, m);
        m.s1 = -m.s1, m.q1 = -m.q1;
    }
    const double m1 = add_rn(mul_rn(r.c_sqrt, m.s1), mul_rn(r.c_q, m.q1));
    c.m0 = add_rn(mul_rn(r.c_sqrt, m.s0), mul_rn(r.c_q, m.q0));
    c.r = sub_rn(m1, mul_rn(ya, c.m0)) / delta;
    c.t = m1 / delta;
    if (kDeriv) {
        const double dm1 = add_rn(mul_rn(-2.0, m.s1), mul_rn(kHalfPi, m.q1));
        c.dm0 = add_rn(mul_rn(-2.0, m.s0), mul_rn(kHalfPi, m.q0));
        c.dr = sub_rn(dm1, mul_rn(ya, c.dm0)) / delta;
    }
    return true;
}
// y K(y) at an end of the grid seen from point i, 0 where the window does not reach it (|y| >= 1) or the end is the point itself.  The term
// ends in sqrt(1 - |y|): 1 - |y| = (reach - |lam_end - lam_i|) / reach, the difference first (exact where the end node lies near the
// profile's edge), so that an end node ON the edge does not leave sqrt(a few ulp) = 1e-8 here.
__device__ __forceinline__ double rot_end_term(const RotProfile& r, double lam_i, double lam_end, bool self)
{
    if (self) return 0.0;
    const double reach = mul_rn(lam_i, r.beta), dl = sub_rn(lam_end, lam_i), ay = fabs(dl);
    const double u = sub_rn(reach, ay) / reach;
    if (!(u > 0.0)) return 0.0;
    const double q = mul_rn(u, add_rn(1.0, ay / reach));
    return mul_rn(dl / reach, add_rn(mul_rn(r.c_sqrt, __dsqrt_rn(q)), mul_rn(r.c_q, q)));
}

// What the point's lanes sum over its cells, closed by the butterfly, in every lane of the point: num, numr (flux, ref; nullptr: not
// formed), den and, with kDeriv, t* = sum t (f_{j+1} - f_j) and e* = the three sums of the d / d eps weights.  Not called where !(V > 0).
struct RotIntSums {
    double num, numr, den, tnum, tnumr, enum_, enumr, eden;
};
template <bool kDeriv>
__device__ __forceinline__ void rot_int_point_sums(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                                   const double* __restrict__ ref, const RotProfile& r, const RotLane& m, RotIntSums& s)
{
    const int64_t i = m.on ? m.pi : n - 1;
    const double li = lam[i];
    const double reach = mul_rn(li, r.beta);
    int64_t i0, i1;
    obs_windows(lam, lam, n, 1.0, sub_rn(li, reach), add_rn(li, reach), m.on, m.W, m.lane, i0, i1);
    const int64_t g0 = i0 > 0 ? i0 - 1 : 0, g1 = i1 < n - 1 ? i1 : n - 1;  // the window's cells and the partial cell on each side
    s = RotIntSums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t g = g0 + m.t; g < g1; g += m.W) {
        RotCell c;
        if (!rot_cell<kDeriv>(r, li, lam[g], lam[g + 1], g == i ? 0 : (g + 1 == i ? 1 : -1), c)) continue;
        const double wa = sub_rn(c.m0, c.r);
        s.den = add_rn(s.den, c.m0);
        if (flux) {
            const double fa = flux[g], fb = flux[g + 1];
            s.num = add_rn(add_rn(s.num, mul_rn(wa, fa)), mul_rn(c.r, fb));
            if (kDeriv) {
                s.tnum = add_rn(s.tnum, mul_rn(c.t, sub_rn(fb, fa)));
                s.enum_ = add_rn(add_rn(s.enum_, mul_rn(sub_rn(c.dm0, c.dr), fa)), mul_rn(c.dr, fb));
            }
        }
        if (ref) {
            const double ga = ref[g], gb = ref[g + 1];
            s.numr = add_rn(add_rn(s.numr, mul_rn(wa, ga)), mul_rn(c.r, gb));
            if (kDeriv) {
                s.tnumr = add_rn(s.tnumr, mul_rn(c.t, sub_rn(gb, ga)));
                s.enumr = add_rn(add_rn(s.enumr, mul_rn(sub_rn(c.dm0, c.dr), ga)), mul_rn(c.dr, gb));
            }
        }
        if (kDeriv) s.eden = add_rn(s.eden, c.dm0);
    }
    for (int off = m.W >> 1; off > 0; off >>= 1) {
        s.num = add_rn(s.num, __shfl_xor(s.num, off)), s.numr = add_rn(s.numr, __shfl_xor(s.numr, off));
        s.den = add_rn(s.den, __shfl_xor(s.den, off));
        if (kDeriv) {
            s.tnum = add_rn(s.tnum, __shfl_xor(s.tnum, off)), s.tnumr = add_rn(s.tnumr, __shfl_xor(s.tnumr, off));
            s.enum_ = add_rn(s.enum_, __shfl_xor(s.enum_, off)), s.enumr = add_rn(s.enumr, __shfl_xor(s.enumr, off));
            s.eden = add_rn(s.eden, __shfl_xor(s.eden, off));
        }
    }
}

// out, out_ref as above; with kDeriv dlnv, dlnv_ref, deps, deps_ref (each nullptr: not written).  !(V > 0): a copy, and zeros.
template <bool kDeriv>
__global__ __launch_bounds__(kBlock) void k_rotate_integrated(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                                              const double* __restrict__ ref, const double* __restrict__ rot,
                                                              double* __restrict__ out, double* __restrict__ out_ref,
                                                              double* __restrict__ dlnv, double* __restrict__ dlnv_ref,
                                                              double* __restrict__ deps, double* __restrict__ deps_ref)
{
    const RotProfile r = rot_profile(rot);
    RotLane m;
    if (!rot_mapping(n, lam, 2.0 * r.beta, r.on, m)) return;
    if (!r.on) {  // (the group's first wave, eight lanes per point: a copy)
        if (m.t == 0 && m.on) {
            out[m.pi] = flux[m.pi];
            if (ref) out_ref[m.pi] = ref[m.pi];
            if (kDeriv) {
                if (dlnv) dlnv[m.pi] = 0.0;
                if (dlnv_ref) dlnv_ref[m.pi] = 0.0;
                if (deps) deps[m.pi] = 0.0;
                if (deps_ref) deps_ref[m.pi] = 0.0;
            }
        }
        return;
    }
    RotIntSums s;
    rot_int_point_sums<kDeriv>(n, lam, flux, ref, r, m, s);
    if (m.t != 0 || !m.on) return;
    const double o = s.num / s.den;
    out[m.pi] = o;
    double e0 = 0.0, e1 = 0.0;
    if (kDeriv) {
        const double li = lam[m.pi];
        e0 = rot_end_term(r, li, lam[0], m.pi == 0), e1 = rot_end_term(r, li, lam[n - 1], m.pi == n - 1);
        if (dlnv) {
            const double tf = add_rn(s.tnum, sub_rn(mul_rn(e0, flux[0]), mul_rn(e1, flux[n - 1])));
            dlnv[m.pi] = sub_rn(tf, mul_rn(o, sub_rn(e0, e1))) / s.den;
        }
        if (deps) deps[m.pi] = sub_rn(s.enum_, mul_rn(o, s.eden)) / s.den;
    }
    if (ref) {
        const double g = s.numr / s.den;
        out_ref[m.pi] = g;
        if (kDeriv && dlnv_ref) {
            const double tg = add_rn(s.tnumr, sub_rn(mul_rn(e0, ref[0]), mul_rn(e1, ref[n - 1])));
            dlnv_ref[m.pi] = sub_rn(tg, mul_rn(g, sub_rn(e0, e1))) / s.den;
        }
        if (kDeriv && deps_ref) deps_ref[m.pi] = sub_rn(s.enumr, mul_rn(g, s.eden)) / s.den;
    }
}

// the stage of stage_adjoint_den and stage_adjoint: node j's weight is r of cell j - 1 plus M0 - r of cell j
struct RotIntegratedStage {
    struct Node {
        double below, above;  // lam_{j-1}, lam_{j+1}, clamped to the grid
    };
    static __device__ __forceinline__ RotProfile load(const double* __restrict__ rot) { return rot_profile(rot); }
    static __device__ __forceinline__ double width(const RotProfile& r) { return 2.0 * r.beta; }
    static __device__ __forceinline__ double den(int64_t n, const double* __restrict__ lam, const RotProfile& r, const RotLane& m)
    {
        RotIntSums s;
        rot_int_point_sums<false>(n, lam, nullptr, nullptr, r, m, s);
        return s.den;
    }
    static __device__ __forceinline__ Node node(int64_t n, const double* __restrict__ lam, int64_t j)
    {
        return Node{lam[j > 0 ? j - 1 : 0], lam[j < n - 1 ? j + 1 : n - 1]};
    }
    // lam_i in [lam_{j-1} / (1 + beta), lam_{j+1} / (1 - beta)]; rot_cell decides
    static __device__ __forceinline__ void candidates(const RotProfile& r, const Node& nd, double, double& lo, double& hi)
    {
        double unused;
        rot_candidates(nd.below, r.beta, lo, unused);
        rot_candidates(nd.above, r.beta, unused, hi);
    }
    static __device__ __forceinline__ bool weight(const RotProfile& r, const Node& nd, int64_t n, int64_t i, int64_t j, double lam_i, double lj, double& w)
    {
        RotCell c;
        bool any = false;
        w = 0.0;
        if (j > 0 && rot_cell<false>(r, lam_i, nd.below, lj, j - 1 == i ? 0 : (j == i ? 1 : -1), c)) w = c.r, any = true;
        if (j < n - 1 && rot_cell<false>(r, lam_i, lj, nd.above, j == i ? 0 : (j + 1 == i ? 1 : -1), c)) w = add_rn(w, sub_rn(c.m0, c.r)), any = true;
        return any;
    }
};
__global__ __launch_bounds__(kBlock) void k_rotate_integrated_adjoint_den(int64_t n, const double* __restrict__ lam,
                                                                          const double* __restrict__ rot, const double* __restrict__ u,
                                                                          const double* __restrict__ u_ref, double* __restrict__ a,
                                                                          double* __restrict__ a_ref)
{
    stage_adjoint_den<RotIntegratedStage>(n, lam, rot, u, u_ref, a, a_ref);
}
__global__ __launch_bounds__(kBlock) void k_rotate_integrated_adjoint(int64_t n, const double* __restrict__ lam,
                                                                      const double* __restrict__ rot, const double* __restrict__ a,
                                                                      const double* __restrict__ a_ref, const double* __restrict__ nus,
                                                                      double* __restrict__ w_out, double* __restrict__ w_ref)
{
    stage_adjoint<RotIntegratedStage>(n, lam, rot, a, a_ref, nus, w_out, w_ref);
}

// rot_moments point by point, as rot_cell calls it (d = yb - ya rounded once; the ends clamped to [-1, 1]): M0 = int K, M1 = int y K for
// the limb darkening eps[i]; an empty cell gives zeros (tests/test_gpu_rotation_integrated.py judges them point by point)
__global__ __launch_bounds__(kBlock) void k_rotate_moments(int64_t n, const double* __restrict__ ya, const double* __restrict__ yb,
                                                           const double* __restrict__ eps, double* __restrict__ out_m0,
                                                           double* __restrict__ out_m1)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double a = fmin(fmax(ya[i], -1.0), 1.0), b = fmin(fmax(yb[i], -1.0), 1.0);
    double m0 = 0.0, m1 = 0.0;
    if (b > a) {
        const double c_sqrt = mul_rn(2.0, sub_rn(1.0, eps[i])), c_q = mul_rn(kHalfPi, eps[i]);
        RotMoments m;
        rot_moments(a, b, sub_rn(b, a), m);
        m0 = add_rn(mul_rn(c_sqrt, m.s0), mul_rn(c_q, m.q0));
        m1 = add_rn(mul_rn(c_sqrt, m.s1), mul_rn(c_q, m.q1));
    }
    out_m0[i] = m0;
    out_m1[i] = m1;
}

// ------------------------------------------------------------------------------------------------
// Disk integration with rigid rotation (include/stardis_hip.h, sdx_disk_integrate_dev): the star's disk as rings of constant mu, ring r
// at the projected radius scale_r = sin theta_r with its OWN spectrum I_r (the formal solution's emergent intensity of that angle,
// k_emergent_intensity) instead of one spectrum times a limb-darkening law.  Along a ring the line-of-sight velocity is V scale_r cos phi,
// phi uniform: the ring's average is the convolution of I_r with the arcsine density 1 / (pi sqrt(1 - y^2)) of half-width V scale_r / c.
// As in k_rotate_integrated the spectrum is piecewise linear between the nodes and the density is integrated against it exactly, cell by
// cell: for point i and ring r, beta_r = (V / c) scale_r, reach = lam_i beta_r; !(reach > 0): A_r[i] = I_r[i]; otherwise over the cells
// g = [j, j + 1] of k_rotate's window for that reach and the partial cell on each side, with y, the clamp c, COUNTS, Delta and d as in
// rot_cell,
//     M0 = int_{c_j}^{c_{j+1}} dy / (pi sqrt(1 - y^2)),   M1 = int y dy / (pi sqrt(1 - y^2)),   r = (M1 - y_j M0) / Delta,
//     A_r[i] = sum_g ((M0 - r) I_r[j] + r I_r[j+1]) / sum_g M0     — ascending g, the two products of a cell added in this order,
//     out[i] = sum_r w_r A_r[i]                                    — two ascending halves over r, the lower added to the upper: the flux's order.
// The moments are rot_half's forms (arc_half): for 0 <= p < s <= 1, D = d (s + p), sin = D / (s sqrt(q_p) + p sqrt(q_s)), cos = p s +
// sqrt(q_p) sqrt(q_s), M0 = atan2(sin, cos) / pi, M1 = D / (pi (sqrt(q_p) + sqrt(q_s)))  (sqrt(q_p) - sqrt(q_s) without the cancellation);
// the other half mirrored, a cell that spans 0 split there (arc_moments, as rot_moments).  The density is integrable but unbounded at
// +-1: sampled at the nodes it would need the cell integrals anyway.  A truncated window is renormalised by its own sum of M0.
//
// disk_cell is the ONE place where a ring's cell is rounded and counts or not.  Mapping (rot_mapping, by the widest ring a disk can have,
// scale = 1), window search, round-robin, ascending order and butterfly are k_rotate's; a point's lanes take the rings one after the
// other, every lane holds every A_r after the butterfly and keeps the two half sums itself: no LDS, no floating-point atomics.
// Whatever the arrays hold: whether a ring is searched at all depends on V and scale_r alone (the same in every lane of the wave, as the
// window search needs); a ring that is searched runs obs_windows in every lane, a point whose own reach is not positive with nothing to
// search; a cell index g satisfies 0 <= g < n - 1, a lane makes at most (n - 1) / W + 1 trips per ring, and a point writes only its own
// element.
__device__ __forceinline__ void arc_half(double p, double s, double d, double& m0, double& m1)
{
    const double qp = mul_rn(sub_rn(1.0, p), add_rn(1.0, p)), qs = mul_rn(sub_rn(1.0, s), add_rn(1.0, s));
    const double rp = __dsqrt_rn(qp), rs = __dsqrt_rn(qs);
    const double dsum = mul_rn(d, add_rn(s, p));  // s^2 - p^2 = q_p - q_s
    const double sn = dsum / add_rn(mul_rn(s, rp), mul_rn(p, rs)), cs = add_rn(mul_rn(p, s), mul_rn(rp, rs));
    m0 = atan2(sn, cs) / kPi;
    m1 = dsum / mul_rn(kPi, add_rn(rp, rs));
}
// -1 <= a < b <= 1, d = b - a (rot_moments' cases)
__device__ __forceinline__ void arc_moments(double a, double b, double d, double& m0, double& m1)
{
    if (a >= 0.0) {
        arc_half(a, b, d, m0, m1);
    } else if (b <= 0.0) {
        arc_half(-b, -a, d, m0, m1);
        m1 = -m1;
    } else {
        double l0, l1, h0, h1;
        arc_half(0.0, -a, -a, l0, l1);
        arc_half(0.0, b, b, h0, h1);
        m0 = add_rn(l0, h0), m1 = 0.0;
        const double na = -a;
        if (na != b) {
            double o0, o1;
            arc_half(fmin(na, b), fmax(na, b), fabs(add_rn(a, b)), o0, o1);
            m1 = b > na ? o1 : -o1;
        }
    }
}
// point i's cell [a, b] = [j, j + 1] of a ring of reach `reach` (self as for rot_cell); false: the cell does not count.
// t (nullptr: not formed): M1 / Delta with M1 over the clamped cell, the cell's coefficient in d / d ln V
__device__ __forceinline__ bool disk_cell(double reach, double lam_i, double lam_a, double lam_b, int self, double& m0, double& r,
                                          double* t = nullptr)
{
    const double ya = self == 0 ? 0.0 : sub_rn(lam_a, lam_i) / reach, yb = self == 1 ? 0.0 : sub_rn(lam_b, lam_i) / reach;
    const double ca = fmin(fmax(ya, -1.0), 1.0), cb = fmin(fmax(yb, -1.0), 1.0);
    if (!(cb > ca)) return false;
    const double delta = sub_rn(lam_b, lam_a) / reach;
    const double d = ca == ya && cb == yb ? delta : sub_rn(cb, ca);
    double m1;
    arc_moments(ca, cb, d, m0, m1);
    r = sub_rn(m1, mul_rn(ya, m0)) / delta;
    if (t) *t = m1 / delta;
    return true;
}
// y K(y) = y / (pi sqrt((1 - y)(1 + y))) at an end of the grid seen from point i: the end term of a truncated window in d / d ln V; 0 where
// the window does not reach the end (|y| >= 1) or the end is the point itself.  1 - |y| = (reach - |lam_end - lam_i|) / reach, the
// difference first, as rot_end_term forms it.  K is singular at |y| = 1: an end within 1e-5 of a ring's edge is outside the
// derivative's contract (include/stardis_hip.h).
__device__ __forceinline__ double disk_end_term(double reach, double lam_i, double lam_end, bool self)
{
    if (self) return 0.0;
    const double dl = sub_rn(lam_end, lam_i), ay = fabs(dl);
    const double u = sub_rn(reach, ay) / reach;
    if (!(u > 0.0)) return 0.0;
    const double q = mul_rn(u, add_rn(1.0, ay / reach));
    return (dl / reach) / mul_rn(kPi, __dsqrt_rn(q));
}

// What the point's lanes sum over the cells of one ring, closed by the butterfly, in every lane of the point: num, numr (Ir, Gr; nullptr:
// not formed), den and, with kDeriv, tnum = sum_g (M1_g / Delta_g) (I[j+1] - I[j]) and tnumr.  The forward kernel and the adjoint's
// denominators call it (the mapping m is the forward's in both), so den has the same bits in both.  Every lane of the wave calls it;
// `on` false: nothing is searched or read.
struct DiskSums {
    double num, numr, den, tnum, tnumr;
};
template <bool kDeriv>
__device__ __forceinline__ void disk_ring_sums(int64_t n, const double* __restrict__ lam, const double* __restrict__ Ir,
                                               const double* __restrict__ Gr, int64_t i, double li, double reach, bool on, const RotLane& m,
                                               DiskSums& s)
{
    int64_t i0, i1;
    obs_windows(lam, lam, n, 1.0, sub_rn(li, reach), add_rn(li, reach), on, m.W, m.lane, i0, i1);
    const int64_t g0 = i0 > 0 ? i0 - 1 : 0, g1 = i1 < n - 1 ? i1 : n - 1;  // the window's cells and the partial cell on each side
    s = DiskSums{0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t g = g0 + m.t; on && g < g1; g += m.W) {
        double m0, sh, t = 0.0;
        if (!disk_cell(reach, li, lam[g], lam[g + 1], g == i ? 0 : (g + 1 == i ? 1 : -1), m0, sh, kDeriv ? &t : nullptr)) continue;
        const double wa = sub_rn(m0, sh);
        s.den = add_rn(s.den, m0);
        if (Ir) {
            const double fa = Ir[g], fb = Ir[g + 1];
            s.num = add_rn(add_rn(s.num, mul_rn(wa, fa)), mul_rn(sh, fb));
            if (kDeriv) s.tnum = add_rn(s.tnum, mul_rn(t, sub_rn(fb, fa)));
        }
        if (Gr) {
            const double ga = Gr[g], gb = Gr[g + 1];
            s.numr = add_rn(add_rn(s.numr, mul_rn(wa, ga)), mul_rn(sh, gb));
            if (kDeriv) s.tnumr = add_rn(s.tnumr, mul_rn(t, sub_rn(gb, ga)));
        }
    }
    for (int off = m.W >> 1; off > 0; off >>= 1) {
        s.num = add_rn(s.num, __shfl_xor(s.num, off)), s.numr = add_rn(s.numr, __shfl_xor(s.numr, off));
        s.den = add_rn(s.den, __shfl_xor(s.den, off));
        if (kDeriv) s.tnum = add_rn(s.tnum, __shfl_xor(s.tnum, off)), s.tnumr = add_rn(s.tnumr, __shfl_xor(s.tnumr, off));
    }
}

// kDeriv false: the forward sum alone (dlnv, dlnv_ref unused).  kDeriv true: also d out / d ln V, exact for the discrete operator (the
// spectrum is piecewise linear and the domain over lambda does not move, so no integration by parts is needed): per ring, reach > 0,
//     dnum = sum_g (M1_g / Delta_g) (I[j+1] - I[j]) - e_hi I[n-1] + e_lo I[0],   dden = -e_hi + e_lo,
//     e_hi = y_hi K(y_hi) where the window is truncated above (y_hi = (lam[n-1] - lam_i) / reach < 1), e_lo = y_lo K(y_lo) where it is
//     truncated below (y_lo = (lam[0] - lam_i) / reach > -1), else 0 (disk_end_term),
//     dA_r[i] = (dnum - A_r[i] dden) / den,   dout[i] = sum_r w_r dA_r[i] in the flux's order;
// !(reach > 0) contributes 0, !(V > 0) gives zeros.  out and out_ref are the same operations on the same operands in both.
template <bool kDeriv>
__global__ __launch_bounds__(kBlock) void k_disk_integrate(int64_t n, const double* __restrict__ lam, int n_rings,
                                                           const double* __restrict__ scale, const double* __restrict__ wts,
                                                           const double* __restrict__ I, int64_t ild, const double* __restrict__ I_ref,
                                                           const double* __restrict__ rot, double* __restrict__ out,
                                                           double* __restrict__ out_ref, double* __restrict__ dlnv,
                                                           double* __restrict__ dlnv_ref)
{
    const double V = rot[0], beta = V / kCKms;  // (the pair's limb darkening is not read: every ring has its own spectrum)
    RotLane m;
    if (!rot_mapping(n, lam, 2.0 * beta, V > 0.0, m)) return;
    const int64_t i = m.on ? m.pi : n - 1;
    const double li = lam[i];
    const int half = (n_rings + 1) >> 1;
    double lower = 0.0, upper = 0.0, lower_ref = 0.0, upper_ref = 0.0;
    double dlower = 0.0, dupper = 0.0, dlower_ref = 0.0, dupper_ref = 0.0;
    for (int r = 0; r < n_rings; ++r) {
        const double* __restrict__ Ir = I + (size_t)r * ild;
        const double* __restrict__ Gr = I_ref ? I_ref + (size_t)r * ild : nullptr;
        const double beta_r = mul_rn(beta, scale[r]), reach = mul_rn(li, beta_r);
        double a = Ir[i], a_ref = Gr ? Gr[i] : 0.0;  // !(reach > 0): a copy
        double da = 0.0, da_ref = 0.0;
        if (beta_r > 0.0) {                          // (the same in every lane of the wave)
            DiskSums s;
            disk_ring_sums<kDeriv>(n, lam, Ir, Gr, i, li, reach, m.on && reach > 0.0, m, s);
            if (reach > 0.0) {
                a = s.num / s.den, a_ref = s.numr / s.den;
                if (kDeriv) {
                    const double e_lo = disk_end_term(reach, li, lam[0], i == 0), e_hi = disk_end_term(reach, li, lam[n - 1], i == n - 1);
                    const double dden = sub_rn(e_lo, e_hi);
                    da = sub_rn(add_rn(s.tnum, sub_rn(mul_rn(e_lo, Ir[0]), mul_rn(e_hi, Ir[n - 1]))), mul_rn(a, dden)) / s.den;
                    if (Gr) da_ref = sub_rn(add_rn(s.tnumr, sub_rn(mul_rn(e_lo, Gr[0]), mul_rn(e_hi, Gr[n - 1]))), mul_rn(a_ref, dden)) / s.den;
                }
            }
        }
        const double w = wts[r], term = mul_rn(a, w), term_ref = mul_rn(a_ref, w);
        if (r < half) lower = add_rn(lower, term), lower_ref = add_rn(lower_ref, term_ref);
        else upper = add_rn(upper, term), upper_ref = add_rn(upper_ref, term_ref);
        if (kDeriv) {
            const double dterm = mul_rn(da, w), dterm_ref = mul_rn(da_ref, w);
            if (r < half) dlower = add_rn(dlower, dterm), dlower_ref = add_rn(dlower_ref, dterm_ref);
            else dupper = add_rn(dupper, dterm), dupper_ref = add_rn(dupper_ref, dterm_ref);
        }
    }
    if (m.t != 0 || !m.on) return;
    out[m.pi] = add_rn(lower, upper);
    if (I_ref) out_ref[m.pi] = add_rn(lower_ref, upper_ref);
    if (kDeriv) {
        dlnv[m.pi] = add_rn(dlower, dupper);
        if (I_ref && dlnv_ref) dlnv_ref[m.pi] = add_rn(dlower_ref, dupper_ref);
    }
}

// The transpose of k_disk_integrate (include/stardis_hip.h, sdx_disk_integrate_adjoint_dev).  The cotangent of a disk-integrated spectrum
// is a plane over (ring, node), each ring's spectrum being convolved with its own kernel:
//     W[r][j] = w_r sum_i (u_i / den_r(i)) ((M0 - r) of cell [j, j + 1] + r of cell [j - 1, j] in point i's row for ring r),
// disk_cell deciding, so the weights are the forward's bit for bit.  It is the broadening stages' pair per ring (blockIdx.y): a_r[i] = u_i /
// den_r(i) through disk_ring_sums in the forward's mapping (k_disk_integrate_adjoint_den), then the gather over the candidates
// lam_i in [lam_{j-1} / (1 + beta_r), lam_{j+1} / (1 - beta_r)] (k_disk_integrate_adjoint; stage_adjoint_of), times w_r, times nu_j / lam_j
// where nus is given.  A ring with !(beta_r > 0) passes w_r u_j through, as does a point whose own reach is not positive.
struct DiskRing {
    double beta, beta_r, weight;  // V / c (the mapping's: the widest ring a disk can have), beta ring_scale[r], w_r
    bool on;                      // beta_r > 0
};
__device__ __forceinline__ DiskRing disk_ring(const double* __restrict__ rot, const double* __restrict__ scale, const double* __restrict__ wts, int r)
{
    const double beta = rot[0] / kCKms, beta_r = mul_rn(beta, scale[r]);
    return DiskRing{beta, beta_r, wts[r], beta_r > 0.0};
}
__device__ __forceinline__ double stage_out(const DiskRing& r, double w)
{
    return mul_rn(r.weight, w);
}
struct DiskStage {
    struct Node {
        double below, above;  // lam_{j-1}, lam_{j+1}, clamped to the grid
    };
    static __device__ __forceinline__ double width(const DiskRing& r) { return 2.0 * r.beta; }
    static __device__ __forceinline__ double den(int64_t n, const double* __restrict__ lam, const DiskRing& r, const RotLane& m)
    {
        const int64_t i = m.on ? m.pi : n - 1;
        const double li = lam[i], reach = mul_rn(li, r.beta_r);
        DiskSums s;
        disk_ring_sums<false>(n, lam, nullptr, nullptr, i, li, reach, m.on && reach > 0.0, m, s);
        return reach > 0.0 ? s.den : 1.0;
    }
    static __device__ __forceinline__ Node node(int64_t n, const double* __restrict__ lam, int64_t j)
    {
        return Node{lam[j > 0 ? j - 1 : 0], lam[j < n - 1 ? j + 1 : n - 1]};
    }
    static __device__ __forceinline__ void candidates(const DiskRing& r, const Node& nd, double, double& lo, double& hi)
    {
        double unused;
        rot_candidates(nd.below, r.beta_r, lo, unused);
        rot_candidates(nd.above, r.beta_r, unused, hi);
    }
    static __device__ __forceinline__ bool weight(const DiskRing& r, const Node& nd, int64_t n, int64_t i, int64_t j, double lam_i, double lj, double& w)
    {
        const double reach = mul_rn(lam_i, r.beta_r);
        w = 1.0;
        if (!(reach > 0.0)) return i == j;  // (the forward's copy)
        double m0, sh;
        bool any = false;
        w = 0.0;
        if (j > 0 && disk_cell(reach, lam_i, nd.below, lj, j - 1 == i ? 0 : (j == i ? 1 : -1), m0, sh)) w = sh, any = true;
        if (j < n - 1 && disk_cell(reach, lam_i, lj, nd.above, j == i ? 0 : (j + 1 == i ? 1 : -1), m0, sh)) w = add_rn(w, sub_rn(m0, sh)), any = true;
        return any;
    }
};
// a, a_ref: [n_rings][row] doubles; blockIdx.y: the ring
__global__ __launch_bounds__(kBlock) void k_disk_integrate_adjoint_den(int64_t n, const double* __restrict__ lam, const double* __restrict__ scale,
                                                                       const double* __restrict__ wts, const double* __restrict__ rot,
                                                                       const double* __restrict__ u, const double* __restrict__ u_ref,
                                                                       double* __restrict__ a, double* __restrict__ a_ref, int64_t row)
{
    const int r = blockIdx.y;
    stage_adjoint_den_of<DiskStage>(n, lam, disk_ring(rot, scale, wts, r), u, u_ref, a + (size_t)r * row, u_ref ? a_ref + (size_t)r * row : nullptr);
}
__global__ __launch_bounds__(kBlock) void k_disk_integrate_adjoint(int64_t n, const double* __restrict__ lam, const double* __restrict__ scale,
                                                                   const double* __restrict__ wts, const double* __restrict__ rot,
                                                                   const double* __restrict__ a, const double* __restrict__ a_ref, int64_t row,
                                                                   const double* __restrict__ nus, double* __restrict__ W, double* __restrict__ W_ref,
                                                                   int64_t wld)
{
    const int r = blockIdx.y;
    stage_adjoint_of<DiskStage>(n, lam, disk_ring(rot, scale, wts, r), a + (size_t)r * row, a_ref ? a_ref + (size_t)r * row : nullptr, nus,
                                W + (size_t)r * wld, W_ref ? W_ref + (size_t)r * wld : nullptr);
}

// ------------------------------------------------------------------------------------------------
// Radial-tangential macroturbulence (include/stardis_hip.h, sdx_macroturbulence_dev): Gray's profile with equal areas and zeta_R = zeta_T =
// zeta, integrated over the disk without limb darkening, K(u) = exp(-u^2) - sqrt(pi) u erfc(u), u = |dv| / zeta, in velocity space on any
// ascending grid, between k_rotate and k_observe.  With beta = zeta / c, for point i
//     reach_i = lam_i (6 beta),  lo_i = lam_i - reach_i,  hi_i = lam_i + reach_i,   j is included iff lo_i <= lam_j <= hi_i or j = i,
//     u_ij = |lam_j - lam_i| / (lam_i beta),   e = exp(-(u u)),   s = (sqrt(pi) u) erfc(u),   K = max(e - s, 0)     (j = i: K = 1, s = 0),
//     w_ij = K h_j,   v_ij = s h_j   (h_j: rot_trapezoid),   out_i = (sum_j w_ij flux_j) / den_i,   den_i = sum_j w_ij,
//     dout_i = (sum_j v_ij flux_j - out_i sum_j v_ij) / den_i = d out_i / d ln zeta at fixed windows  (dK / d ln zeta = s: no new term).
// K(6) = 3e-18 of the peak: the window ends where the profile has left fp64.  !(zeta > 0) copies, dout = 0.  mac_weight is the ONE place
// where reach, u, K, s, w and v are rounded and a pair is included or not: the forward kernel, the adjoint's denominators and the
// adjoint's gather call it.  Mapping (rot_mapping with the window's width 2 (6 beta)), window search (obs_windows), trapezoid weights,
// order of the sums and the adjoint's two launches are k_rotate's; so are the bounds on every access and loop stated there.
constexpr double kMacReach = 6.0;

struct MacProfile {
    double beta, reach;  // zeta / c, 6 beta
    bool on;             // zeta > 0
};
__device__ __forceinline__ MacProfile mac_profile(const double* __restrict__ mac)
{
    const double zeta = mac[0], beta = zeta / kCKms;
    return MacProfile{beta, mul_rn(kMacReach, beta), zeta > 0.0};
}
// point i's weights for point j (self: j == i), h = the trapezoid weight of j: w = K h, v = s h; false: i does not include j
__device__ __forceinline__ bool mac_weight(const MacProfile& r, double lam_i, double lam_j, bool self, double h, double& w, double& v)
{
    double K = 1.0, s = 0.0;
    if (!self) {
        const double reach = mul_rn(lam_i, r.reach), lo = sub_rn(lam_i, reach), hi = add_rn(lam_i, reach);
        if (!(lo <= lam_j && lam_j <= hi)) return false;
        const double u = fabs(sub_rn(lam_j, lam_i)) / mul_rn(lam_i, r.beta);
        s = mul_rn(mul_rn(kSqrtPi, u), erfc(u));
        K = fmax(sub_rn(exp(-mul_rn(u, u)), s), 0.0);
    }
    w = mul_rn(K, h), v = mul_rn(s, h);
    return true;
}

// What the point's lanes sum, closed by the butterfly, in every lane of the point: num = sum_j w_ij flux[j], numr = sum_j w_ij ref[j],
// den = sum_j w_ij and, with deriv, the same three sums of v_ij (nullptr / false: not formed).  Not called where !(zeta > 0).
struct MacSums {
    double num, numr, den, vnum, vnumr, vden;
};
__device__ __forceinline__ void mac_point_sums(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                               const double* __restrict__ ref, bool deriv, const MacProfile& r, const RotLane& m, MacSums& s)
{
    const int64_t i = m.on ? m.pi : n - 1;
    const double li = lam[i];
    const double reach = mul_rn(li, r.reach);
    int64_t i0, i1;
    obs_windows(lam, lam, n, 1.0, sub_rn(li, reach), add_rn(li, reach), m.on, m.W, m.lane, i0, i1);
    s = MacSums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t j = i0 + m.t; j < i1; j += m.W) {
        double w, v;
        if (!mac_weight(r, li, lam[j], j == i, rot_trapezoid(lam, n, j), w, v)) continue;
        const double f = flux ? flux[j] : 0.0, g = ref ? ref[j] : 0.0;
        if (flux) s.num = add_rn(s.num, mul_rn(w, f));
        if (ref) s.numr = add_rn(s.numr, mul_rn(w, g));
        s.den = add_rn(s.den, w);
        if (deriv) {
            if (flux) s.vnum = add_rn(s.vnum, mul_rn(v, f));
            if (ref) s.vnumr = add_rn(s.vnumr, mul_rn(v, g));
            s.vden = add_rn(s.vden, v);
        }
    }
    for (int off = m.W >> 1; off > 0; off >>= 1) {
        s.num = add_rn(s.num, __shfl_xor(s.num, off)), s.numr = add_rn(s.numr, __shfl_xor(s.numr, off));
        s.den = add_rn(s.den, __shfl_xor(s.den, off));
        if (deriv) {
            s.vnum = add_rn(s.vnum, __shfl_xor(s.vnum, off)), s.vnumr = add_rn(s.vnumr, __shfl_xor(s.vnumr, off));
            s.vden = add_rn(s.vden, __shfl_xor(s.vden, off));
        }
    }
}

// dout, dout_ref: optional (nullptr: the v sums are not formed); dout_ref only with ref
__global__ __launch_bounds__(kBlock) void k_macroturbulence(int64_t n, const double* __restrict__ lam, const double* __restrict__ flux,
                                                            const double* __restrict__ ref, const double* __restrict__ mac,
                                                            double* __restrict__ out, double* __restrict__ out_ref, double* __restrict__ dout,
                                                            double* __restrict__ dout_ref)
{
    const MacProfile r = mac_profile(mac);
    RotLane m;
    if (!rot_mapping(n, lam, 2.0 * r.reach, r.on, m)) return;
    if (!r.on) {  // (the group's first wave, eight lanes per point: a copy)
        if (m.t == 0 && m.on) {
            out[m.pi] = flux[m.pi];
            if (ref) out_ref[m.pi] = ref[m.pi];
            if (dout) dout[m.pi] = 0.0;
            if (dout_ref) dout_ref[m.pi] = 0.0;
        }
        return;
    }
    MacSums s;
    mac_point_sums(n, lam, flux, ref, dout != nullptr || dout_ref != nullptr, r, m, s);
    if (m.t != 0 || !m.on) return;
    const double o = s.num / s.den;
    out[m.pi] = o;
    if (dout) dout[m.pi] = sub_rn(s.vnum, mul_rn(o, s.vden)) / s.den;
    if (ref) {
        const double g = s.numr / s.den;
        out_ref[m.pi] = g;
        if (dout_ref) dout_ref[m.pi] = sub_rn(s.vnumr, mul_rn(g, s.vden)) / s.den;
    }
}

// the stage of stage_adjoint_den and stage_adjoint
struct MacStage {
    struct Node {
        double h;  // the trapezoid weight of lam_j
    };
    static __device__ __forceinline__ MacProfile load(const double* __restrict__ mac) { return mac_profile(mac); }
    static __device__ __forceinline__ double width(const MacProfile& r) { return 2.0 * r.reach; }
    static __device__ __forceinline__ double den(int64_t n, const double* __restrict__ lam, const MacProfile& r, const RotLane& m)
    {
        MacSums s;
        mac_point_sums(n, lam, nullptr, nullptr, false, r, m, s);
        return s.den;
    }
    static __device__ __forceinline__ Node node(int64_t n, const double* __restrict__ lam, int64_t j) { return Node{rot_trapezoid(lam, n, j)}; }
    // lam_i in [lam_j / (1 + 6 beta), lam_j / (1 - 6 beta)]; mac_weight decides
    static __device__ __forceinline__ void candidates(const MacProfile& r, const Node&, double lj, double& lo, double& hi)
    {
        rot_candidates(lj, r.reach, lo, hi);
    }
    static __device__ __forceinline__ bool weight(const MacProfile& r, const Node& nd, int64_t, int64_t i, int64_t j, double lam_i, double lj, double& w)
    {
        double v;
        return mac_weight(r, lam_i, lj, i == j, nd.h, w, v);
    }
};
__global__ __launch_bounds__(kBlock) void k_macroturbulence_adjoint_den(int64_t n, const double* __restrict__ lam, const double* __restrict__ mac,
                                                                        const double* __restrict__ u, const double* __restrict__ u_ref,
                                                                        double* __restrict__ a, double* __restrict__ a_ref)
{
    stage_adjoint_den<MacStage>(n, lam, mac, u, u_ref, a, a_ref);
}
__global__ __launch_bounds__(kBlock) void k_macroturbulence_adjoint(int64_t n, const double* __restrict__ lam, const double* __restrict__ mac,
                                                                    const double* __restrict__ a, const double* __restrict__ a_ref,
                                                                    const double* __restrict__ nus, double* __restrict__ w_out,
                                                                    double* __restrict__ w_ref)
{
    stage_adjoint<MacStage>(n, lam, mac, a, a_ref, nus, w_out, w_ref);
}

// ------------------------------------------------------------------------------------------------
// The weight plane of the per-line sensitivities from the response functions: W[k][j] = w[j] R_alpha[k][j] / total[k][j] (w = nullptr: 1),
// every operation one correctly rounded fp64 operation; a zero in total gives what IEEE gives.
__global__ __launch_bounds__(kBlock) void k_response_weight(int n_depth, int64_t n_nu, const double* __restrict__ R, int64_t rld,
                                                            const double* __restrict__ total, int64_t tld, const double* __restrict__ w,
                                                            double* __restrict__ out, int64_t old)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n_nu) return;
    const double q = R[(size_t)k * rld + i] / total[(size_t)k * tld + i];
    out[(size_t)k * old + i] = w ? mul_rn(w[i], q) : q;
}

// ------------------------------------------------------------------------------------------------
// The adjoints of the line-opacity sum (include/stardis_hip.h): per (line, depth) item, over i in [lo_ld, hi_ld) within the shard,
//   sdx_line_adjoint_dev        s[l][d] = sum W[d][i] * voigt_term(nu_i - nu_l; 1 / dw_ld, y_ld, amp_ld)                (StrengthSums)
//   sdx_line_param_adjoint_dev  S0 = sum W T,  Sx = sum W amp K_x,  Sxx = sum W amp x K_x,  Sy = sum W amp K_y           (ProfileSums)
// the window from window_rule on the GLOBAL grid (d_nu by block_dnu_scan, the centre by closest_index: what sdx_line_windows_dev
// reports), the term with narrow_params + region1_setup as the fp64 line kernels form it, K_x and K_y of the region's own formula
// (voigt_grad_x).  Always the direct sum, always fp64.  One set of kernel bodies serves both: a sums policy names the number of sums
// of an item (kSums), its constants and what one point adds to the sums; everything else below is written once.
//
// Windows run from 20 points to the whole grid, so k_line_adjoint_plan (one thread per item) sorts the items by the length of the
// clipped window first.  It appends with integer atomics, so the position of an item in a list depends on the run — which wave sums
// an item does, the order of its sum does not:
//   short  half-width <= kNarrowHalfWidth: adj_direct<P, 4>, sixteen items per wave, four lanes per item — the 20 points of a floor
//          window keep all four lanes busy for five trips, where sixteen lanes per item idle 12 of 32 lane-trips and a wave per item
//          44 of 64 lanes; the floor windows are line cores, every point the long Faddeeva regions;
//   long   up to kAdjTiledMin points: adj_direct<P, 64>, one wave per item, lanes striding the window (coalesced loads of W and nus);
//   tiled  longer: adj_tiled<P>, the transpose of the line kernels' wide role.  A wave per item reads 16 bytes per term and is
//          bound by the L2 (the first measurement in profiles/EXPERIMENTS.md: 5 x the direct sum at S-c3); here a wave holds a TILE of kAdjTile columns of one depth
//          in registers (nus, W: sixteen of each per lane), walks the depth's list of tiled lines and closes every (line, tile) with a
//          butterfly — the loads are shared by all the lines of the depth.  A wave owns a run of consecutive tiles (a supertile) and
//          every J-th line of the list; lane 0 adds the tiles of a supertile in ascending order into the item's slot of `partial`.
//          The number of supertiles M follows from the number of tiled items (adj_tiling: `cap` groups of kSums partial sums in all),
//          i.e. from the shapes, the windows and the shard.
// The discipline of the sums: x = (nu_i - nu_l) * inv is one product, formed before the point function; a lane adds its points in
// ascending order, one FMA per term and sum; a butterfly per sum over the lanes (offsets G/2 ... 1) closes the item or the tile; the
// gathers (one wave per line, lane <-> depth) add an item's supertiles in ascending order (adj_item_sums) and the line's depths by the
// same butterfly.  No floating-point atomics.  An item whose window misses the shard is exactly 0.
// Storage: sum k of an item at sld[k * items + item] (the plan's zero for an empty item lands in plane 0: the strength gather reads
// it, the profile gather does not), sum k of supertile s of a tiled item at partial[(tslot * M + s) * kSums + k].
constexpr int kAdjTileP = 16;
constexpr int kAdjTile = 64 * kAdjTileP;
constexpr int kAdjTiledMin = 4 * kAdjTile;
struct AdjWork {
    double* pd;        // [0] = d_nu, [1] = 1 / d_nu
    int* counters;     // [0] short items, [1] long items, [2] tiled items, [4 + d] tiled items of depth d
    int* centre;       // [N_l]
    int* list_short;   // [items]
    int* list_long;    // [items]
    int* list_tiled;   // [N_d][N_l] the lines of the tiled items of each depth
    int* tslot;        // [items] a tiled item's row of `partial` (not written for the others)
    double* sld;       // [kSums][items]; the strength adjoint's is the caller's out_line_depth where that is given
    double* partial;   // [tiled items][M][kSums]
    int64_t cap;       // groups of kSums doubles in `partial`, at least the number of items
    int n_tiles;       // tiles of the shard
};
struct AdjLines {
    int n_depth, gamma_cols;
    int64_t n_nu, nu_begin, nu_count, n_lines;
    const double *nus, *line_nus, *doppler, *gammas, *alphas;
};

__global__ __launch_bounds__(kPreBlock) void k_line_adjoint_setup(AdjLines a, AdjWork w)
{
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        __shared__ double s_red[kPreBlock / 64];
        for (int k = tid; k < 4 + a.n_depth; k += kPreBlock) w.counters[k] = 0;
        const double d_nu = block_dnu_scan(a.nus, a.n_nu, s_red);
        if (tid == 0) w.pd[0] = d_nu, w.pd[1] = 1.0 / d_nu;
        return;
    }
    const int64_t l = (int64_t)(blockIdx.x - 1) * kPreBlock + tid;
    if (l < a.n_lines) w.centre[l] = (int)closest_index(a.nus, a.n_nu, a.line_nus[l]);
}

// the item's window clipped to the shard -> [b, e) (e <= b: empty); returns the half-width of the rule
__device__ __forceinline__ int64_t adjoint_window(const AdjLines& a, const AdjWork& w, double d_nu, double r_dnu, int64_t l, double dw, double g,
                                                  double al, int64_t& b, int64_t& e)
{
    int lo, hi;
    const int64_t hw = window_rule(w.centre[l], a.n_nu, d_nu, r_dnu, g, dw, al, lo, hi);
    b = max((int64_t)lo, a.nu_begin);
    e = min((int64_t)hi, a.nu_begin + a.nu_count);
    return hw;
}
// supertiles per item and tiles per supertile, from the number of tiled items
__device__ __forceinline__ void adj_tiling(const AdjWork& w, int& M, int& tps)
{
    const int64_t n_tiled = max(w.counters[2], 1);
    const int64_t m = max((int64_t)1, min((int64_t)w.n_tiles, w.cap / n_tiled));
    tps = (int)((w.n_tiles + m - 1) / m);
    M = (w.n_tiles + tps - 1) / tps;  // (<= m: the rows of `partial` fit)
}

// 0: nothing to add, 1: short, 2: long, 3: tiled
__device__ __forceinline__ int adjoint_class(int64_t hw, int64_t b, int64_t e)
{
    return e <= b ? 0 : (hw <= kNarrowHalfWidth ? 1 : (e - b > kAdjTiledMin ? 3 : 2));
}

// One thread per item in memory order, so that neighbours in a list are neighbours in the tables.  A tiled item takes a row of `partial`
// (one atomic per wave) and a place in its depth's list of tiled lines (one atomic per item).  Two other plans were measured and left
// (profiles/EXPERIMENTS.md, "Per-line flux sensitivities"): a wave per 64 lines of one depth appends with one atomic, but its lists then
// jump through the tables and the list walks pay for it; one list of the lines tiled at ANY depth, walked at every depth, costs the
// tiled role more than the atomics cost here.
__global__ __launch_bounds__(kBlock) void k_line_adjoint_plan(AdjLines a, AdjWork w)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_items = a.n_lines * a.n_depth;
    const int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int cls = 0;
    int64_t l = 0;
    int d = 0;
    if (item < n_items) {
        l = item / a.n_depth;
        d = (int)(item - l * a.n_depth);
        int64_t b, e;
        const int64_t hw = adjoint_window(a, w, w.pd[0], w.pd[1], l, a.doppler[item], a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)],
                                          a.alphas[item], b, e);
        cls = adjoint_class(hw, b, e);
        if (cls == 0) w.sld[item] = 0.0;
    }
    const unsigned long long below = (1ull << lane) - 1;
    const unsigned long long ms = __ballot(cls == 1), ml = __ballot(cls == 2), mt = __ballot(cls == 3);
    int bs = 0, bl = 0, bt = 0;
    if (lane == 0) {
        if (ms) bs = atomicAdd(&w.counters[0], __popcll(ms));
        if (ml) bl = atomicAdd(&w.counters[1], __popcll(ml));
        if (mt) bt = atomicAdd(&w.counters[2], __popcll(mt));
    }
    bs = __shfl(bs, 0), bl = __shfl(bl, 0), bt = __shfl(bt, 0);
    if (cls == 1) w.list_short[bs + __popcll(ms & below)] = (int)item;
    if (cls == 2) w.list_long[bl + __popcll(ml & below)] = (int)item;
    if (cls == 3) {
        w.tslot[item] = bt + __popcll(mt & below);
        w.list_tiled[(size_t)d * a.n_lines + atomicAdd(&w.counters[4 + d], 1)] = (int)l;
    }
}

// The sums policies: the constants of an item, and what one point (weight wt, x, the item's y and amp) adds to the item's sums —
// add() with the point function's own region tests, add_wing() without them, for a whole tile in the line's far wing.
struct StrengthSums {
    static constexpr int kSums = 1;
    using Consts = RegionI;
    static __device__ __forceinline__ Consts setup(double y, double amp) { return region1_setup(y, amp); }
    static __device__ __forceinline__ void add(double (&acc)[1], double wt, double x, double y, double amp, const Consts& k)
    {
        acc[0] = fma(wt, voigt_add_x(0.0, x, y, amp, k), acc[0]);  // (voigt_term at x)
    }
    static __device__ __forceinline__ void add_wing(double (&acc)[1], double wt, double x, const Consts& k) { acc[0] = fma(wt, region1_add(0.0, x, k), acc[0]); }
};
struct ProfileSums {
    static constexpr int kSums = 4;  // S0, Sx, Sxx, Sy
    using Consts = RegionIGrad;
    static __device__ __forceinline__ Consts setup(double y, double amp) { return region1_grad_setup(y, amp); }
    static __device__ __forceinline__ void param_add(double (&acc)[4], double wt, double x, double t, double tx, double ty)
    {
        acc[0] = fma(wt, t, acc[0]);
        acc[1] = fma(wt, tx, acc[1]);
        acc[2] = fma(wt, x * tx, acc[2]);
        acc[3] = fma(wt, ty, acc[3]);
    }
    static __device__ __forceinline__ void add(double (&acc)[4], double wt, double x, double y, double amp, const Consts& k)
    {
        double t, tx, ty;
        voigt_grad_x(x, y, amp, k, t, tx, ty);
        param_add(acc, wt, x, t, tx, ty);
    }
    static __device__ __forceinline__ void add_wing(double (&acc)[4], double wt, double x, const Consts& k)
    {
        double t, tx, ty;
        region1_grad(x, k, t, tx, ty);
        param_add(acc, wt, x, t, tx, ty);
    }
};

// the short (G = 4) and the long (G = 64) items: G lanes per item, striding its window
template <class P, int G>
__device__ __forceinline__ void adj_direct(const AdjLines& a, const AdjWork& w, const double* __restrict__ weight, int64_t wld)
{
    constexpr int kPerWave = 64 / G, kSums = P::kSums;
    const int lane = threadIdx.x & 63, sub = lane & (G - 1);
    const int64_t n_waves = (int64_t)gridDim.x * (kBlock / 64);
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const double d_nu = w.pd[0], r_dnu = w.pd[1];
    const int64_t n_units = w.counters[G == 64 ? 1 : 0];
    const int64_t n_items = a.n_lines * a.n_depth;
    const int* __restrict__ list = G == 64 ? w.list_long : w.list_short;
    for (int64_t u0 = wave * kPerWave; u0 < n_units; u0 += n_waves * kPerWave) {  // (wave-uniform: every lane reaches the butterfly)
        const int64_t u = u0 + lane / G;
        const bool on = u < n_units;
        const int64_t item = on ? list[u] : 0;
        const int64_t l = item / a.n_depth;
        const int d = (int)(item - l * a.n_depth);
        const double lnu = a.line_nus[l], dw = a.doppler[item], g = a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)], al = a.alphas[item];
        int64_t b, e;
        adjoint_window(a, w, d_nu, r_dnu, l, dw, g, al, b, e);
        if (!on) e = b;
        double inv, y, amp;
        narrow_params(dw, g, al, inv, y, amp);
        const typename P::Consts k1 = P::setup(y, amp);
        const double* __restrict__ wrow = weight + (size_t)d * wld;
        double acc[kSums] = {};
        for (int64_t i = b + sub; i < e; i += G) {
            const double x = (a.nus[i] - lnu) * inv;
            P::add(acc, wrow[i - a.nu_begin], x, y, amp, k1);
        }
#pragma unroll
        for (int k = 0; k < kSums; ++k) {
#pragma unroll
            for (int off = G >> 1; off > 0; off >>= 1) acc[k] = add_rn(acc[k], __shfl_xor(acc[k], off));
        }
        if (sub == 0 && on) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) w.sld[(size_t)k * n_items + item] = acc[k];
        }
    }
}

// wave = (depth d, supertile s, line subset j of J): the tiles of s in ascending order, in each the lines j, j + J, ... of depth d's list
template <class P>
__device__ __forceinline__ void adj_tiled(const AdjLines& a, const AdjWork& w, const double* __restrict__ weight, int64_t wld, int J)
{
    constexpr int kSums = P::kSums;
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * (kBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int per_depth = w.n_tiles * J;
    const int d = (int)(wid / per_depth);
    if (d >= a.n_depth || w.counters[2] == 0) return;
    const int r = (int)(wid - (int64_t)d * per_depth), s = r / J, j = r - s * J;
    int M, tps;
    adj_tiling(w, M, tps);
    const int n_d = w.counters[4 + d];
    if (s >= M || j >= n_d) return;
    const double d_nu = w.pd[0], r_dnu = w.pd[1];
    const int64_t shard_end = a.nu_begin + a.nu_count;
    const double* __restrict__ wrow = weight + (size_t)d * wld;
    const int* __restrict__ list = w.list_tiled + (size_t)d * a.n_lines;
    const int t_end = min((s + 1) * tps, w.n_tiles);
    for (int t = s * tps; t < t_end; ++t) {
        const int64_t base = a.nu_begin + (int64_t)t * kAdjTile;
        const int64_t tile_end = min(base + kAdjTile, shard_end);
        const double nu_first = a.nus[base], nu_last = a.nus[tile_end - 1];  // (the grid descends)
        double nu[kAdjTileP], wt[kAdjTileP];
#pragma unroll
        for (int p = 0; p < kAdjTileP; ++p) {
            const int64_t i = base + p * 64 + lane;
            const bool ok = i < shard_end;
            nu[p] = ok ? a.nus[i] : 0.0;
            wt[p] = ok ? wrow[i - a.nu_begin] : 0.0;
        }
        for (int e = j; e < n_d; e += J) {
            const int64_t l = list[e];
            const size_t item = (size_t)l * a.n_depth + d;
            const double lnu = a.line_nus[l], dw = a.doppler[item], g = a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)], al = a.alphas[item];
            int64_t b, we;
            adjoint_window(a, w, d_nu, r_dnu, l, dw, g, al, b, we);
            if (we <= base || b >= tile_end) continue;  // (uniform)
            double inv, y, amp;
            narrow_params(dw, g, al, inv, y, amp);
            const typename P::Consts k1 = P::setup(y, amp);
            double acc[kSums] = {};
            // A whole tile inside the window and in the line's far wing — the line's frequency outside the tile's, both end points
            // with |x| + y > 15 — needs no test per point: the rounded difference and product are monotone in the frequency, so every
            // point of the tile then passes the point function's own test, and add_wing is what it evaluates.
            const bool wings = (lnu > nu_first || lnu < nu_last) && add_rn(fabs((nu_first - lnu) * inv), y) > 15.0 && add_rn(fabs((nu_last - lnu) * inv), y) > 15.0;
            if (wings && b <= base && we >= base + kAdjTile) {
#pragma unroll
                for (int p = 0; p < kAdjTileP; ++p) P::add_wing(acc, wt[p], (nu[p] - lnu) * inv, k1);
            } else {
                const unsigned len = (unsigned)(we - b);
                const int rel0 = (int)(base + lane - b);  // (negative: in front of the window, far above len as an unsigned number)
#pragma unroll
                for (int p = 0; p < kAdjTileP; ++p)
                    if ((unsigned)(rel0 + p * 64) < len) P::add(acc, wt[p], (nu[p] - lnu) * inv, y, amp, k1);
            }
#pragma unroll
            for (int k = 0; k < kSums; ++k) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) acc[k] = add_rn(acc[k], __shfl_xor(acc[k], off));
            }
            if (lane == 0) {
                double* const slot = w.partial + ((size_t)w.tslot[item] * M + s) * kSums;
                const bool first = t == max(s * tps, (int)((b - a.nu_begin) / kAdjTile));  // the supertile's first tile inside the window
#pragma unroll
                for (int k = 0; k < kSums; ++k) slot[k] = first ? acc[k] : add_rn(slot[k], acc[k]);
            }
        }
    }
}

// the gathers' common part, an item's sums -> sum: a tiled item's supertiles in ascending order, any other item's from sld (class 0
// there: the plan's zero in plane 0)
template <class P>
__device__ __forceinline__ void adj_item_sums(const AdjLines& a, const AdjWork& w, int M, int tps, size_t item, int cls, int64_t b, int64_t e,
                                              double (&sum)[P::kSums])
{
    constexpr int kSums = P::kSums;
    if (cls == 3) {
        const int slot = w.tslot[item];
        const int sa = (int)((b - a.nu_begin) / kAdjTile) / tps, sb = (int)((e - 1 - a.nu_begin) / kAdjTile) / tps;
#pragma unroll
        for (int k = 0; k < kSums; ++k) sum[k] = 0.0;
        for (int s = sa; s <= sb; ++s) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) sum[k] = add_rn(sum[k], w.partial[((size_t)slot * M + s) * kSums + k]);
        }
    } else {
        const size_t n_items = (size_t)a.n_lines * a.n_depth;
#pragma unroll
        for (int k = 0; k < kSums; ++k) sum[k] = w.sld[k * n_items + item];
    }
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_line_adjoint(AdjLines a, AdjWork w, const double* __restrict__ weight, int64_t wld)
{
    adj_direct<StrengthSums, G>(a, w, weight, wld);
}
// The strength adjoint's tiled role stays the hand-written copy of adj_tiled<StrengthSums>: the bits are the same, but the shared body
// compiled the whole-tile wing condition as one mask instead of two branches and measured 3.5 % slower at S-c3 (profiles/EXPERIMENTS.md,
// "Line adjoints: one kernel set").  A change to adj_tiled is made here too; the hash A/B of scripts/lib_ab.py `adjoints` holds the two together.
__global__ __launch_bounds__(kBlock) void k_line_adjoint_tiled(AdjLines a, AdjWork w, const double* __restrict__ weight, int64_t wld, int J)
{
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * (kBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int per_depth = w.n_tiles * J;
    const int d = (int)(wid / per_depth);
    if (d >= a.n_depth || w.counters[2] == 0) return;
    const int r = (int)(wid - (int64_t)d * per_depth), s = r / J, j = r - s * J;
    int M, tps;
    adj_tiling(w, M, tps);
    const int n_d = w.counters[4 + d];
    if (s >= M || j >= n_d) return;
    const double d_nu = w.pd[0], r_dnu = w.pd[1];
    const int64_t shard_end = a.nu_begin + a.nu_count;
    const double* __restrict__ wrow = weight + (size_t)d * wld;
    const int* __restrict__ list = w.list_tiled + (size_t)d * a.n_lines;
    const int t_end = min((s + 1) * tps, w.n_tiles);
    for (int t = s * tps; t < t_end; ++t) {
        const int64_t base = a.nu_begin + (int64_t)t * kAdjTile;
        const int64_t tile_end = min(base + kAdjTile, shard_end);
        const double nu_first = a.nus[base], nu_last = a.nus[tile_end - 1];  // (the grid descends)
        double nu[kAdjTileP], wt[kAdjTileP];
#pragma unroll
        for (int p = 0; p < kAdjTileP; ++p) {
            const int64_t i = base + p * 64 + lane;
            const bool ok = i < shard_end;
            nu[p] = ok ? a.nus[i] : 0.0;
            wt[p] = ok ? wrow[i - a.nu_begin] : 0.0;
        }
        for (int e = j; e < n_d; e += J) {
            const int64_t l = list[e];
            const size_t item = (size_t)l * a.n_depth + d;
            const double lnu = a.line_nus[l], dw = a.doppler[item], g = a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)], al = a.alphas[item];
            int64_t b, we;
            adjoint_window(a, w, d_nu, r_dnu, l, dw, g, al, b, we);
            if (we <= base || b >= tile_end) continue;  // (uniform)
            double inv, y, amp;
            narrow_params(dw, g, al, inv, y, amp);
            const RegionI k1 = region1_setup(y, amp);
            double acc = 0.0;
            // A whole tile inside the window and in the line's far wing — the line's frequency outside the tile's, both end points
            // with |x| + y > 15 — needs no test per point: the rounded difference and product are monotone in the frequency, so every
            // point of the tile then passes voigt_term's own test, and region1_add is what it evaluates.
            const bool wings = (lnu > nu_first || lnu < nu_last) && add_rn(fabs((nu_first - lnu) * inv), y) > 15.0 && add_rn(fabs((nu_last - lnu) * inv), y) > 15.0;
            if (wings && b <= base && we >= base + kAdjTile) {
#pragma unroll
                for (int p = 0; p < kAdjTileP; ++p) acc = fma(wt[p], region1_add(0.0, (nu[p] - lnu) * inv, k1), acc);
            } else {
                const unsigned len = (unsigned)(we - b);
                const int rel0 = (int)(base + lane - b);  // (negative: in front of the window, far above len as an unsigned number)
#pragma unroll
                for (int p = 0; p < kAdjTileP; ++p)
                    if ((unsigned)(rel0 + p * 64) < len) acc = fma(wt[p], voigt_term(nu[p] - lnu, inv, y, amp, k1), acc);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc = add_rn(acc, __shfl_xor(acc, off));
            if (lane == 0) {
                double* const slot = w.partial + (size_t)w.tslot[item] * M + s;
                const bool first = t == max(s * tps, (int)((b - a.nu_begin) / kAdjTile));  // the supertile's first tile inside the window
                *slot = first ? acc : add_rn(*slot, acc);
            }
        }
    }
}
template <int G>
__global__ __launch_bounds__(kBlock) void k_line_param_adjoint(AdjLines a, AdjWork w, const double* __restrict__ weight, int64_t wld)
{
    adj_direct<ProfileSums, G>(a, w, weight, wld);
}
__global__ __launch_bounds__(kBlock) void k_line_param_adjoint_tiled(AdjLines a, AdjWork w, const double* __restrict__ weight, int64_t wld, int J)
{
    adj_tiled<ProfileSums>(a, w, weight, wld, J);
}

// s[l][d] of the line's items (a tiled item's is written back into sld), and their sum over the depths
__global__ __launch_bounds__(kBlock) void k_line_adjoint_gather(AdjLines a, AdjWork w, double* __restrict__ out_line)
{
    const int lane = threadIdx.x & 63;
    const int64_t l = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (l >= a.n_lines) return;
    int M, tps;
    adj_tiling(w, M, tps);
    double line = 0.0;
    for (int d0 = 0; d0 < a.n_depth; d0 += 64) {
        const int d = d0 + lane;
        double v[1] = {0.0};
        if (d < a.n_depth) {
            const size_t item = (size_t)l * a.n_depth + d;
            int64_t b, e;
            const int64_t hw = adjoint_window(a, w, w.pd[0], w.pd[1], l, a.doppler[item], a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)],
                                              a.alphas[item], b, e);
            const int cls = adjoint_class(hw, b, e);
            adj_item_sums<StrengthSums>(a, w, M, tps, item, cls, b, e, v);
            if (cls == 3) w.sld[item] = v[0];
        }
        for (int off = 32; off > 0; off >>= 1) v[0] = add_rn(v[0], __shfl_xor(v[0], off));
        line = add_rn(line, v[0]);
    }
    if (lane == 0 && out_line) out_line[l] = line;
}

// d/d ln gamma_ld = y Sy,    d/d ln dw_ld = -(S0 + Sxx + y Sy),    d/d nu_l = -Sx / dw_ld    of the line's items, and their sums over the depths
struct ParamOut {
    double *damping, *doppler, *centre;                    // [N_l] or null
    double *damping_depth, *doppler_depth, *centre_depth;  // [N_l][N_d] or null
};
__global__ __launch_bounds__(kBlock) void k_line_param_adjoint_gather(AdjLines a, AdjWork w, ParamOut o)
{
    const int lane = threadIdx.x & 63;
    const int64_t l = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (l >= a.n_lines) return;
    int M, tps;
    adj_tiling(w, M, tps);
    double line[3] = {0.0, 0.0, 0.0};
    for (int d0 = 0; d0 < a.n_depth; d0 += 64) {
        const int d = d0 + lane;
        double v[3] = {0.0, 0.0, 0.0};
        if (d < a.n_depth) {
            const size_t item = (size_t)l * a.n_depth + d;
            const double dw = a.doppler[item], g = a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)], al = a.alphas[item];
            int64_t b, e;
            const int64_t hw = adjoint_window(a, w, w.pd[0], w.pd[1], l, dw, g, al, b, e);
            const int cls = adjoint_class(hw, b, e);
            if (cls != 0) {  // (an item without a term in the shard: exactly 0)
                double sum[ProfileSums::kSums];
                adj_item_sums<ProfileSums>(a, w, M, tps, item, cls, b, e, sum);
                double inv, y, amp;
                narrow_params(dw, g, al, inv, y, amp);
                v[0] = mul_rn(y, sum[3]);
                v[1] = -add_rn(add_rn(sum[0], sum[2]), v[0]);
                v[2] = -mul_rn(sum[1], inv);
            }
            if (o.damping_depth) o.damping_depth[item] = v[0];
            if (o.doppler_depth) o.doppler_depth[item] = v[1];
            if (o.centre_depth) o.centre_depth[item] = v[2];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[k] = add_rn(v[k], __shfl_xor(v[k], off));
            line[k] = add_rn(line[k], v[k]);
        }
    }
    if (lane == 0) {
        if (o.damping) o.damping[l] = line[0];
        if (o.doppler) o.doppler[l] = line[1];
        if (o.centre) o.centre[l] = line[2];
    }
}

// ------------------------------------------------------------------------------------------------
// The tangent of the line-opacity sum (include/stardis_hip.h, sdx_line_tangent_dev): the plane
//     out[d][i] = sum over the items (l, d) whose window covers i of  a T + g y Ty - b (T + x Tx + y Ty) - n Tx / dw
// with T = amp K, Tx = amp K_x, Ty = amp K_y from voigt_grad_x and the directions a = d ln alpha, g = d ln gamma, b = d ln dw, n = d nu_l
// of the item — the transpose of k_line_adjoint and k_line_param_adjoint, at their windows (adjoint_window's rule on the GLOBAL grid)
// and regions.  Always the direct sum, always fp64.
//
// A column's sum must not depend on the run or on the shard, so nothing here appends with atomics and no sum crosses lanes:
//   k_line_tangent_plan  (depth, 256 lines) per block: the window of every item clipped to the shard into win_lo / win_hi [N_d][N_l] —
//                        empty (0, 0) where the window misses the shard or EVERY direction of the item is exactly zero (a species mask
//                        costs what the species costs); a WIDE item (half-width of the rule above kTanWide) is marked by -1 - lo.  The
//                        block counts its wide items;
//   k_line_tangent_scan  a wave per depth: exclusive prefix of the blocks' counts;
//   k_line_tangent_list  the plan's geometry: ballot and prefix place the wide lines of a depth in ASCENDING line order in its list;
//   k_line_tangent       a wave per (depth, tile of kTanTile columns of the shard), a lane owns kTanP columns (stride 64: coalesced).  It
//                        walks the depth's wide list, then the contiguous range of lines whose centre index lies within kTanWide of the
//                        tile (centre[] descends as the lines ascend: a 64-ary search, all lanes probing) — 64 candidates at a time: each
//                        lane tests one window against the tile and, where it hits, forms its item's constants (one round of loads, one
//                        reciprocal for the 64); a ballot names the hits, and the wave evaluates them in ascending order, the constants
//                        of each from its lane by v_readlane.  A whole tile in a line's far wing takes region1_grad without a test.
// So every column adds its wide items in ascending line order and then its other items in ascending line order, whatever the tile it
// falls in: the bits do not depend on the shard.  A column no item covers is written as 0.0.  (Tiles of 512 and 1024 columns were
// measured and lost at both sizes: profiles/EXPERIMENTS.md, "The tangent of the line-opacity sum".)
constexpr int kTanP = 4;
constexpr int kTanTile = 64 * kTanP;
constexpr int kTanWide = 256;
struct TanDirs {
    const double *strength, *damping, *doppler, *centre;  // [N_l][cols] or null
    int cols;                                             // 1 or N_d
};
struct TanWork {
    int* centre;    // [N_l] (k_line_adjoint_setup)
    double* pd;     // [0] = d_nu, [1] = 1 / d_nu (k_line_adjoint_setup)
    int* win_lo;    // [N_d][N_l]
    int* win_hi;    // [N_d][N_l]
    int* list;      // [N_d][N_l] the wide lines of each depth, ascending
    int* chunk;     // [N_d][n_chunks] wide items per block of the plan, then their exclusive prefix
    int* n_wide;    // [N_d]
    int n_chunks;
};

// the wave's count of `flag` into s_cnt -> this thread's rank among the block's flagged threads, and (total) their number
__device__ __forceinline__ int tan_block_rank(bool flag, int* s_cnt, int& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_cnt[wv] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int k = 0; k < kBlock / 64; ++k) {
        if (k < wv) before += s_cnt[k];
        total += s_cnt[k];
    }
    return before + __popcll(m & ((1ull << lane) - 1));
}

__global__ __launch_bounds__(kBlock) void k_line_tangent_plan(AdjLines a, TanDirs dir, TanWork w)
{
    __shared__ int s_cnt[kBlock / 64];
    const int d = blockIdx.y;
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool wide = false;
    if (l < a.n_lines) {
        const size_t item = (size_t)l * a.n_depth + d, k = (size_t)l * dir.cols + (dir.cols == 1 ? 0 : d);
        const bool live = (dir.strength && dir.strength[k] != 0.0) || (dir.damping && dir.damping[k] != 0.0) ||
                          (dir.doppler && dir.doppler[k] != 0.0) || (dir.centre && dir.centre[k] != 0.0);
        int lo = 0, hi = 0;
        if (live) {
            int rlo, rhi;
            const int64_t hw = window_rule(w.centre[l], a.n_nu, w.pd[0], w.pd[1], a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)],
                                           a.doppler[item], a.alphas[item], rlo, rhi);
            const int64_t b = max((int64_t)rlo, a.nu_begin), e = min((int64_t)rhi, a.nu_begin + a.nu_count);
            if (e > b) {
                wide = hw > kTanWide;
                lo = wide ? -1 - (int)b : (int)b;
                hi = (int)e;
            }
        }
        w.win_lo[(size_t)d * a.n_lines + l] = lo;
        w.win_hi[(size_t)d * a.n_lines + l] = hi;
    }
    int total;
    tan_block_rank(wide, s_cnt, total);
    if (threadIdx.x == 0) w.chunk[(size_t)d * w.n_chunks + blockIdx.x] = total;
}

__global__ __launch_bounds__(64) void k_line_tangent_scan(TanWork w)
{
    const int d = blockIdx.x, lane = threadIdx.x;
    int* const c = w.chunk + (size_t)d * w.n_chunks;
    int base = 0;
    for (int k0 = 0; k0 < w.n_chunks; k0 += 64) {  // (uniform)
        const int k = k0 + lane;
        const int v = k < w.n_chunks ? c[k] : 0;
        int inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inc, off);
            if (lane >= off) inc += t;
        }
        if (k < w.n_chunks) c[k] = base + inc - v;
        base += __shfl(inc, 63);
    }
    if (lane == 0) w.n_wide[d] = base;
}

__global__ __launch_bounds__(kBlock) void k_line_tangent_list(AdjLines a, TanWork w)
{
    __shared__ int s_cnt[kBlock / 64];
    const int d = blockIdx.y;
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool wide = l < a.n_lines && w.win_lo[(size_t)d * a.n_lines + l] < 0;
    int total;
    const int rank = tan_block_rank(wide, s_cnt, total);
    if (wide) w.list[(size_t)d * a.n_lines + w.chunk[(size_t)d * w.n_chunks + blockIdx.x] + rank] = (int)l;
}

// first l in [0, n) with centre[l] <= v, n if there is none; centre[] does not ascend.  All 64 lanes probe: log64(n) dependent loads.
__device__ __forceinline__ int64_t tan_first_le(const int* __restrict__ centre, int64_t n, int64_t v, int lane)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {  // (uniform)
        const int64_t step = (hi - lo + 63) >> 6;
        const int64_t idx = lo + lane * step;
        const int k = __popcll(__ballot(idx < hi && centre[idx] > v));  // the probes in front of the answer: lanes 0 ... k - 1
        if (k == 0) break;
        hi = min(hi, lo + k * step);
        lo += (k - 1) * step + 1;
    }
    return lo;
}

// a lane's value at the wave-uniform lane k
__device__ __forceinline__ double tan_bcast(double v, int k)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// kGrad = false: strength is the only direction — the term alone, by voigt_term as the line kernels evaluate it, one FMA per point
template <bool kGrad>
__global__ __launch_bounds__(kBlock) void k_line_tangent(AdjLines a, TanDirs dir, TanWork w, double* __restrict__ out, int64_t out_ld, int n_tiles)
{
    constexpr int P = kTanP, kTile = kTanTile;
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * (kBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = (int)(wid / n_tiles);
    if (d >= a.n_depth) return;
    const int t = (int)(wid - (int64_t)d * n_tiles);
    const int64_t base = a.nu_begin + (int64_t)t * kTile;
    const int64_t tile_end = min(base + kTile, a.nu_begin + a.nu_count);
    const bool whole = tile_end == base + kTile;
    const double nu_first = a.nus[base], nu_last = a.nus[tile_end - 1];  // (the grid descends)
    double nu[P], acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int64_t i = base + p * 64 + lane;
        nu[p] = i < tile_end ? a.nus[i] : 0.0;
        acc[p] = 0.0;
    }
    if (a.n_lines > 0) {
        const int* __restrict__ lo_row = w.win_lo + (size_t)d * a.n_lines;
        const int* __restrict__ hi_row = w.win_hi + (size_t)d * a.n_lines;
        const int* __restrict__ list = w.list + (size_t)d * a.n_lines;
        // the other items reach at most kTanWide points from their centre index
        const int64_t l0 = tan_first_le(w.centre, a.n_lines, tile_end + kTanWide, lane);
        const int64_t l1 = tan_first_le(w.centre, a.n_lines, base - kTanWide - 1, lane);
        for (int seg = 0; seg < 2; ++seg) {
            const int64_t first = seg ? l0 : 0, last = seg ? l1 : w.n_wide[d];
            for (int64_t e0 = first; e0 < last; e0 += 64) {  // (uniform)
                const int64_t e = e0 + lane;
                int64_t l = 0;
                int lo = -1, hi = 0;
                if (e < last) {
                    l = seg ? e : list[e];
                    lo = lo_row[l], hi = hi_row[l];
                    if (!seg) lo = -1 - lo;  // (the list holds wide items only; in the range they stay negative and are passed over)
                }
                const bool hit = lo >= 0 && hi > base && lo < tile_end;
                // the constants of the 64 candidates side by side, each hit in its own lane: one round of loads and one reciprocal
                // for all of them, where a walk that formed them hit by hit would wait for every item's loads in turn
                double lnu = 0.0, inv = 0.0, y = 0.0, amp = 0.0, ct = 0.0, cy = 0.0, cxx = 0.0, cx = 0.0;
                RegionIGrad k1 = {0.0, 0.0, 0.0, 0.0};
                bool wing = false;
                if (hit) {
                    const size_t item = (size_t)l * a.n_depth + d, kd = (size_t)l * dir.cols + (dir.cols == 1 ? 0 : d);
                    lnu = a.line_nus[l];
                    narrow_params(a.doppler[item], a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)], a.alphas[item], inv, y, amp);
                    k1 = region1_grad_setup(y, amp);
                    const double da = dir.strength ? dir.strength[kd] : 0.0, dg = dir.damping ? dir.damping[kd] : 0.0;
                    const double db = dir.doppler ? dir.doppler[kd] : 0.0, dn = dir.centre ? dir.centre[kd] : 0.0;
                    // a T + g y Ty - b (T + x Tx + y Ty) - n Tx / dw  =  ct T + cy Ty + cxx (x Tx) + cx Tx
                    ct = da - db, cy = (dg - db) * y, cxx = -db, cx = -(dn * inv);
                    // A whole tile inside the window and in the line's far wing — k_line_adjoint_tiled's condition — needs no test per
                    // point: every point then passes voigt_grad_x's own test, and region1_grad is what it evaluates (the same bits).
                    wing = whole && lo <= base && hi >= base + kTile && (lnu > nu_first || lnu < nu_last) &&
                           add_rn(fabs((nu_first - lnu) * inv), y) > 15.0 && add_rn(fabs((nu_last - lnu) * inv), y) > 15.0;
                }
                unsigned long long hits = __ballot(hit);
                const unsigned long long wings = __ballot(wing);
                while (hits) {  // (uniform) ascending
                    const int k = __builtin_ctzll(hits);
                    hits &= hits - 1;
                    const double s_lnu = tan_bcast(lnu, k), s_inv = tan_bcast(inv, k), s_ct = tan_bcast(ct, k), s_cy = tan_bcast(cy, k);
                    const double s_cxx = tan_bcast(cxx, k), s_cx = tan_bcast(cx, k);
                    const RegionIGrad s_k1 = {tan_bcast(k1.yk, k), tan_bcast(k1.c, k), tan_bcast(k1.cv, k), tan_bcast(k1.cd, k)};
                    if ((wings >> k) & 1) {
#pragma unroll
                        for (int p = 0; p < P; ++p) {
                            const double x = (nu[p] - s_lnu) * s_inv;
                            if constexpr (kGrad) {
                                double tt, tx, ty;
                                region1_grad(x, s_k1, tt, tx, ty);
                                acc[p] = add_rn(acc[p], fma(s_ct, tt, fma(s_cy, ty, fma(s_cxx, x * tx, s_cx * tx))));
                            } else {
                                acc[p] = fma(s_ct, region1_add(0.0, x, RegionI{s_k1.yk, s_k1.cv, s_k1.cd}), acc[p]);
                            }
                        }
                    } else {
                        const double s_y = tan_bcast(y, k), s_amp = tan_bcast(amp, k);
                        const int b = __builtin_amdgcn_readlane(lo, k), we = __builtin_amdgcn_readlane(hi, k);
                        const unsigned len = (unsigned)(we - b);
                        const int rel0 = (int)(base + lane - b);  // (negative: in front of the window, far above len as an unsigned number)
#pragma unroll
                        for (int p = 0; p < P; ++p)
                            if ((unsigned)(rel0 + p * 64) < len) {
                                if constexpr (kGrad) {
                                    const double x = (nu[p] - s_lnu) * s_inv;
                                    double tt, tx, ty;
                                    voigt_grad_x(x, s_y, s_amp, s_k1, tt, tx, ty);
                                    acc[p] = add_rn(acc[p], fma(s_ct, tt, fma(s_cy, ty, fma(s_cxx, x * tx, s_cx * tx))));
                                } else {
                                    acc[p] = fma(s_ct, voigt_term(nu[p] - s_lnu, s_inv, s_y, s_amp, RegionI{s_k1.yk, s_k1.cv, s_k1.cd}), acc[p]);
                                }
                            }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int64_t i = base + p * 64 + lane;
        if (i < tile_end) out[(size_t)d * out_ld + (i - a.nu_begin)] = acc[p];
    }
}

// voigt_grad_x element-wise, the sibling of k_voigt_term: amp K, amp K_x, amp K_y at x = delta_nu * inv_dw with the routine's own region
// tests (tests/test_gpu_voigt_grad.py judges it point by point)
__global__ __launch_bounds__(kBlock) void k_voigt_grad(int64_t n, const double* __restrict__ dnu, const double* __restrict__ inv_dw,
                                                       const double* __restrict__ y, const double* __restrict__ amp, double* __restrict__ out_k,
                                                       double* __restrict__ out_kx, double* __restrict__ out_ky)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const RegionIGrad k1 = region1_grad_setup(y[i], amp[i]);
    double t, tx, ty;
    voigt_grad_x(dnu[i] * inv_dw[i], y[i], amp[i], k1, t, tx, ty);
    out_k[i] = t, out_kx[i] = tx, out_ky[i] = ty;
}

// ------------------------------------------------------------------------------------------------
// Isolated-line equivalent widths (sdx_line_equivalent_widths_dev; the definition stands in include/stardis_hip.h).  An ITEM is a
// (selected line j, strength factor k) pair, item = j * n_scale + k; its line's opacities are alpha' = mul_rn(alpha, s) at every depth.
//   k_line_adjoint_setup  the grid spacing and the centres of all lines (the adjoints' kernel, their scratch head)
//   k_ew_plan    one thread per item: window_rule on the global grid with alpha' at every depth -> the union [ulo, uhi) (every window
//                holds the centre's neighbourhood, so the union is an interval: the smallest lower and the largest upper bound), and
//                the number of work units of the item: segments of kEwSegment points of the union clipped to the shard
//   k_ew_scan    one block: the exclusive prefix sum of the unit counts -> uoff [items + 1].  Unit u of item t is segment u - uoff[t]:
//                the lists follow from the tables, the selection and the shard alone (no atomics anywhere)
//   k_ew_walk    a workgroup per unit (blocks stride the units; the item of a unit by bisection of uoff).  The block stages the item's
//                per-depth constants once (EwColumns), then every wave takes gpw points of the segment at a time: lane <-> (point,
//                angle) as k_raytrace_cont; the lanes of a point stage its column — voigt_term inside the depth's window, +0 outside,
//                A = add_rn(B, term), sqrt(A), sqrt(B), the Planck source — and walk the two recurrences, total and background, on
//                the same ray lengths and source values with the same rt_coef operations.  One theta-sum per chain at the end, in
//                k_raytrace's order (two ascending halves); r = (F_B - F) / F_B, the node weight h, and the term h r and r into the
//                segment's slots.  Wave 0 closes the unit: lane p adds slots p, p + 64, p + 128, p + 192 in this order, a
//                butterfly (offsets 32 ... 1) adds the lanes; the maximum of r likewise -> partial[u]
//   k_ew_gather  one thread per item: the units in ascending order, add_rn for W, fmax for the depth; no unit: both 0.0
// An index of line_index outside [0, n_lines) is clamped here (no access out of bounds); the Python layer refuses it before upload.
struct EwArgs {
    int n_depth, gamma_cols, n_scale, n_theta;
    int64_t n_nu, nu_begin, nu_count, n_lines, n_sel;
    const double *nus, *x, *line_nus, *doppler, *gammas, *alphas;
    const int64_t* line_index;  // [n_sel] or null: line j
    const double* scale;        // [n_sel][n_scale] or null: 1.0
    const double* background;   // [n_depth][bld], column 0 at nu_begin
    int64_t bld;
    const double *temps, *ray_dist, *wts;
};
struct EwWork {
    const double* pd;   // [0] = d_nu, [1] = 1 / d_nu (k_line_adjoint_setup)
    const int* centre;  // [N_l] (k_line_adjoint_setup)
    int* ulo;           // [items] the union of the item's windows, unclipped
    int* uhi;
    int* uoff;          // [items + 1] the item's first unit
    double2* partial;   // [units] (W, depth) of a unit
};

__device__ __forceinline__ int64_t ew_line(const EwArgs& a, int64_t j)
{
    const int64_t l = a.line_index ? a.line_index[j] : j;
    return l < 0 ? 0 : (l >= a.n_lines ? a.n_lines - 1 : l);
}

__global__ __launch_bounds__(kBlock) void k_ew_plan(EwArgs a, EwWork w)
{
    const int64_t n_items = a.n_sel * a.n_scale;
    const int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (item >= n_items) return;
    const int64_t j = item / a.n_scale;
    const int64_t l = ew_line(a, j);
    const double s = a.scale ? a.scale[item] : 1.0;
    const double d_nu = w.pd[0], r_dnu = w.pd[1];
    const int c = w.centre[l];
    int ulo = 2147483647, uhi = 0;
    for (int d = 0; d < a.n_depth; ++d) {
        int lo, hi;
        window_rule(c, a.n_nu, d_nu, r_dnu, a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)], a.doppler[l * a.n_depth + d],
                    mul_rn(a.alphas[l * a.n_depth + d], s), lo, hi);
        ulo = min(ulo, lo), uhi = max(uhi, hi);
    }
    w.ulo[item] = ulo, w.uhi[item] = uhi;
    const int64_t b = max((int64_t)ulo, a.nu_begin), e = min((int64_t)uhi, a.nu_begin + a.nu_count);
    w.uoff[item] = e > b ? (int)((e - b + kEwSegment - 1) / kEwSegment) : 0;
}

// counts in uoff[0 .. n) -> their exclusive prefix sums in place, the total in uoff[n]; one block of kPreBlock threads, a run of
// consecutive items per thread
__global__ __launch_bounds__(kPreBlock) void k_ew_scan(int64_t n, int* __restrict__ uoff)
{
    __shared__ int s_sum[kPreBlock];
    const int tid = threadIdx.x;
    const int64_t per = (n + kPreBlock - 1) / kPreBlock;
    const int64_t b = min(n, tid * per), e = min(n, b + per);
    int sum = 0;
    for (int64_t i = b; i < e; ++i) sum += uoff[i];
    s_sum[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kPreBlock; off <<= 1) {
        const int below = tid >= off ? s_sum[tid - off] : 0;
        __syncthreads();
        s_sum[tid] += below;
        __syncthreads();
    }
    int run = s_sum[tid] - sum;
    for (int64_t i = b; i < e; ++i) {
        const int cnt = uoff[i];
        uoff[i] = run;
        run += cnt;
    }
    if (tid == kPreBlock - 1) uoff[n] = s_sum[tid];
}

__global__ __launch_bounds__(kRtBlock) void k_ew_walk(EwArgs a, EwWork w, int G, int gpw)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = lane / G, g = lane - grp * G;
    const bool active = grp < gpw;
    const int n_depth = a.n_depth, n_gap = n_depth - 1, col = n_depth, n_theta = a.n_theta;
    const EwColumns L(G, n_depth, gpw);  // (sdx_rt_layout.h: the host sizes the launch by the same struct)
    int2* cW = (int2*)(smem + L.window());
    double* cInv = smem + L.inv();
    double* cY = smem + L.y();
    double* cAmp = smem + L.amp();
    double* cYk = smem + L.region1();
    double* cCv = cYk + col;
    double* cCd = cCv + col;
    double* sT = smem + L.terms();
    double* sR = smem + L.ratios();
    double* wbase = smem + L.shared_doubles() + (size_t)wave * L.wave_doubles();
    double2* sP = (double2*)(wbase + L.pairs());  // (source function, sqrt(alpha total)) [gpw][col]
    double* sC = wbase + L.back();                // sqrt(alpha background)             [gpw][col]
    double* sX = wbase + L.flux();                // emergent flux terms, total         [gpw][G]
    double* sXc = wbase + L.flux_back();          // emergent flux terms, background    [gpw][G]
    const int64_t n_items = a.n_sel * a.n_scale;
    const int n_units = w.uoff[n_items];
    const RtConst kc = rt_const_literals();  // (literals, as in k_raytrace)
    const int th = min(g, n_theta - 1);
    const double wt = g < n_theta ? a.wts[th] : 0.0;
    const int gi = (active ? grp : 0) * col;
    const int half = (n_theta + 1) >> 1;

    for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
        int64_t item = 0;
        {  // the last item whose first unit is not behind u (items without units share the offset of the next one with units)
            int64_t hi = n_items;
            while (hi - item > 1) {
                const int64_t mid = (item + hi) >> 1;
                if (w.uoff[mid] <= u) item = mid; else hi = mid;
            }
        }
        const int seg = u - w.uoff[item];
        const int64_t l = ew_line(a, item / a.n_scale);
        const double s = a.scale ? a.scale[item] : 1.0;
        const int64_t ulo = w.ulo[item], uhi = w.uhi[item];
        const int64_t ue = min(uhi, a.nu_begin + a.nu_count);
        const int64_t sb = max(ulo, a.nu_begin) + (int64_t)seg * kEwSegment;
        const int len = (int)min((int64_t)kEwSegment, ue - sb);
        const double lnu = a.line_nus[l];

        __syncthreads();  // the unit before: its constants and slots are read no more
        for (int d = tid; d < n_depth; d += kRtBlock) {
            const double dw = a.doppler[l * n_depth + d], gm = a.gammas[l * a.gamma_cols + (a.gamma_cols == 1 ? 0 : d)];
            const double al = mul_rn(a.alphas[l * n_depth + d], s);
            int lo, hi;
            window_rule(w.centre[l], a.n_nu, w.pd[0], w.pd[1], gm, dw, al, lo, hi);
            double inv, y, amp;
            narrow_params(dw, gm, al, inv, y, amp);
            const RegionI k1 = region1_setup(y, amp);
            cW[d] = int2{lo, hi};
            cInv[d] = inv, cY[d] = y, cAmp[d] = amp, cYk[d] = k1.yk, cCv[d] = k1.cv, cCd[d] = k1.cd;
        }
        __syncthreads();

        for (int p0 = wave * gpw; p0 < len; p0 += kRtWaves * gpw) {
            const int64_t i = sb + min(p0 + grp, len - 1);  // (lanes behind the segment's end repeat its last point and are not read)
            const double nu = a.nus[i];
            if (active) {
                const int ii = (int)i;
                const double delta = nu - lnu;
                for (int d = g; d < n_depth; d += G) {
                    const double ab = a.background[(size_t)d * a.bld + (i - a.nu_begin)];
                    const int2 win = cW[d];
                    double term = 0.0;
                    if (ii >= win.x && ii < win.y) term = voigt_term(delta, cInv[d], cY[d], cAmp[d], RegionI{cYk[d], cCv[d], cCd[d]});
                    sP[grp * col + d] = double2{planck_staged(nu, a.temps[d]), sqrt(add_rn(ab, term))};
                    sC[grp * col + d] = sqrt(ab);
                }
            }
            wave_sync();

            // the outward walk of k_raytrace_cont: two chains on the same ray lengths and source values
            double inten = 0.0, intc = 0.0;
            const double2 q0 = sP[gi], q1 = sP[gi + 1];
            double a1 = q1.y, ac1 = sC[gi + 1];
            const double* rdp = a.ray_dist + th;
            double tau0 = mul_rn(q0.y * a1, *rdp), tauc0 = mul_rn(sC[gi] * ac1, *rdp);
            rdp += n_gap > 1 ? n_theta : 0;
            double rd_next = *rdp;
            double s1 = q1.x, d10 = q0.x - s1;
            for (int gap = 0; gap < n_gap - 1; ++gap) {
                const double2 q2 = sP[gi + gap + 2];
                const double s2 = q2.x, a2 = q2.y, ac2 = sC[gi + gap + 2];
                const double mean1 = a1 * a2, meanc1 = ac1 * ac2, d21 = s2 - s1;
                const double rd = rd_next;
                const double t1 = mul_rn(mean1, rd), tc1 = mul_rn(meanc1, rd);
                rdp += gap + 2 < n_gap ? n_theta : 0;
                rd_next = *rdp;
                double c, e, cc, ec;
                rt_coef<false>(tau0, t1, d10, d21, s1, c, e, kc);
                rt_coef<false>(tauc0, tc1, d10, d21, s1, cc, ec, kc);
                inten = fma(c, inten, e), intc = fma(cc, intc, ec);
                tau0 = t1, tauc0 = tc1;
                d10 = -d21, s1 = s2, a1 = a2, ac1 = ac2;
            }
            {
                double c, e, cc, ec;
                rt_coef<true>(tau0, 0.0, d10, 0.0, s1, c, e, kc);
                rt_coef<true>(tauc0, 0.0, d10, 0.0, s1, cc, ec, kc);
                inten = fma(c, inten, e), intc = fma(cc, intc, ec);
            }
            if (active) sX[grp * G + g] = inten * wt, sXc[grp * G + g] = intc * wt;
            wave_sync();
            if (lane < gpw && p0 + lane < len) {
                const double* c = sX + lane * G;
                const double* cc = sXc + lane * G;
                double f0 = 0.0, f1 = 0.0, b0 = 0.0, b1 = 0.0;
                for (int t = 0; t < half; ++t) f0 = add_rn(f0, c[t]), b0 = add_rn(b0, cc[t]);
                for (int t = half; t < n_theta; ++t) f1 = add_rn(f1, c[t]), b1 = add_rn(b1, cc[t]);
                const double F = add_rn(f0, f1), Fb = add_rn(b0, b1);
                const double r = (Fb - F) / Fb;
                const int64_t ip = sb + p0 + lane;
                const double xi = a.x[ip];
                const double right = ip + 1 < uhi ? fabs(a.x[ip + 1] - xi) : 0.0, left = ip - 1 >= ulo ? fabs(xi - a.x[ip - 1]) : 0.0;
                const double h = mul_rn(0.5, add_rn(right, left));
                sT[p0 + lane] = mul_rn(h, r);
                sR[p0 + lane] = r;
            }
            wave_sync();
        }
        __syncthreads();
        if (wave == 0) {
            double sum = 0.0, top = -__builtin_huge_val();
#pragma unroll
            for (int q = 0; q < kEwSegment / 64; ++q) {
                const int p = lane + 64 * q;
                if (p < len) sum = add_rn(sum, sT[p]), top = fmax(top, sR[p]);
            }
            for (int off = 32; off > 0; off >>= 1) sum = add_rn(sum, __shfl_xor(sum, off)), top = fmax(top, __shfl_xor(top, off));
            if (lane == 0) w.partial[u] = double2{sum, top};
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_ew_gather(int64_t n_items, EwWork w, double* __restrict__ out_W, double* __restrict__ out_depth)
{
    const int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (item >= n_items) return;
    const int b = w.uoff[item], e = w.uoff[item + 1];
    double sum = 0.0, top = 0.0;
    for (int u = b; u < e; ++u) {
        const double2 p = w.partial[u];
        sum = add_rn(sum, p.x);
        top = u == b ? p.y : fmax(top, p.y);
    }
    if (out_W) out_W[item] = sum;
    if (out_depth) out_depth[item] = top;
}

}  // namespace sdx
