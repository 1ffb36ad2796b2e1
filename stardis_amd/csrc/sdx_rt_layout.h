// sdx_rt_layout.h — the dynamic-LDS layouts of the formal-solution kernels (sdx_kernels.h), each stated ONCE: the kernel takes its
// region offsets from the struct, the host (stardis_hip.hip) takes the launch's byte count and chooses the launch shape from it.
// Offsets and sizes are ints, as the kernels index; the host's helpers below keep them exact by refusing, before any arithmetic, a
// model whose single column is larger than LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

constexpr int kRtBlock = 256;             // k_raytrace, k_raytrace_cont, k_raytrace_f32, k_contribution: four waves
constexpr int kRtWaves = kRtBlock / 64;
constexpr size_t kLdsBytes = 64 * 1024;   // what a workgroup may ask for

constexpr int kRtBatch = 4;  // gaps per flux reduction of k_raytrace, k_raytrace_cont and k_contribution
// k_raytrace, k_contribution.  Per wave: the (source function, sqrt(alpha)) pairs [gpw][col] as double2, then the flux terms
// [kRtBatch][gpw][G] of a batch of gaps.  G lanes per frequency, one angle per lane, gpw frequencies per wave.
// k_emergent_intensity takes the same layout (k_raytrace's budget decides what it serves) and parks its [gpw][G] emergent intensities
// in the first of the flux slots for the theta-major write.
struct RtColumns {
    int gpw, col, G;
    __host__ __device__ constexpr RtColumns(int G_, int n_depth, int gpw_) : gpw(gpw_), col(n_depth), G(G_) {}
    __host__ __device__ constexpr int pairs() const { return 0; }
    __host__ __device__ constexpr int flux() const { return 2 * gpw * col; }
    __host__ __device__ constexpr int wave_doubles() const { return flux() + kRtBatch * gpw * G; }
    __host__ __device__ constexpr size_t bytes() const { return (size_t)kRtWaves * wave_doubles() * sizeof(double); }
};

// k_raytrace_cont: RtColumns with sqrt(alpha continuum) [gpw][col] behind the pairs and a second batch of flux terms for the
// continuum chain; a wave's share is rounded up to an even number of doubles, so that every wave's pairs stay 16-byte aligned.
struct RtContColumns {
    int gpw, col, G;
    __host__ __device__ constexpr RtContColumns(int G_, int n_depth, int gpw_) : gpw(gpw_), col(n_depth), G(G_) {}
    __host__ __device__ constexpr int pairs() const { return 0; }
    __host__ __device__ constexpr int cont() const { return 2 * gpw * col; }
    __host__ __device__ constexpr int flux() const { return cont() + gpw * col; }
    __host__ __device__ constexpr int flux_cont() const { return flux() + kRtBatch * gpw * G; }
    __host__ __device__ constexpr int wave_doubles() const { return (flux_cont() + kRtBatch * gpw * G + 1) & ~1; }
    __host__ __device__ constexpr size_t bytes() const { return (size_t)kRtWaves * wave_doubles() * sizeof(double); }
};

// k_ew_walk (isolated-line equivalent widths): a workgroup walks one segment of kEwSegment window points of one (line, strength) item.
// Shared by the block, one array [col] each (a lane staging depth d reads entry d of each: consecutive lanes, consecutive 8 bytes):
// the depth's window [lo, hi) as two ints in one slot, 1 / doppler width, y, the amplitude, the three region-I constants; then the
// segment's terms h r and ratios r [kEwSegment] each.  Then per wave RtContColumns' columns — the (source function, sqrt(alpha total))
// pairs [gpw][col] as double2, sqrt(alpha background) [gpw][col] — and ONE set of flux terms per chain [gpw][G]: only the emergent flux
// is summed.  Every region that holds double2 starts at an even double.
constexpr int kEwSegment = 256;  // window points per work unit of k_ew_walk
struct EwColumns {
    int gpw, col, G;
    __host__ __device__ constexpr EwColumns(int G_, int n_depth, int gpw_) : gpw(gpw_), col(n_depth), G(G_) {}
    __host__ __device__ constexpr int window() const { return 0; }
    __host__ __device__ constexpr int inv() const { return col; }
    __host__ __device__ constexpr int y() const { return 2 * col; }
    __host__ __device__ constexpr int amp() const { return 3 * col; }
    __host__ __device__ constexpr int region1() const { return 4 * col; }  // yk, cv, cd: [3][col]
    __host__ __device__ constexpr int terms() const { return (7 * col + 1) & ~1; }
    __host__ __device__ constexpr int ratios() const { return terms() + kEwSegment; }
    __host__ __device__ constexpr int shared_doubles() const { return ratios() + kEwSegment; }
    __host__ __device__ constexpr int pairs() const { return 0; }  // (this and the next three: from the wave's base)
    __host__ __device__ constexpr int back() const { return 2 * gpw * col; }
    __host__ __device__ constexpr int flux() const { return back() + gpw * col; }
    __host__ __device__ constexpr int flux_back() const { return flux() + gpw * G; }
    __host__ __device__ constexpr int wave_doubles() const { return (flux_back() + gpw * G + 1) & ~1; }
    __host__ __device__ constexpr size_t bytes() const { return ((size_t)shared_doubles() + (size_t)kRtWaves * wave_doubles()) * sizeof(double); }
};

// k_raytrace_f32 (floats).  Shared by the block: the ray table [n_gap][n_theta], 1 / (k T) [col] and the relative temperature
// differences [col], rounded up to whole float4s; then per wave the float4 of every point [gpw][col] and the flux terms [batch][gpw][G].
constexpr int kRt32Batch = 8;  // gaps per flux reduction of k_raytrace_f32 (6 measured: no gain from the eighth block a CU's LDS then holds)
struct RtF32Columns {
    int n_gap, col, n_theta, G, gpw;
    __host__ __device__ constexpr RtF32Columns(int n_theta_, int G_, int n_depth, int gpw_)
        : n_gap(n_depth - 1), col(n_depth), n_theta(n_theta_), G(G_), gpw(gpw_) {}
    __host__ __device__ constexpr int ray_table() const { return 0; }
    __host__ __device__ constexpr int inv_kt() const { return n_gap * n_theta; }
    __host__ __device__ constexpr int dtemp() const { return inv_kt() + col; }
    __host__ __device__ constexpr int shared_floats() const { return (dtemp() + col + 3) & ~3; }
    __host__ __device__ constexpr int points() const { return 0; }  // (this and flux(): from the wave's base)
    __host__ __device__ constexpr int flux() const { return 4 * gpw * col; }
    __host__ __device__ constexpr int wave_floats() const { return flux() + kRt32Batch * gpw * G; }
    __host__ __device__ constexpr size_t bytes() const { return ((size_t)shared_floats() + (size_t)kRtWaves * wave_floats()) * sizeof(float); }
};

// k_raytrace_seg<NS, LMAX>, k_raytrace_seg_step<NS, LMAX, ..>, per workgroup of NS waves and gpw = 64 / n_theta frequencies: the
// segment maps [NS][64][2]; the ray table TRANSPOSED [n_theta][rstride] with an odd row stride (the angles of a wave read distinct
// banks); the (source, sqrt(alpha)) pairs [gpw][col], 16-byte aligned.  After the barrier of step 2 the flux terms [NS][LMAX][gpw][G]
// reuse the space from the ray table on, so the launch asks for the larger of the two.
struct RtSegments {
    int NS, LMAX, n_theta, n_gap, col;
    __host__ __device__ constexpr RtSegments(int NS_, int LMAX_, int n_theta_, int n_depth)
        : NS(NS_), LMAX(LMAX_), n_theta(n_theta_), n_gap(n_depth - 1), col(n_depth) {}
    __host__ __device__ constexpr int gpw() const { return 64 / n_theta; }
    __host__ __device__ constexpr int segment() const { return (n_gap + NS - 1) / NS; }  // gaps per wave
    __host__ __device__ constexpr int rstride() const { return n_gap | 1; }
    __host__ __device__ constexpr int maps() const { return 0; }
    __host__ __device__ constexpr int ray_table() const { return NS * 128; }
    __host__ __device__ constexpr int pairs_from_table() const { return (n_theta * rstride() + 1) & ~1; }
    __host__ __device__ constexpr int pairs() const { return ray_table() + pairs_from_table(); }
    __host__ __device__ constexpr int flux() const { return ray_table(); }
    __host__ __device__ constexpr int staging_end() const { return pairs() + 2 * gpw() * col; }
    __host__ __device__ constexpr int flux_end() const { return flux() + NS * LMAX * gpw() * n_theta; }
    __host__ __device__ constexpr int doubles() const { return staging_end() > flux_end() ? staging_end() : flux_end(); }
    __host__ __device__ constexpr size_t bytes() const { return (size_t)doubles() * sizeof(double); }
    // (what keeps a wave's gaps inside its LMAX register slots; the host checks it beside bytes())
    __host__ __device__ constexpr bool segment_fits() const { return segment() <= LMAX; }
};

// k_response: a workgroup of ONE wave (kRespBlock lanes).  RtColumns' pairs [gpw][col] as double2; then the stash of the forward walk,
// the intensity entering every gap per ray [col - 1][gpw * G] (a ray's slot is group * G + angle: consecutive lanes, consecutive
// doubles); then the terms of a batch of rows for each of the two outputs, [2][kRtBatch][gpw][G].  At 56 depth points and 20 angles
// that is 32.2 KB per wave — four waves of it do not fit the 64 KB a workgroup may ask for, hence the block size of its own.
constexpr int kRespBlock = 64;
constexpr int kRespWaves = kRespBlock / 64;
struct RtResponse {
    int gpw, col, G;
    __host__ __device__ constexpr RtResponse(int G_, int n_depth, int gpw_) : gpw(gpw_), col(n_depth), G(G_) {}
    __host__ __device__ constexpr int pairs() const { return 0; }
    __host__ __device__ constexpr int slots() const { return gpw * G; }  // rays of a wave
    __host__ __device__ constexpr int stash() const { return 2 * gpw * col; }
    __host__ __device__ constexpr int terms_alpha() const { return stash() + (col - 1) * slots(); }
    __host__ __device__ constexpr int terms_source() const { return terms_alpha() + kRtBatch * slots(); }
    __host__ __device__ constexpr int wave_doubles() const { return (terms_source() + kRtBatch * slots() + 1) & ~1; }
    __host__ __device__ constexpr size_t bytes() const { return (size_t)kRespWaves * wave_doubles() * sizeof(double); }
};

// k_lambda<kIterate> (mean intensity, and the scattering source iteration).  Per wave: RtColumns' pairs [gpw][col] as double2 — the
// source column is the ITERATE, rewritten in place —; then four columns [gpw][col] each: the thermal term (1 - albedo) B, the albedo,
// the diagonal (the iteration turns it into 1 / (1 - albedo clamp(L))) and the mean intensity J (between the sweeps and the update it
// holds the change of the iterate); then the terms of a batch of rows [kRtBatch][gpw][G], which also serve the per-column maxima of
// the stopping rule ([2][gpw][G]).  A column's whole iteration lives in these bytes: the block size follows from them (lambda_waves),
// bytes() is ONE wave's share.
struct RtLambda {
    int gpw, col, G;
    __host__ __device__ constexpr RtLambda(int G_, int n_depth, int gpw_) : gpw(gpw_), col(n_depth), G(G_) {}
    __host__ __device__ constexpr int pairs() const { return 0; }
    __host__ __device__ constexpr int thermal() const { return 2 * gpw * col; }
    __host__ __device__ constexpr int albedo() const { return thermal() + gpw * col; }
    __host__ __device__ constexpr int diag() const { return albedo() + gpw * col; }
    __host__ __device__ constexpr int mean() const { return diag() + gpw * col; }
    __host__ __device__ constexpr int terms() const { return mean() + gpw * col; }
    __host__ __device__ constexpr int wave_doubles() const { return (terms() + kRtBatch * gpw * G + 1) & ~1; }
    __host__ __device__ constexpr size_t bytes() const { return (size_t)wave_doubles() * sizeof(double); }
};

// k_lambda_ng (k_lambda<true> with Ng acceleration).  RtLambda's regions in RtLambda's order; then the
// history [4][gpw][col]: slots 0..2 are a ring over the three iterates before the current one (an update writes the iterate it
// replaces into the slot the trip count selects: one extra column write), slot 3 is the copy of the iterate an extrapolation replaced,
// which the safeguard may take back; then the terms [kRtBatch + 1][gpw][G]: RtLambda's batch of rows and maxima, and the G partials of each
// of the extrapolation's five sums per column ([5][gpw][G]: the per-column scalars pass through LDS in lane order).  bytes() is ONE
// wave's share, as RtLambda's.
constexpr int kNgHistory = 4;  // ring of three and the safeguard's copy
constexpr int kNgSums = 5;     // A1, B1, C1, B2, C2
struct RtLambdaNg {
    int gpw, col, G;
    __host__ __device__ constexpr RtLambdaNg(int G_, int n_depth, int gpw_) : gpw(gpw_), col(n_depth), G(G_) {}
    __host__ __device__ constexpr int pairs() const { return 0; }
    __host__ __device__ constexpr int thermal() const { return 2 * gpw * col; }
    __host__ __device__ constexpr int albedo() const { return thermal() + gpw * col; }
    __host__ __device__ constexpr int diag() const { return albedo() + gpw * col; }
    __host__ __device__ constexpr int mean() const { return diag() + gpw * col; }
    __host__ __device__ constexpr int history(int slot) const { return mean() + (1 + slot) * gpw * col; }
    __host__ __device__ constexpr int terms() const { return history(kNgHistory); }
    __host__ __device__ constexpr int wave_doubles() const { return (terms() + (kRtBatch + 1) * gpw * G + 1) & ~1; }
    __host__ __device__ constexpr size_t bytes() const { return (size_t)wave_doubles() * sizeof(double); }
};

// k_lambda_adjoint<kSolve> (the transposed mean-intensity operator, its opacity derivative, and the adjoint scattering solve).  Per
// wave: RtColumns' pairs [gpw][col] as double2 (the source column S the derivative is taken at, sqrt(alpha)); then eight columns
// [gpw][col] each: z (what the transposed operator is applied to; in the solve albedo y), the result Lambda^T z, the iterate y, the
// cotangent, the albedo, the diagonal (the solve turns it into 1 / (1 - albedo clamp(L))), the mean intensity J of S, and the opacity
// derivative G; then k_response's stash of the forward sweep, the value entering every step per ray [col - 1][gpw * G], reused by the
// second sweep; then the terms of a batch of rows [kRtBatch][gpw][G], which also serve the maxima of the stopping rule ([2][gpw][G]).
// One wave's share at one frequency: ((n_theta + 10) n_depth + 3 n_theta) doubles.  bytes() is ONE wave's share; waves() and blocks()
// are the launch: as many shares as 64 KB hold, at most kRtWaves.
struct RtLambdaAdjoint {
    int gpw, col, G;
    __host__ __device__ constexpr RtLambdaAdjoint(int G_, int n_depth, int gpw_) : gpw(gpw_), col(n_depth), G(G_) {}
    __host__ __device__ constexpr int pairs() const { return 0; }
    __host__ __device__ constexpr int slots() const { return gpw * G; }  // rays of a wave
    __host__ __device__ constexpr int column(int n) const { return (2 + n) * gpw * col; }
    __host__ __device__ constexpr int z() const { return column(0); }
    __host__ __device__ constexpr int result() const { return column(1); }
    __host__ __device__ constexpr int iterate() const { return column(2); }
    __host__ __device__ constexpr int cotangent() const { return column(3); }
    __host__ __device__ constexpr int albedo() const { return column(4); }
    __host__ __device__ constexpr int diag() const { return column(5); }
    __host__ __device__ constexpr int mean() const { return column(6); }
    __host__ __device__ constexpr int gradient() const { return column(7); }
    __host__ __device__ constexpr int stash() const { return column(8); }
    __host__ __device__ constexpr int terms() const { return stash() + (col - 1) * slots(); }
    __host__ __device__ constexpr int wave_doubles() const { return (terms() + kRtBatch * slots() + 1) & ~1; }
    __host__ __device__ constexpr size_t bytes() const { return (size_t)wave_doubles() * sizeof(double); }
    int waves() const { return kLdsBytes / bytes() >= (size_t)kRtWaves ? kRtWaves : (int)(kLdsBytes / bytes()); }
    unsigned blocks(long long n_nu) const { return (unsigned)((n_nu + (long long)gpw * waves() - 1) / ((long long)gpw * waves())); }
};

// ---- the host's choice of a launch shape ----------------------------------------------------------------------------------------
// A model whose column alone is larger than LDS fits no layout; asked first, it also keeps every int above far from overflow.
constexpr int kRtMaxDepth = (int)(kLdsBytes / sizeof(double));
// Frequencies per wave of a per-wave layout (RtColumns, RtContColumns): 64 / G, lowered (idle lanes) until the staged columns fit LDS;
// 0 when not even one frequency per wave does.
template <class Layout>
inline int rt_fit_gpw(int G, int n_depth)
{
    if (n_depth > kRtMaxDepth) return 0;
    int gpw = 64 / G;
    while (gpw > 1 && Layout(G, n_depth, gpw).bytes() > kLdsBytes) --gpw;
    return Layout(G, n_depth, gpw).bytes() <= kLdsBytes ? gpw : 0;
}
// Workgroups of kRtBlock threads that cover n_nu frequencies at gpw frequencies per wave.
inline unsigned rt_blocks(long long n_nu, int gpw)
{
    return (unsigned)((n_nu + (long long)gpw * kRtWaves - 1) / ((long long)gpw * kRtWaves));
}

// Workgroups of kRespBlock threads (k_response) that cover n_nu frequencies at gpw frequencies per wave.
inline unsigned response_blocks(long long n_nu, int gpw)
{
    return (unsigned)((n_nu + (long long)gpw * kRespWaves - 1) / ((long long)gpw * kRespWaves));
}

// k_lambda: waves per workgroup — as many of RtLambda's shares as 64 KB hold, at most kRtWaves — and the workgroups that cover n_nu
// frequencies at gpw frequencies per wave (gpw from rt_fit_gpw<RtLambda>: one wave's share fits by then).
template <class Layout>
inline int lambda_waves_of(int G, int n_depth, int gpw)
{
    const size_t fit = kLdsBytes / Layout(G, n_depth, gpw).bytes();
    return fit >= (size_t)kRtWaves ? kRtWaves : (int)fit;
}
inline int lambda_waves(int G, int n_depth, int gpw) { return lambda_waves_of<RtLambda>(G, n_depth, gpw); }
inline unsigned lambda_blocks(long long n_nu, int gpw, int waves)
{
    return (unsigned)((n_nu + (long long)gpw * waves - 1) / ((long long)gpw * waves));
}

// ---- what the kernels rely on, at a few representative shapes --------------------------------------------------------------------
namespace rt_layout_checks {
constexpr bool even(int doubles) { return doubles % 2 == 0; }      // a double2 region: 16-byte aligned
constexpr bool quad(int floats) { return floats % 4 == 0; }        // a float4 region
constexpr bool columns_ok(int G, int n_depth, int gpw)
{
    const RtColumns a(G, n_depth, gpw);
    const RtContColumns c(G, n_depth, gpw);
    return a.pairs() + 2 * gpw * n_depth <= a.flux() && a.flux() + kRtBatch * gpw * G <= a.wave_doubles() && even(a.pairs()) && even(a.wave_doubles()) &&
           c.pairs() + 2 * gpw * n_depth <= c.cont() && c.cont() + gpw * n_depth <= c.flux() && c.flux() + kRtBatch * gpw * G <= c.flux_cont() &&
           c.flux_cont() + kRtBatch * gpw * G <= c.wave_doubles() && even(c.pairs()) && even(c.wave_doubles());
}
constexpr bool f32_ok(int n_theta, int n_depth)
{
    const RtF32Columns f(n_theta, n_theta, n_depth, 64 / n_theta);
    return f.ray_table() + f.n_gap * n_theta <= f.inv_kt() && f.inv_kt() + n_depth <= f.dtemp() && f.dtemp() + n_depth <= f.shared_floats() &&
           f.points() + 4 * f.gpw * n_depth <= f.flux() && f.flux() + kRt32Batch * f.gpw * f.G <= f.wave_floats() && quad(f.shared_floats()) && quad(f.points()) && quad(f.wave_floats());
}
constexpr bool segments_ok(int NS, int LMAX, int n_theta, int n_depth)
{
    const RtSegments s(NS, LMAX, n_theta, n_depth);
    return s.maps() + NS * 128 <= s.ray_table() && s.ray_table() + n_theta * s.rstride() <= s.pairs() && even(s.pairs()) && s.rstride() % 2 == 1 &&
           s.rstride() >= s.n_gap && s.flux() >= s.ray_table() && s.flux_end() <= s.doubles() && s.staging_end() <= s.doubles();
}
constexpr bool response_ok(int G, int n_depth, int gpw)
{
    const RtResponse r(G, n_depth, gpw);
    return gpw * G <= 64 && r.pairs() + 2 * gpw * n_depth <= r.stash() && r.stash() + (n_depth - 1) * r.slots() <= r.terms_alpha() &&
           r.terms_alpha() + kRtBatch * r.slots() <= r.terms_source() && r.terms_source() + kRtBatch * r.slots() <= r.wave_doubles() &&
           even(r.pairs()) && even(r.wave_doubles());
}
constexpr bool ew_ok(int G, int n_depth, int gpw)
{
    const EwColumns c(G, n_depth, gpw);
    return gpw * G <= 64 && c.region1() + 3 * n_depth <= c.terms() && c.terms() + kEwSegment <= c.ratios() && even(c.shared_doubles()) &&
           c.pairs() + 2 * gpw * n_depth <= c.back() && c.back() + gpw * n_depth <= c.flux() && c.flux() + gpw * G <= c.flux_back() &&
           c.flux_back() + gpw * G <= c.wave_doubles() && even(c.pairs()) && even(c.wave_doubles());
}
constexpr bool lambda_ok(int G, int n_depth, int gpw)
{
    const RtLambda l(G, n_depth, gpw);
    return gpw * G <= 64 && l.pairs() + 2 * gpw * n_depth <= l.thermal() && l.thermal() + gpw * n_depth <= l.albedo() &&
           l.albedo() + gpw * n_depth <= l.diag() && l.diag() + gpw * n_depth <= l.mean() && l.mean() + gpw * n_depth <= l.terms() &&
           l.terms() + kRtBatch * gpw * G <= l.wave_doubles() && 2 * gpw * G <= kRtBatch * gpw * G && even(l.pairs()) && even(l.wave_doubles());
}
constexpr bool lambda_adjoint_ok(int G, int n_depth, int gpw)
{
    const RtLambdaAdjoint l(G, n_depth, gpw);
    return gpw * G <= 64 && l.pairs() + 2 * gpw * n_depth <= l.z() && l.gradient() + gpw * n_depth <= l.stash() &&
           l.stash() + (n_depth - 1) * l.slots() <= l.terms() && l.terms() + kRtBatch * l.slots() <= l.wave_doubles() && 2 * l.slots() <= kRtBatch * l.slots() &&
           even(l.pairs()) && even(l.wave_doubles());
}
// the benchmark's shape (four waves of it fit a workgroup); odd depth and angle counts, both ends of the angle range; the deepest
// model at 20 angles and at one
static_assert(lambda_ok(20, 56, 3) && 4 * RtLambda(20, 56, 3).bytes() <= kLdsBytes, "RtLambda: four waves of 56 depth points at 20 angles must fit");
static_assert(lambda_ok(1, 2, 64) && lambda_ok(1, 3, 64) && lambda_ok(3, 3, 21) && lambda_ok(7, 9, 9) && lambda_ok(20, 57, 3) && lambda_ok(64, 40, 1), "RtLambda");
static_assert(RtLambda(20, 1352, 1).bytes() <= kLdsBytes && RtLambda(20, 1353, 1).bytes() > kLdsBytes && RtLambda(1, 1364, 1).bytes() <= kLdsBytes, "RtLambda");
constexpr bool lambda_ng_ok(int G, int n_depth, int gpw)
{
    const RtLambdaNg l(G, n_depth, gpw);
    const RtLambda p(G, n_depth, gpw);
    return gpw * G <= 64 && l.thermal() == p.thermal() && l.albedo() == p.albedo() && l.diag() == p.diag() && l.mean() == p.mean() &&
           l.mean() + gpw * n_depth <= l.history(0) && l.history(kNgHistory - 1) + gpw * n_depth <= l.terms() &&
           l.terms() + kNgSums * gpw * G <= l.wave_doubles() && l.terms() + kRtBatch * gpw * G <= l.wave_doubles() && even(l.pairs()) && even(l.wave_doubles());
}
// the accelerated iteration: the benchmark's shape still fits four waves; the siblings' odd shapes; the deepest model at 20 angles
static_assert(lambda_ng_ok(20, 56, 3) && 4 * RtLambdaNg(20, 56, 3).bytes() <= kLdsBytes, "RtLambdaNg: four waves of 56 depth points at 20 angles must fit");
static_assert(lambda_ng_ok(1, 2, 64) && lambda_ng_ok(1, 3, 64) && lambda_ng_ok(3, 3, 21) && lambda_ng_ok(7, 9, 9) && lambda_ng_ok(20, 57, 3) && lambda_ng_ok(64, 40, 1), "RtLambdaNg");
static_assert(RtLambdaNg(20, 809, 1).bytes() <= kLdsBytes && RtLambdaNg(20, 810, 1).bytes() > kLdsBytes, "RtLambdaNg");
// the benchmark's shape fits at three points per wave; odd depth counts, both ends of the angle range; 20 angles keep three points per
// wave up to 167 depth points
static_assert(ew_ok(20, 56, 3) && ew_ok(1, 3, 64) && ew_ok(7, 57, 9) && ew_ok(64, 2, 1) && ew_ok(20, 167, 3) && ew_ok(20, 168, 2), "EwColumns");
static_assert(EwColumns(20, 167, 3).bytes() <= kLdsBytes && EwColumns(20, 168, 3).bytes() > kLdsBytes && EwColumns(20, 168, 2).bytes() <= kLdsBytes, "EwColumns");
// 3, 7 and 20 angles (odd row counts), deep models with gpw lowered, 64 angles at the shallowest model
static_assert(columns_ok(3, 56, 21) && columns_ok(7, 301, 3) && columns_ok(20, 302, 2) && columns_ok(5, 984, 1), "RtColumns / RtContColumns");
static_assert(columns_ok(20, 175, 2) && columns_ok(64, 2, 1), "RtColumns / RtContColumns");
static_assert(f32_ok(20, 56) && f32_ok(7, 57) && f32_ok(64, 2) && f32_ok(1, 3), "RtF32Columns");
// even and odd gap counts, the shallowest models; the flux terms fit the launch whichever of the two is larger
static_assert(segments_ok(8, 7, 20, 56) && segments_ok(8, 7, 7, 57) && segments_ok(8, 7, 64, 2) && segments_ok(8, 7, 1, 3), "RtSegments");
static_assert(RtSegments(8, 7, 20, 56).doubles() == RtSegments(8, 7, 20, 56).flux_end(), "20 angles: the flux terms are the larger");
static_assert(RtSegments(8, 7, 1, 57).doubles() == RtSegments(8, 7, 1, 57).staging_end(), "one angle, 64 columns: the staging is the larger");
// the benchmark's shape (56 depth points, 20 angles: three frequencies per wave) fits; odd ray counts, both ends of the angle range
static_assert(response_ok(20, 56, 3) && RtResponse(20, 56, 3).bytes() <= kLdsBytes, "RtResponse: 56 depth points at 20 angles must fit");
static_assert(response_ok(1, 2, 64) && response_ok(5, 3, 12) && response_ok(7, 9, 9) && response_ok(64, 40, 1) && response_ok(3, 117, 21), "RtResponse");
// the benchmark's shape fits at three frequencies per wave (one wave per workgroup); odd counts, both ends of the angle range; the
// deepest model at 20 angles
static_assert(lambda_adjoint_ok(20, 56, 3) && RtLambdaAdjoint(20, 56, 3).bytes() <= kLdsBytes, "RtLambdaAdjoint: 56 depth points at 20 angles must fit");
static_assert(lambda_adjoint_ok(1, 2, 64) && lambda_adjoint_ok(1, 3, 64) && lambda_adjoint_ok(3, 3, 21) && lambda_adjoint_ok(7, 9, 9) && lambda_adjoint_ok(64, 40, 1), "RtLambdaAdjoint");
static_assert(RtLambdaAdjoint(20, 271, 1).bytes() <= kLdsBytes && RtLambdaAdjoint(20, 272, 1).bytes() > kLdsBytes, "RtLambdaAdjoint");
}  // namespace rt_layout_checks
