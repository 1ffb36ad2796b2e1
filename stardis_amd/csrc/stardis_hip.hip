// stardis_hip.hip — C ABI (include/stardis_hip.h) over the gfx950 kernels in sdx_kernels.h.
// Build: stardis_amd/csrc/Makefile  (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enums only: the library is opened at run time (RcclApi below)

#include <memory>
#include <thread>

#include "../../include/stardis_hip.h"
#include "sdx_kernels.h"
#include "sdx_host_plan.h"

using namespace sdx;

namespace {

thread_local std::string g_error;
thread_local int g_error_code = 0;

// Experiment and analysis knobs (SDX_RT_SEG, SDX_WIDE_BLOCKS, SDX_SPLIT_LAUNCHES, ... — listed in include/stardis_hip.h): some of
// them change the order of summation or the choice of kernel, i.e. the last bits of a result and the "union of shards ==
// single GPU, bit for bit" invariant when ranks inherit different environments.  They are read ONLY when the one documented
// switch SDX_EXPERIMENT=1 is set; without it the environment cannot change what the library computes.
const char* knob(const char* name)
{
    static const bool on = [] {
        const char* e = std::getenv("SDX_EXPERIMENT");
        return e && std::atoi(e) == 1;
    }();
    return on ? std::getenv(name) : nullptr;
}

int fail(int code, const std::string& msg)
{
    g_error = msg;
    g_error_code = code;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? SDX_ERR_OOM : SDX_ERR_HIP,                     \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                        \
    } while (0)

#define REQUIRE(cond, msg)                                  \
    do {                                                    \
        if (!(cond)) return fail(SDX_ERR_ARG, msg);         \
    } while (0)

struct ProfileRecord {
    const char* name;
    const char* variant;  // which device kernel ran under this name (k_raytrace: "k_raytrace<1>", "k_raytrace_seg<8,7>", ...), or nullptr
    hipEvent_t start, stop;
};

}  // namespace

struct sdx_ctx {
    int device = 0;
    int n_cu = 256;  // compute units of the device
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // line-opacity scratch (depth-major pre-pass arrays)
    void* line_ws = nullptr;
    size_t line_ws_bytes = 0;
    // small scratch: d_nu partials, evaluation counter, bf coefficients
    void* small_ws = nullptr;
    size_t small_ws_bytes = 0;
    // partial line-opacity planes [n_split + 1][n_depth][nu_count] (last plane: narrow windows)
    void* part_ws = nullptr;
    size_t part_ws_bytes = 0;
    void* adj_ws = nullptr;  // the per-line sensitivities' centres, lists and partial sums (sdx_line_adjoint_dev)
    size_t adj_ws_bytes = 0;
    void* obs_ws = nullptr;  // the instrument adjoint's per-pixel factors a, b and scans PH, SL (sdx_observe_adjoint_dev)
    size_t obs_ws_bytes = 0;
    void* stage_ws = nullptr;  // a broadening stage's adjoint factors a = u / den, two rows of n (stage_adjoint)
    size_t stage_ws_bytes = 0;
    void* far_ws = nullptr;  // far_range of the line kernels' far field: two ints per global tile
    size_t far_ws_bytes = 0;
    // cnt_ge[N_nu + 2] (lines per centre index, for the narrow-window kernel) and the per-line integer lists: CntLayout
    void* cnt_ws = nullptr;
    size_t cnt_ws_bytes = 0;
    // tuning options (sdx_set_int_option)
    int64_t indexed_min_lines = 8192;  // line lists at least this long: wide lines found by centre range / the huge-line list instead of a full scan
    int64_t prepass_ticket_min_blocks = 16384;  // culled shards: from this many line blocks on the pre-pass draws its work from a counter
    int64_t mixed_precision = 0;       // 1: fp32 rational for far-wing (region I) evaluations of whole-tile windows
    int64_t segmented_raytrace = -1;   // -1: by the size of the GLOBAL grid; 0 never; 1 whenever the kernel supports the shape (the general
                                       // kernel); 2 the same, preferring k_raytrace_seg_step where the launch has its shape (as -1 does)
    int64_t far_field = -1;            // -1: by the size of the GLOBAL grid; 0 never; 1 whenever the line kernel runs 256-point tiles
    int64_t wide_list = -1;            // -1 / 1: short lists walk a compacted list of their wide lines wherever the pre-pass can build it; 0: they scan every line
    int64_t grid_plan = -1;            // -1: a step that is given an sdx_grid_plan uses it; 0: it is ignored (A/B runs inside one library)
    int64_t adjoint_partials = (int64_t)1 << 22;  // doubles of sdx_line_adjoint_dev's partial sums (at least one per item is always there): bounds the supertiles per item
    int64_t narrow_records = -1;       // -1: by the density of the list; 1: the pre-pass writes narrow records; 0: the narrow role reads the caller's tables (long dense fp64 lists)
    // timing
    hipEvent_t t0 = nullptr, t1 = nullptr;
    void* cont_ws = nullptr;  // continuum plane [n_depth][nu_count] of the fused step
    size_t cont_ws_bytes = 0;
    // staging of the host-pointer (*_f64) entry points: one device arena and one pinned host buffer, grown on demand and kept
    void* io_dev = nullptr;
    size_t io_dev_bytes = 0;
    void* io_pin = nullptr;
    size_t io_pin_bytes = 0;
    void* xfer_pin = nullptr;  // pinned bounce buffer of sdx_memcpy_h2d / _d2h (pageable user buffers would be pinned per call)
    size_t xfer_pin_bytes = 0;
    // sdx_malloc / sdx_free: freed blocks are kept (by capacity) and handed out again — every use is ordered on this context's
    // stream, so a block can be reused the moment it is freed; a drop-in call of the Python mirror uploads ~30 small arrays
    std::mutex pool_mutex;  // guards the block pool and the bounce buffer (DeviceArray.__del__ may run on any thread)
    std::unordered_map<void*, size_t> live_blocks;  // handed out: pointer -> capacity
    std::multimap<size_t, void*> free_blocks;       // kept: capacity -> pointer
    size_t free_block_bytes = 0;
    // bumped whenever a scratch buffer is reallocated: hipGraphs captured earlier hold the old device pointers
    uint64_t ws_generation = 0;
    // two-collective mode: what sdx_synthesize_classify_dev left in the scratch (grid spacing, the shard's line ranges, the
    // continuum plane) and for which problem; the synthesis that follows with options->line_m_max checks and consumes it
    struct {
        bool valid = false;
        bool far = false;         // ... the far field was on in phase 1 and
        bool far_ranges = false;  // ... its launch computed the tiles' far ranges (far_ws)
        int n_depth = 0;
        int64_t n_nu = 0, nu_begin = 0, nu_count = 0, n_lines = 0;
        uint64_t generation = 0;
    } classified;
    // the continuum launch of the last fused step, as its launch site enqueued it (sdx_continuum_route): kernel 0 none yet,
    // 1 k_prepass_continuum, 2 k_classify_continuum
    struct {
        int kernel = 0, tiled = 0, depths_per_block = 0, table_in_lds = 0, planned = 0, threads = 0, tiles = 0, rows = 0;
        int64_t shmem = 0;
    } cont_route;
    bool profile = false;
    std::vector<ProfileRecord> records;
    std::vector<hipEvent_t> event_pool;
};

// What the un-culled pre-pass launch forms from the grid, the line frequencies and the tabulated cross-section alone (include/stardis_hip.h)
struct sdx_grid_plan {
    sdx_ctx* ctx;
    // built from (checked against the step's arguments)
    int64_t n_nu, n_lines;
    const double *nus, *line_nus, *lambdas, *table_wavelength, *table_sigma;
    int n_table;
    // owned: doubles [0] = d_nu, [1] = 1 / d_nu, [kPlanFreqOffset + k n_nu + i] = plane k of frequency i (cross-section, nu^-3, r4, r6, r8);
    // ints cnt_ge [n_nu + 2], then centre [n_lines]
    double* d;
    int* i;
};

namespace {

// The problem as values: built once by the extern "C" entry points, right after their argument checks, and handed down as they are.
struct Grid {  // the model's depths, the frequency grid and the columns [nu_begin, nu_begin + nu_count) of this call
    int n_depth;
    int64_t n_nu;
    const double* nus;
    int64_t nu_begin, nu_count;
};
struct Lines {  // dense tables, or — `gen` — the description the pre-pass generates them from (doppler, gammas and alphas are then null)
    int64_t n_lines;
    const double *line_nus, *doppler, *gammas;
    int gamma_cols;
    const double* alphas;
    const LineParams* gen;
};
struct Rays {
    int n_theta;
    const double *temps, *ray_dist, *wts;
};

// small_ws, in bytes: the grid-spacing partial maxima, the counters (zeroed when the buffer is allocated: ensure_small), the grid sample
constexpr size_t kEvalsOffset = 2048;       // evaluation counter (one unsigned long long)
constexpr size_t kTicketOffset = 2064;      // work counters of a culled shard's counter-driven pre-pass launch (k_hlist_count zeroes eight)
constexpr size_t kListTicketOffset = 2128;  // finished line blocks of a short list's pre-pass (LineWork::ticket with n_csplit)
constexpr size_t kSampleOffset = 4096;      // the grid sample
constexpr size_t kSmallHeader = kSampleOffset + 8 * (size_t)sdx::kGridSample;
static_assert(sizeof(double) * sdx::kDnuPartials <= kEvalsOffset, "the partial maxima end before the evaluation counter");
static_assert(kEvalsOffset + sizeof(unsigned long long) <= kTicketOffset, "the evaluation counter ends before the ticket counters");
static_assert(kTicketOffset + 8 * sizeof(int) <= kListTicketOffset, "the ticket counters end before the list ticket");
static_assert(kListTicketOffset + sizeof(int) <= kSampleOffset, "the list ticket ends before the grid sample");
static_assert(kSampleOffset == sizeof(double) * sdx::kGridSampleOffset, "the kernels find the grid sample kGridSampleOffset doubles behind the partial maxima");

// cnt_ws, in ints: cnt_ge, then per line centre, nhw_max, whw_max and the lists hlist, wlist, wrank [n + 1], xlist; then hcount (its
// counters, `sel` 4 behind them), the list launches' per-block counts and — 8-byte aligned, doubles — the classification pass's per-line maxima
struct CntLayout {
    size_t n, centre, nhw_max, whw_max, hlist, wlist, wrank, xlist, hcount, sel, block_cnt, m_max, bytes;
    CntLayout(int64_t n_nu, int64_t n_lines) : n((size_t)n_lines)
    {
        centre = (size_t)(n_nu + 2 + 63) / 64 * 64;  // the length of cnt_ge
        nhw_max = centre + n, whw_max = nhw_max + n, hlist = whw_max + n, wlist = hlist + n, wrank = wlist + n, xlist = wrank + n + 1;
        hcount = whw_max + 5 * n + 8, sel = hcount + 4, block_cnt = hcount + 16;  // 3 ints per block of the list launches behind block_cnt
        m_max = (block_cnt + 3 * (n / 1024 + 8) + 1) & ~(size_t)1;  // (the buffer itself is aligned far beyond 8 bytes)
        bytes = (centre + 10 * n + 128 + 3 * (n / 1024 + 8) + 8) * sizeof(int);
    }
};

int ensure(sdx_ctx* ctx, void** buf, size_t* have, size_t need)
{
    if (*have >= need) return SDX_OK;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    hipStreamIsCapturing(ctx->stream, &st);
    if (st != hipStreamCaptureStatusNone)
        return fail(SDX_ERR_ARG, "workspace must be reserved before stream capture (sdx_reserve_line_workspace / warm-up call)");
    if (*buf) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipFree(*buf));
        *buf = nullptr;
        *have = 0;
    }
    hipError_t e = hipMalloc(buf, need);
    if (e == hipErrorOutOfMemory) {  // blocks kept by sdx_free are reclaimable: release them and try once more
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lock(ctx->pool_mutex);
        if (!ctx->free_blocks.empty()) {
            hipStreamSynchronize(ctx->stream);
            for (auto& b : ctx->free_blocks) hipFree(b.second);
            ctx->free_blocks.clear();
            ctx->free_block_bytes = 0;
            e = hipMalloc(buf, need);
        }
    }
    if (e != hipSuccess) {
        *buf = nullptr;
        return fail(e == hipErrorOutOfMemory ? SDX_ERR_OOM : SDX_ERR_HIP, std::string("hipMalloc(workspace): ") + hipGetErrorString(e));
    }
    *have = need;
    ++ctx->ws_generation;
    return SDX_OK;
}

// the small scratch: its counters [kEvalsOffset, kSampleOffset) start at zero — the launch that counts the finished line blocks of a short
// list's pre-pass (LineWork::ticket with n_csplit) leaves its counter at zero and relies on finding it so
constexpr int64_t kListAutoChunks = 16;  // "wide_list" = -1: short lists of at least this many chunks of 64 lines per line subset
int ensure_small(sdx_ctx* ctx, size_t need)
{
    const size_t before = ctx->small_ws_bytes;
    int rc = ensure(ctx, &ctx->small_ws, &ctx->small_ws_bytes, need);
    if (rc) return rc;
    if (ctx->small_ws_bytes != before) HIP_TRY(hipMemsetAsync((char*)ctx->small_ws + kEvalsOffset, 0, kSampleOffset - kEvalsOffset, ctx->stream));
    return SDX_OK;
}

// per (line, depth) item: wide scan 16 + record 48 + slow 16 + fp32 record 32, narrow record 32, huge-line scan copy 16
size_t line_ws_need(int n_depth, int64_t n_lines) { return (size_t)n_depth * (size_t)n_lines * 160 + 256; }

LineWork carve(sdx_ctx* ctx, int n_depth, int64_t n_lines, const CntLayout& cnt)
{
    const size_t n = (size_t)n_depth * (size_t)n_lines;
    char* p = (char*)ctx->line_ws;
    LineWork w{};
    w.wrec = (WideRec*)p;                    // 48 n, 16-byte aligned
    w.wscan = (WideScan*)(w.wrec + n);       // 16 n
    w.wslow = (WideSlow*)(w.wscan + n);      // 16 n
    WideRec32* rec32 = (WideRec32*)(w.wslow + n);  // 32 n
    w.wrec32 = ctx->mixed_precision ? rec32 : nullptr;
    w.n_inv = (double*)(rec32 + n);  // 8 n each
    w.n_y = w.n_inv + n;
    w.n_amp = w.n_y + n;
    w.nhw = (unsigned char*)(w.n_amp + n);  // 1 n (the 8 n bytes of the former window bounds stay reserved)
    if (ctx->mixed_precision) {  // the narrow role's records as floats in the same 24 n bytes, + the line frequencies as float pairs
        w.n_inv32 = (float*)w.n_inv;
        w.n_y32 = w.n_inv32 + n;
        w.n_amp32 = w.n_y32 + n;
        w.lnu32 = (float2v*)(w.n_amp32 + n);
    }
    w.hscan = (WideScan*)((int*)(w.n_amp + n) + 2 * n);  // 16 n (only the first hcount[0] entries of a row are used)
    w.cnt_ge = (int*)ctx->cnt_ws;
    w.centre = w.cnt_ge + cnt.centre;
    w.nhw_max = w.cnt_ge + cnt.nhw_max;
    w.whw_max = w.cnt_ge + cnt.whw_max;
    w.hcount = w.cnt_ge + cnt.hcount;  // (hlist, wlist, wrank, xlist: set for long lists, launch_line_lists)
    w.evals = (unsigned long long*)((char*)ctx->small_ws + kEvalsOffset);
    return w;
}

hipEvent_t take_event(sdx_ctx* ctx)
{
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}

struct LaunchScope {
    sdx_ctx* ctx;
    ProfileRecord rec{};
    bool on;
    LaunchScope(sdx_ctx* c, const char* name, const char* variant = nullptr) : ctx(c), on(c->profile)
    {
        if (on) {
            rec.name = name;
            rec.variant = variant;
            rec.start = take_event(ctx);
            rec.stop = take_event(ctx);
            hipEventRecord(rec.start, ctx->stream);
        }
    }
    ~LaunchScope()
    {
        if (on) {
            hipEventRecord(rec.stop, ctx->stream);
            ctx->records.push_back(rec);
        }
    }
};

int check_launch(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SDX_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return SDX_OK;
}

inline dim3 grid2(int64_t n, int rows) { return dim3((unsigned)((n + kBlock - 1) / kBlock), (unsigned)rows); }
inline unsigned blocks1(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// d_nu partial maxima into small_ws (reserved by line_prepass), and on the side the far ranges the step asks for (FarReq, count = 0: none)
int launch_dnu(sdx_ctx* ctx, int64_t n_nu, const double* nus, int* n_partial, const FarReq& far)
{
    const int nb = (int)std::min<int64_t>(kDnuPartials, std::max<int64_t>(1, (n_nu + kBlock * 8 - 1) / (kBlock * 8)));
    {
        LaunchScope ls(ctx, "k_dnu_partial");
        hipLaunchKernelGGL(k_dnu_partial, dim3(nb), dim3(kBlock), 0, ctx->stream, n_nu, nus, (double*)ctx->small_ws, (int*)nullptr, (int64_t)0, far);
    }
    *n_partial = nb;
    return check_launch("k_dnu_partial");
}

static int check_file_planes(const sdx_continuum* c, int64_t n_nu)
{
    REQUIRE(c->n_file_planes >= 0 && c->n_file_planes <= 4, "continuum: n_file_planes must be 0..4");
    for (int k = 0; k < c->n_file_planes; ++k) REQUIRE(c->file_plane[k], "continuum: null file plane");
    REQUIRE(c->n_file_planes == 0 || c->file_plane_ld >= n_nu, "continuum: file_plane_ld must cover the grid");
    return SDX_OK;
}

ContinuumArgs to_args(const sdx_continuum* c, const double* bf_coef)
{
    ContinuumArgs a{};
    a.lambdas = c->lambdas;
    a.n_table = c->n_table;
    a.table_wavelength = c->table_wavelength;
    a.table_sigma = c->table_sigma;
    a.table_density = c->table_density;
    a.bf_n_species = c->bf_cutoff ? c->bf_n_species : 0;
    a.bf_species_offsets = c->bf_species_offsets;
    a.bf_species_ion_number = c->bf_species_ion_number;
    a.bf_cutoff = c->bf_cutoff;
    a.bf_n_levels = a.bf_n_species > 0 ? c->bf_n_levels : 0;
    a.bf_coef = bf_coef;
    a.ff_n_species = c->ff_number_density ? c->ff_n_species : 0;
    a.ff_species_ion_number = c->ff_species_ion_number;
    a.ff_number_density = c->ff_number_density;
    a.ray_n_h = c->ray_n_h;
    a.ray_n_he = c->ray_n_he;
    a.ray_n_h2 = c->ray_n_h2;
    a.rayleigh_enabled = c->rayleigh_enabled;
    a.electron_density = c->electron_density;
    a.temperature = c->temperature;
    a.n_file_planes = std::max(0, std::min(4, c->n_file_planes));
    for (int k = 0; k < a.n_file_planes; ++k) a.file_plane[k] = c->file_plane[k];
    a.file_plane_ld = c->file_plane_ld;
    return a;
}

// bf coefficients [n_levels][n_depth] into small_ws after the header; n_levels must be known on the host
int launch_bf_coef(sdx_ctx* ctx, int n_depth, int n_species, int n_levels, const int32_t* offs, const int32_t* ions,
                   const double* cutoff, const double* level_density, double** coef_out)
{
    const size_t need = kSmallHeader + (size_t)n_levels * n_depth * sizeof(double);
    int rc = ensure_small(ctx, need);
    if (rc) return rc;
    double* coef = (double*)((char*)ctx->small_ws + kSmallHeader);
    {
        LaunchScope ls(ctx, "k_bf_coef");
        hipLaunchKernelGGL(k_bf_coef, dim3(blocks1((int64_t)n_levels * n_depth)), dim3(kBlock), 0, ctx->stream, n_depth,
                           n_species, offs, ions, cutoff, level_density, coef);
    }
    *coef_out = coef;
    return check_launch("k_bf_coef");
}

}  // namespace

// ================================================================================================ runtime
extern "C" {

const char* sdx_version(void) { return "stardis_hip 0.1 (gfx950, fp64)"; }
const char* sdx_last_error_string(void) { return g_error.c_str(); }
int sdx_last_error_code(void) { return g_error_code; }

int sdx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int sdx_set_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return SDX_OK;
}

sdx_ctx* sdx_create(int device, void* stream)
{
    if (hipSetDevice(device) != hipSuccess) {
        fail(SDX_ERR_HIP, "hipSetDevice failed: no usable HIP device " + std::to_string(device));
        (void)hipGetLastError();
        return nullptr;
    }
    sdx_ctx* ctx = new sdx_ctx();
    ctx->device = device;
    if (hipDeviceGetAttribute(&ctx->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ctx->n_cu <= 0) ctx->n_cu = 256;
    if (stream) {
        ctx->stream = (hipStream_t)stream;
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            fail(SDX_ERR_HIP, "hipStreamCreate failed");
            delete ctx;
            return nullptr;
        }
        ctx->own_stream = true;
    }
    hipEventCreate(&ctx->t0);
    hipEventCreate(&ctx->t1);
    return ctx;
}

void sdx_destroy(sdx_ctx* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (auto& r : ctx->records) {
        hipEventDestroy(r.start);
        hipEventDestroy(r.stop);
    }
    for (auto e : ctx->event_pool) hipEventDestroy(e);
    if (ctx->cont_ws) hipFree(ctx->cont_ws);
    if (ctx->t0) hipEventDestroy(ctx->t0);
    if (ctx->t1) hipEventDestroy(ctx->t1);
    if (ctx->line_ws) hipFree(ctx->line_ws);
    if (ctx->small_ws) hipFree(ctx->small_ws);
    if (ctx->part_ws) hipFree(ctx->part_ws);
    if (ctx->far_ws) hipFree(ctx->far_ws);
    if (ctx->adj_ws) hipFree(ctx->adj_ws);
    if (ctx->obs_ws) hipFree(ctx->obs_ws);
    if (ctx->stage_ws) hipFree(ctx->stage_ws);
    if (ctx->cnt_ws) hipFree(ctx->cnt_ws);
    if (ctx->io_dev) hipFree(ctx->io_dev);
    if (ctx->io_pin) hipHostFree(ctx->io_pin);
    if (ctx->xfer_pin) hipHostFree(ctx->xfer_pin);
    for (auto& b : ctx->free_blocks) hipFree(b.second);
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

int sdx_set_stream(sdx_ctx* ctx, void* stream)
{
    REQUIRE(ctx, "null context");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream) {
        hipStreamDestroy(ctx->stream);
        ctx->own_stream = false;
    }
    if (stream) {
        ctx->stream = (hipStream_t)stream;
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    }
    return SDX_OK;
}

void* sdx_get_stream(sdx_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int sdx_set_int_option(sdx_ctx* ctx, const char* name, int64_t value)
{
    REQUIRE(ctx && name, "sdx_set_int_option: null pointer");
    if (std::strcmp(name, "indexed_min_lines") == 0) {
        ctx->indexed_min_lines = value;
        return SDX_OK;
    }
    if (std::strcmp(name, "prepass_ticket_min_blocks") == 0) {
        ctx->prepass_ticket_min_blocks = value;
        return SDX_OK;
    }
    if (std::strcmp(name, "mixed_precision") == 0) {
        ctx->mixed_precision = value ? 1 : 0;
        return SDX_OK;
    }
    if (std::strcmp(name, "segmented_raytrace") == 0) {
        ctx->segmented_raytrace = value < 0 ? -1 : (value >= 2 ? 2 : (value ? 1 : 0));
        return SDX_OK;
    }
    if (std::strcmp(name, "far_field") == 0) {
        ctx->far_field = value < 0 ? -1 : (value ? 1 : 0);
        return SDX_OK;
    }
    if (std::strcmp(name, "wide_list") == 0) {
        ctx->wide_list = value < 0 ? -1 : (value ? 1 : 0);
        return SDX_OK;
    }
    if (std::strcmp(name, "grid_plan") == 0) {
        ctx->grid_plan = value < 0 ? -1 : (value ? 1 : 0);
        return SDX_OK;
    }
    if (std::strcmp(name, "narrow_records") == 0) {
        ctx->narrow_records = value < 0 ? -1 : (value ? 1 : 0);
        return SDX_OK;
    }
    if (std::strcmp(name, "adjoint_partials") == 0) {
        ctx->adjoint_partials = value < 1 ? 1 : value;
        return SDX_OK;
    }
    return fail(SDX_ERR_ARG, std::string("unknown option ") + name);
}

// FAR FIELD (line_far_body, the far role of the line kernels): a third plane.  Like every choice that moves a rounding it is made from the GLOBAL grid — grids of at
// least kFarMinPoints frequencies (below that a launch of the line kernel is bound by latency, not by its evaluations) — or set
// explicitly (context option "far_field").
constexpr int64_t kFarMinPoints = 32768;
static_assert(kFarMinPoints == 32768, "sdx_far_field_rule reports this constant");
static bool far_field_on(const sdx_ctx* ctx, int64_t n_nu_global)
{
    const int far_mode = (int)ctx->far_field;  // (context option: -1 by the rule, 0 never, 1 whenever possible)
    return far_mode != 0 && (far_mode == 1 || n_nu_global >= kFarMinPoints);
}
int sdx_far_field_active(const sdx_ctx* ctx, int64_t n_nu_global)
{
    REQUIRE(ctx, "null context");
    return far_field_on(ctx, n_nu_global) ? 1 : 0;
}

int sdx_continuum_route(const sdx_ctx* ctx, int64_t* out, int n_out)
{
    REQUIRE(ctx && out && n_out >= 0, "sdx_continuum_route: null pointer");
    const auto& r = ctx->cont_route;
    const int64_t v[10] = {r.kernel, r.tiled, r.depths_per_block, r.table_in_lds, r.planned, r.threads, r.tiles, r.rows, r.shmem, ctx->n_cu};
    for (int k = 0; k < n_out && k < 10; ++k) out[k] = v[k];
    return SDX_OK;
}

int sdx_far_field_rule(int64_t* min_points, int* tile_points, int* near_points)
{
    if (min_points) *min_points = 32768;  // kFarMinPoints (static_assert where it is defined)
    if (tile_points) *tile_points = kFarTile;
    // a (line, tile) pair is far when the line's centre is >= kFarRatio tile half-widths from the tile's centre: a point closer than
    // that + half a tile to the centre is always evaluated where it lies
    if (near_points) *near_points = (int)(kFarRatio * (kFarTile / 2)) + kFarTile / 2;
    return SDX_OK;
}

int sdx_synchronize(sdx_ctx* ctx)
{
    REQUIRE(ctx, "null context");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SDX_OK;
}

constexpr size_t kBlockPoolLimit = (size_t)4 << 30;  // bytes of freed blocks kept per context
static size_t block_capacity(size_t bytes)
{
    if (bytes <= 256) return 256;
    if (bytes >= ((size_t)1 << 20)) return (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);  // whole MiB
    size_t c = 256;
    while (c < bytes) c <<= 1;
    return c;
}

void* sdx_malloc(sdx_ctx* ctx, size_t bytes)
{
    if (!ctx) return nullptr;
    hipSetDevice(ctx->device);
    const size_t cap = block_capacity(bytes);
    std::lock_guard<std::mutex> lock(ctx->pool_mutex);
    auto it = ctx->free_blocks.lower_bound(cap);
    if (it != ctx->free_blocks.end() && it->first <= 2 * cap) {  // a kept block of (nearly) this size
        void* p = it->second;
        ctx->free_block_bytes -= it->first;
        ctx->live_blocks[p] = it->first;
        ctx->free_blocks.erase(it);
        return p;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, cap);
    if (e != hipSuccess && !ctx->free_blocks.empty()) {  // out of memory with blocks in the pool: release them and try again
        hipStreamSynchronize(ctx->stream);
        for (auto& b : ctx->free_blocks) hipFree(b.second);
        ctx->free_blocks.clear();
        ctx->free_block_bytes = 0;
        e = hipMalloc(&p, cap);
    }
    if (e != hipSuccess) {
        fail(SDX_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
        return nullptr;
    }
    ctx->live_blocks[p] = cap;
    return p;
}

int sdx_free(sdx_ctx* ctx, void* ptr)
{
    REQUIRE(ctx, "null context");
    if (!ptr) return SDX_OK;
    {
        std::lock_guard<std::mutex> lock(ctx->pool_mutex);
        auto it = ctx->live_blocks.find(ptr);
        if (it == ctx->live_blocks.end()) {
            // not handed out by sdx_malloc of this context (or freed already: the block may be pooled or reused by now)
            return fail(SDX_ERR_ARG, "sdx_free: pointer is not a live block of this context (double free?)");
        }
        const size_t cap = it->second;
        ctx->live_blocks.erase(it);
        if (ctx->free_block_bytes + cap <= kBlockPoolLimit) {
            ctx->free_blocks.emplace(cap, ptr);
            ctx->free_block_bytes += cap;
            return SDX_OK;
        }
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipFree(ptr));
    return SDX_OK;
}

// ---- grid plan -------------------------------------------------------------------------------------------------------------
static int enqueue_grid_plan(sdx_grid_plan* p)
{
    sdx_ctx* ctx = p->ctx;
    const int n_line_blocks = (int)((p->n_lines + kPreBlock - 1) / kPreBlock);
    const int n_pix_blocks = (int)((p->n_nu + 2 + kPreBlock - 1) / kPreBlock);
    const int n_freq_blocks = (int)((p->n_nu + kPreBlock - 1) / kPreBlock);
    {
        LaunchScope ls(ctx, "k_grid_plan_build");
        hipLaunchKernelGGL(k_grid_plan_build, dim3((unsigned)(1 + n_line_blocks + n_pix_blocks + n_freq_blocks)), dim3(kPreBlock), 0, ctx->stream, p->n_nu,
                           p->nus, p->n_lines, p->line_nus, p->lambdas, p->n_table, p->table_wavelength, p->table_sigma, p->d, p->i,
                           p->i + (p->n_nu + 2), n_line_blocks, n_pix_blocks);
    }
    return check_launch("k_grid_plan_build");
}

int sdx_grid_plan_create(sdx_ctx* ctx, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus, const sdx_continuum* cont,
                         sdx_grid_plan** out)
{
    REQUIRE(ctx && out, "grid plan: null context or result pointer");
    *out = nullptr;
    REQUIRE(n_nu > 0 && n_nu < (int64_t)2147483647 && nus, "grid plan: the grid must have 1 .. 2^31 - 2 points");
    REQUIRE(n_lines >= 0 && n_lines < (int64_t)2147483647 && (n_lines == 0 || line_nus), "grid plan: bad line list");
    const bool table = cont && cont->table_sigma;
    REQUIRE(!table || (cont->lambdas && cont->table_wavelength && cont->n_table > 0), "grid plan: a cross-section table needs lambdas and its wavelength axis");
    hipSetDevice(ctx->device);
    sdx_grid_plan* p = new sdx_grid_plan{};
    p->ctx = ctx, p->n_nu = n_nu, p->n_lines = n_lines, p->nus = nus, p->line_nus = line_nus;
    p->lambdas = cont ? cont->lambdas : nullptr;
    p->table_wavelength = cont ? cont->table_wavelength : nullptr;
    p->table_sigma = cont ? cont->table_sigma : nullptr;
    p->n_table = cont ? cont->n_table : 0;
    p->d = (double*)sdx_malloc(ctx, ((size_t)kPlanFreqOffset + 5 * (size_t)n_nu) * sizeof(double));
    p->i = p->d ? (int*)sdx_malloc(ctx, ((size_t)n_nu + 2 + (size_t)n_lines) * sizeof(int)) : nullptr;
    int rc = p->i ? enqueue_grid_plan(p) : sdx_last_error_code();
    if (rc) {
        sdx_grid_plan_destroy(p);
        return rc;
    }
    *out = p;
    return SDX_OK;
}

int sdx_grid_plan_refresh(sdx_grid_plan* plan)
{
    REQUIRE(plan, "grid plan: null plan");
    return enqueue_grid_plan(plan);
}

void sdx_grid_plan_destroy(sdx_grid_plan* plan)
{
    if (!plan) return;
    // (blocks go back to the context's pool: every use is ordered on its stream)
    if (plan->i) sdx_free(plan->ctx, plan->i);
    if (plan->d) sdx_free(plan->ctx, plan->d);
    delete plan;
}

// the step's arguments against what a plan was built from: refused before anything is enqueued
static int check_grid_plan(const sdx_ctx* ctx, const sdx_grid_plan* p, const Grid& g, const Lines& l, const sdx_continuum* cont)
{
    REQUIRE(p->ctx == ctx, "synthesize: the grid plan belongs to another context");
    REQUIRE(p->n_nu == g.n_nu && p->nus == g.nus, "synthesize: the grid plan was built for another frequency grid (pointer or size)");
    REQUIRE(p->n_lines == l.n_lines && (l.n_lines == 0 || p->line_nus == l.line_nus), "synthesize: the grid plan was built for another line list (pointer or size)");
    REQUIRE(p->table_sigma == cont->table_sigma && (!cont->table_sigma || (p->lambdas == cont->lambdas && p->table_wavelength == cont->table_wavelength &&
                                                                           p->n_table == cont->n_table)),
            "synthesize: the grid plan was built for another cross-section table (pointers or size)");
    return SDX_OK;
}

// Copies between pageable user memory and the device go through a pinned bounce buffer of the context, in chunks: handing the
// runtime a pageable pointer makes it pin the user's pages for the call — measured 9 ms for a 61 KB numpy array, where the
// bounce costs a memcpy and a 10 us DMA.
constexpr size_t kXferChunk = (size_t)8 << 20;
static int xfer_buffer(sdx_ctx* ctx, size_t bytes)
{
    const size_t want = std::min(kXferChunk, std::max(bytes, (size_t)1 << 20));
    if (ctx->xfer_pin_bytes >= want) return SDX_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->xfer_pin) HIP_TRY(hipHostFree(ctx->xfer_pin));
    ctx->xfer_pin = nullptr;
    ctx->xfer_pin_bytes = 0;
    HIP_TRY(hipHostMalloc(&ctx->xfer_pin, want, hipHostMallocDefault));
    ctx->xfer_pin_bytes = want;
    return SDX_OK;
}

int sdx_memcpy_h2d(sdx_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    REQUIRE(ctx && (bytes == 0 || (dst && src)), "sdx_memcpy_h2d: null pointer");
    if (bytes == 0) return SDX_OK;
    static const bool no_pin = knob("SDX_NO_PINNED_STAGING") != nullptr;
    if (no_pin) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // pageable source: safe to reuse on return
        return SDX_OK;
    }
    std::lock_guard<std::mutex> lock(ctx->pool_mutex);  // one bounce buffer per context
    int rc = xfer_buffer(ctx, bytes);
    if (rc) return rc;
    for (size_t off = 0; off < bytes; off += ctx->xfer_pin_bytes) {
        const size_t n = std::min(ctx->xfer_pin_bytes, bytes - off);
        std::memcpy(ctx->xfer_pin, (const char*)src + off, n);
        HIP_TRY(hipMemcpyAsync((char*)dst + off, ctx->xfer_pin, n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // the bounce buffer is reused by the next chunk / call
    }
    return SDX_OK;
}

int sdx_memcpy_d2h(sdx_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    REQUIRE(ctx && (bytes == 0 || (dst && src)), "sdx_memcpy_d2h: null pointer");
    if (bytes == 0) return SDX_OK;
    static const bool no_pin = knob("SDX_NO_PINNED_STAGING") != nullptr;
    if (no_pin) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return SDX_OK;
    }
    std::lock_guard<std::mutex> lock(ctx->pool_mutex);
    int rc = xfer_buffer(ctx, bytes);
    if (rc) return rc;
    for (size_t off = 0; off < bytes; off += ctx->xfer_pin_bytes) {
        const size_t n = std::min(ctx->xfer_pin_bytes, bytes - off);
        HIP_TRY(hipMemcpyAsync(ctx->xfer_pin, (const char*)src + off, n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        std::memcpy((char*)dst + off, ctx->xfer_pin, n);
    }
    return SDX_OK;
}

// Page-locked host memory for callers that keep their own staging / result buffers there (the Python mirror's fused call): the
// copies below move it by DMA directly, without the bounce buffer and its memcpy.
void* sdx_host_alloc(sdx_ctx* ctx, size_t bytes)
{
    if (!ctx || bytes == 0) {
        fail(SDX_ERR_ARG, "sdx_host_alloc: null context or zero size");
        return nullptr;
    }
    void* p = nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        fail(SDX_ERR_OOM, "sdx_host_alloc: hipHostMalloc of " + std::to_string(bytes) + " bytes failed");
        return nullptr;
    }
    return p;
}

int sdx_host_free(void* ptr)
{
    if (!ptr) return SDX_OK;
    HIP_TRY(hipHostFree(ptr));
    return SDX_OK;
}

int sdx_memcpy_h2d_pinned(sdx_ctx* ctx, void* dst, const void* src_pinned, size_t bytes)
{
    REQUIRE(ctx && (bytes == 0 || (dst && src_pinned)), "sdx_memcpy_h2d_pinned: null pointer");
    if (bytes == 0) return SDX_OK;
    HIP_TRY(hipMemcpyAsync(dst, src_pinned, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SDX_OK;
}

int sdx_memcpy_d2h_pinned(sdx_ctx* ctx, void* dst_pinned, const void* src, size_t bytes)
{
    REQUIRE(ctx && (bytes == 0 || (dst_pinned && src)), "sdx_memcpy_d2h_pinned: null pointer");
    if (bytes == 0) return SDX_OK;
    HIP_TRY(hipMemcpyAsync(dst_pinned, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SDX_OK;
}

int sdx_memset(sdx_ctx* ctx, void* dst, int value, size_t bytes)
{
    REQUIRE(ctx && (bytes == 0 || dst), "sdx_memset: null pointer");
    if (bytes == 0) return SDX_OK;
    HIP_TRY(hipMemsetAsync(dst, value, bytes, ctx->stream));
    return SDX_OK;
}

int sdx_reserve_line_workspace(sdx_ctx* ctx, int n_depth, int64_t n_lines)
{
    REQUIRE(ctx && n_depth > 0 && n_lines >= 0, "sdx_reserve_line_workspace: bad sizes");
    int rc = ensure_small(ctx, kSmallHeader);
    if (rc) return rc;
    return ensure(ctx, &ctx->line_ws, &ctx->line_ws_bytes, line_ws_need(n_depth, n_lines));
}

int sdx_graph_begin(sdx_ctx* ctx)
{
    REQUIRE(ctx, "null context");
    HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    return SDX_OK;
}

// A captured graph has the context's scratch pointers baked in: the handle remembers the workspace generation it was
// captured under and sdx_graph_launch refuses to replay it after any scratch buffer has been reallocated since.
struct GraphHandle {
    hipGraphExec_t exec;
    uint64_t generation;
};

int sdx_graph_end(sdx_ctx* ctx, void** graph_exec_out)
{
    REQUIRE(ctx && graph_exec_out, "sdx_graph_end: null pointer");
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamEndCapture(ctx->stream, &graph));
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(SDX_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    *graph_exec_out = (void*)new GraphHandle{exec, ctx->ws_generation};
    return SDX_OK;
}

int sdx_graph_launch(sdx_ctx* ctx, void* graph_exec)
{
    REQUIRE(ctx && graph_exec, "sdx_graph_launch: null pointer");
    GraphHandle* h = (GraphHandle*)graph_exec;
    if (h->generation != ctx->ws_generation)
        return fail(SDX_ERR_STALE, "graph is stale: the context's workspace was reallocated after the capture (a larger problem ran on the "
                                   "same context); capture again");
    HIP_TRY(hipGraphLaunch(h->exec, ctx->stream));
    return SDX_OK;
}

int sdx_graph_destroy(sdx_ctx* ctx, void* graph_exec)
{
    REQUIRE(ctx, "null context");
    if (graph_exec) {
        GraphHandle* h = (GraphHandle*)graph_exec;
        hipError_t e = hipGraphExecDestroy(h->exec);
        delete h;
        if (e != hipSuccess) return fail(SDX_ERR_HIP, std::string("hipGraphExecDestroy: ") + hipGetErrorString(e));
    }
    return SDX_OK;
}

int sdx_timer_start(sdx_ctx* ctx)
{
    REQUIRE(ctx, "null context");
    HIP_TRY(hipEventRecord(ctx->t0, ctx->stream));
    return SDX_OK;
}

int sdx_timer_stop(sdx_ctx* ctx, double* elapsed_ms)
{
    REQUIRE(ctx && elapsed_ms, "sdx_timer_stop: null pointer");
    HIP_TRY(hipEventRecord(ctx->t1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->t1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->t0, ctx->t1));
    *elapsed_ms = ms;
    return SDX_OK;
}

int sdx_profile_enable(sdx_ctx* ctx, int on)
{
    REQUIRE(ctx, "null context");
    ctx->profile = on != 0;
    return SDX_OK;
}

int sdx_profile_reset(sdx_ctx* ctx)
{
    REQUIRE(ctx, "null context");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (auto& r : ctx->records) {
        ctx->event_pool.push_back(r.start);
        ctx->event_pool.push_back(r.stop);
    }
    ctx->records.clear();
    return SDX_OK;
}

int sdx_profile_get(sdx_ctx* ctx, const char* kernel, int64_t* launches, double* total_ms)
{
    REQUIRE(ctx && kernel && launches && total_ms, "sdx_profile_get: null pointer");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int64_t n = 0;
    double tot = 0.0;
    for (auto& r : ctx->records) {
        if (std::strcmp(r.name, kernel) != 0) continue;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.start, r.stop));
        tot += ms;
        ++n;
    }
    *launches = n;
    *total_ms = tot;
    return SDX_OK;
}

int sdx_profile_variant(sdx_ctx* ctx, const char* kernel, char* out, int out_len)
{
    REQUIRE(ctx && kernel && out && out_len > 0, "sdx_profile_variant: null pointer");
    out[0] = 0;
    for (auto& r : ctx->records)
        if (std::strcmp(r.name, kernel) == 0 && r.variant) std::snprintf(out, (size_t)out_len, "%s", r.variant);
    return SDX_OK;
}

// ================================================================================================ line opacity
// Frequency shards of long lists, two-collective mode: the classification stream of a culled pre-pass (the largest (gamma + dw) alpha
// of every line, 8 N_l (2 N_d + G) bytes read by EVERY rank) split over the ranks — phase 1 classifies a share of the lines into the
// caller's m_max array (and does everything else of that launch: grid spacing, the shard's line ranges, the continuum plane), the
// caller exchanges the shares (an all-gather of 8 N_l bytes), phase 2 is the rest of the step on the gathered array.
struct ClassifyPhase {
    int phase;             // 1 or 2
    int64_t begin, count;  // phase 1: the lines to classify
    double* m_max;         // [n_lines]: phase 1 writes [begin, begin + count), phase 2 reads everything
};

// The segmented formal solution (k_raytrace_seg: the gaps of a ray over the 8 waves of a workgroup) pays ~40 % more
// instructions for eight times the waves: it wins where k_raytrace would leave the chip under three waves per SIMD.
// lane / G as a multiply and a shift in k_raytrace_seg (lane_div, sdx_kernels.h): exact for lane < 64, 1 <= G <= 64
static int lane_recip(int G)
{
    return 65536 / G + 1;
}
static RtSegments seg_layout(int n_depth, int nth)
{
    return RtSegments(8, 7, nth, n_depth);  // eight waves, at most seven gaps each
}
// Which kernel runs must not depend on how the grid is sharded or on the device (the two differ by the rounding of the affine
// composition, a few ulp: a shard below the threshold next to an unsharded run above it would break the bit-identity of
// sharded and unsharded spectra): the choice is made from the GLOBAL grid size against a fixed constant — three k_raytrace
// waves per SIMD of a 256-CU part — or set explicitly (context option "segmented_raytrace").
constexpr int64_t kSegLegacyWaves = (int64_t)3 * 4 * 256;
static int segmented_mode(const sdx_ctx* ctx)
{
    // A/B knob: 0 never, 1 whenever possible (the general kernel), 2 whenever possible and the step kernel where the shape allows
    static const int env_mode = knob("SDX_RT_SEG") ? std::atoi(knob("SDX_RT_SEG")) : -1;
    const int mode = ctx->segmented_raytrace >= 0 ? (int)ctx->segmented_raytrace : env_mode;
    return mode < 0 ? -1 : std::min(mode, 2);
}
static bool use_segmented_raytrace(const sdx_ctx* ctx, int n_depth, int64_t n_nu_global, int n_theta, bool plain)
{
    const int mode = segmented_mode(ctx);
    if (mode == 0 || !plain || n_theta > 64) return false;
    if (!seg_layout(n_depth, n_theta).segment_fits() || seg_layout(n_depth, n_theta).bytes() > kLdsBytes) return false;
    if (mode >= 1) return true;
    const int64_t legacy_waves = (n_nu_global + 64 / n_theta - 1) / (64 / n_theta);
    return legacy_waves < kSegLegacyWaves;
}

// long lists: hlist / wlist / wrank from whw_max, or from a classification pass (two small launches)
static void launch_line_lists(sdx_ctx* ctx, const CntLayout& cnt, LineWork& w, int pre_lines, const ClassSource* from_classification)
{
    ClassSource cs{};
    if (from_classification) cs = *from_classification;
    else cs.whw_max = w.whw_max;
    int* const base = (int*)ctx->cnt_ws;
    const int64_t n_lines = (int64_t)cnt.n;
    w.hlist = base + cnt.hlist;
    w.wlist = base + cnt.wlist;
    w.wrank = base + cnt.wrank;
    w.xlist = w.sel ? base + cnt.xlist : nullptr;  // culled runs only
    const unsigned hb = (unsigned)((n_lines + kHlistBlock - 1) / kHlistBlock);
    int* block_cnt = base + cnt.block_cnt;  // 3 hb ints behind the counters and sel
    hipLaunchKernelGGL(k_hlist_count, dim3(hb), dim3(kHlistBlock), 0, ctx->stream, n_lines, cs, block_cnt, w.sel, pre_lines, w.ticket);
    hipLaunchKernelGGL(k_hlist_scatter, dim3(hb), dim3(kHlistBlock), 0, ctx->stream, n_lines, cs, (const int*)block_cnt, w.hlist,
                       w.wlist, w.wrank, w.hcount, w.xlist, w.sel, pre_lines);
}

// What a caller asks of the pre-pass beyond the problem itself ...
struct PrepassRequest {
    int32_t *lo_ref, *hi_ref;   // the windows alone (sdx_line_windows_dev); null: the line kernels' records
    bool count_evals;
    const sdx_continuum* cont;  // the fused step: its continuum plane [n_depth][nu_count] is computed ...
    double* cont_plane;         // ... into this by the trailing blocks of the pre-pass (or the classification) launch
    const ClassifyPhase* ph;    // two-collective mode
    int wide_splits;            // the wide role's line subsets (a short list's wide lines are listed per subset); 0: no such list
    const sdx_grid_plan* plan;
    FarReq far;                 // the tiles whose far ranges the step's grid-spacing launch computes on the side (count = 0: none)
};

// continuum blocks of the fused step: one per (frequency tile of `threads` points, group of dgs depths) when the per-depth
// factors of a group fit LDS (always, for a handful of bound-free levels), else one per (tile, depth) evaluating every point
// from scratch
struct ContPlan {
    ContinuumArgs ca;
    size_t shmem;
    int cont_tiles, stage_table;
    unsigned cont_rows;
    bool tiled;
};
// (other_blocks: the line and pixel blocks of a pre-pass launch the tiles ride with)
static int plan_continuum(const sdx_ctx* ctx, const sdx_continuum* cont, const Grid& g, int threads, int64_t other_blocks, ContPlan* p)
{
    const int n_depth = g.n_depth;
    p->ca = to_args(cont, nullptr);
    ContinuumArgs& ca = p->ca;
    ca.bf_level_density = cont->bf_level_density;
    REQUIRE(ca.bf_n_species <= 0 || (cont->bf_n_levels > 0 && cont->bf_n_levels <= 4096), "synthesize: bf_n_levels must be set (1..4096)");
    const size_t n_lev = ca.bf_n_species > 0 ? (size_t)cont->bf_n_levels : 0;
    p->stage_table = ca.table_sigma && ca.n_table > 0 && ca.n_table <= 1024;  // 1-D cross-section table searched from LDS
    p->shmem = std::max<size_t>(8, (n_lev + (p->stage_table ? 2 * (size_t)ca.n_table : 0)) * sizeof(double));  // (untiled: the bound-free edges, the table)
    p->cont_tiles = (int)((g.nu_count + (int64_t)threads * kContPoints - 1) / ((int64_t)threads * kContPoints));
    const size_t tile_shmem = ((size_t)kContDepths * (n_lev + 6) + (p->stage_table ? 2 * (size_t)ca.n_table : 0)) * sizeof(double);
    p->cont_rows = (unsigned)n_depth;
    p->tiled = false;
    if (tile_shmem <= 48 * 1024) {
        // depths per block: as many as leave ~2 x 1024 threads of such blocks per CU (one depth per block on small grids)
        int dgs = (int)std::max<int64_t>(1, std::min<int64_t>(kContDepths, ((int64_t)p->cont_tiles * threads / kPreBlock * n_depth) / (2 * (int64_t)ctx->n_cu)));
        if (threads == kPreBlock) {
            // ... next to the launch's pre-pass blocks: ALL blocks of the launch in one round of the chip's 2 x n_cu slots of 1024
            // threads (S-c2: 133 pre-pass blocks + 448 one-depth tiles were 581 on 512 slots — the 69 of the second round ended
            // the launch at 15.6 us where two depths per tile end it at 12.0; device time stamps, scripts/r5/pre_stats.sh)
            const int64_t slots = std::max<int64_t>(1, 2 * (int64_t)ctx->n_cu - other_blocks * ((n_depth + kPreDepths - 1) / kPreDepths));
            const int64_t fit = ((int64_t)p->cont_tiles * n_depth + slots - 1) / slots;
            dgs = (int)std::max<int64_t>(dgs, std::min<int64_t>(kContDepths, fit));
        }
        // riding with the classification stream (256-thread blocks) the chip is full anyway: as many depths per block as
        // there are — the per-frequency work (table search, nu^-3, Rayleigh powers) is then shared by eight points
        if (threads == kBlock) dgs = kContDepths;
        p->stage_table |= 2 | (dgs << 4);
        p->shmem = tile_shmem;
        p->cont_rows = (unsigned)((n_depth + dgs - 1) / dgs);
        p->tiled = true;
    }
    return SDX_OK;
}

// sdx_continuum_route: what a launch hands its continuum blocks, read the way the kernels read it (`stage_table` bit 0: table in
// LDS, bit 1: depth-group tiles, bits 4..7: depths per block; a planned launch always runs tiles and stages no table)
static void note_cont_route(sdx_ctx* ctx, int kernel, const ContPlan& cp, bool planned, int threads)
{
    auto& r = ctx->cont_route;
    r.kernel = kernel;
    r.tiled = planned || (cp.stage_table & 2) != 0;
    r.depths_per_block = r.tiled ? (cp.stage_table >> 4) & 15 : 1;
    r.table_in_lds = !planned && (cp.stage_table & 1) != 0;
    r.planned = planned;
    r.threads = threads;
    r.tiles = cp.cont_tiles;
    r.rows = (int)cp.cont_rows;
    r.shmem = (int64_t)cp.shmem;
}

// ... and what it gets back (where the caller wants it)
struct PrepassResult {
    LineWork w;
    bool far_ranges;  // a launch has taken the requested far ranges along
};
// what line_prepass has decided when it comes to its launches: private to it and its pieces below
struct PrepassLaunch {
    LineWork w;
    bool far_ranges;
    int pre_lines, n_line_blocks, n_pixel_blocks, n_partial;
    bool scan_in_block;       // every pre-pass block re-scans a small grid instead of a separate launch
    const ContPlan* planned;  // the grid plan is honoured, with these continuum tiles; else null
    bool continuum_done;      // the continuum plane rode with the classification launch
};

// culled runs: classification stream, the line lists, then ONE pre-pass launch with range + gather blocks.  In the fused
// step the continuum plane rides with the classification launch — an HBM stream that leaves the vector units idle —
// instead of the pre-pass launch, which a shard's line blocks already fill (S-c3 / 8: 540 line + gather blocks and 590
// continuum blocks on 512 block slots)
static int prepass_culled(sdx_ctx* ctx, const Grid& g, const Lines& l, const PrepassRequest& req, const CntLayout& cnt, PrepassLaunch& s)
{
    const int n_depth = g.n_depth;
    const int64_t n_nu = g.n_nu, n_lines = l.n_lines;
    const ClassifyPhase* const ph = req.ph;
    const sdx_continuum* const cont = req.cont;
    LineWork& w = s.w;
    int* const sel = (int*)ctx->cnt_ws + cnt.sel;
    w.sel = sel;
    // classification blocks: contiguous runs of lines, a few blocks per CU (256 threads: 4 waves x 4 lines x 3 arrays in flight)
    const int64_t cls_begin = ph && ph->phase == 1 ? ph->begin : 0, cls_end = ph && ph->phase == 1 ? ph->begin + ph->count : n_lines;
    // (a SHARE of the list — two-collective mode — is a few microseconds of streaming: sixteen lines per block, one trip of each
    // wave's loop, so that the launch is as long as one round trip and not as a chain of nine; the whole list is a stream that
    // wants its bytes in flight, not short chains)
    const bool share = ph && ph->phase == 1;
    const int64_t cls_per_block = share ? 16 : 64;
    const unsigned n_cls = (unsigned)std::max<int64_t>(1, std::min<int64_t>((cls_end - cls_begin + cls_per_block - 1) / cls_per_block, (int64_t)8 * ctx->n_cu));
    // the per-line maxima: doubles behind the integer lists of cnt_ws (8-byte aligned), or the caller's array (two-collective mode)
    double* const m_max = ph ? ph->m_max : (double*)((int*)ctx->cnt_ws + cnt.m_max);
    double* const dnu_ws = (double*)ctx->small_ws;
    ContPlan cp;
    if (cont) {
        if (int rc = plan_continuum(ctx, cont, g, kBlock, 0, &cp)) return rc;
        s.continuum_done = cp.tiled;
    }
    if (ph && ph->phase == 2) {
        // the classification launch ran in phase 1 (sdx_synthesize_classify_dev) and left the grid spacing, `sel` and the
        // continuum plane in this context's scratch — for THIS problem, and no buffer has moved since
        const auto& c = ctx->classified;
        REQUIRE(c.valid && c.n_depth == n_depth && c.n_nu == n_nu && c.nu_begin == g.nu_begin && c.nu_count == g.nu_count && c.n_lines == n_lines,
                "synthesize: options->line_m_max needs sdx_synthesize_classify_dev on this context first, for the same grid, shard and line list");
        REQUIRE(c.generation == ctx->ws_generation, "synthesize: the context's scratch was reallocated between sdx_synthesize_classify_dev and the synthesis");
        REQUIRE(!cont || s.continuum_done, "synthesize: two-collective mode needs the tiled continuum");
        // consumed: a second phase 2 needs a new phase 1 (the resident inputs may have been updated in place since; a recorded
        // graph replays both phases without this host check)
        ctx->classified.valid = false;
    } else {
        REQUIRE(!ph || !cont || s.continuum_done, "synthesize: two-collective mode needs the tiled continuum (at most 4096 bound-free levels)");
        LaunchScope ls(ctx, "k_classify");
        if (s.continuum_done) {
            // half the classification blocks (16 of 32 wave slots per CU: the stream keeps its bytes in flight), the
            // continuum blocks take the other slots
            const unsigned n_cls_half = share ? n_cls : std::max(1u, n_cls / 2);
            note_cont_route(ctx, 2, cp, false, kBlock);
            hipLaunchKernelGGL(k_classify_continuum, dim3((unsigned)s.n_partial + n_cls_half + (unsigned)cp.cont_tiles * cp.cont_rows), dim3(kBlock), cp.shmem, ctx->stream,
                               s.n_partial, (int)n_cls_half, n_depth, n_nu, n_lines, dnu_ws, l.doppler, l.gammas, l.gamma_cols, l.alphas, m_max, g.nus,
                               cp.cont_tiles, g.nu_begin, g.nu_count, cp.ca, req.cont_plane, g.nu_count, cp.stage_table, l.line_nus, g.nu_begin, g.nu_count,
                               sel, cls_begin, cls_end, req.far);
        } else {
            hipLaunchKernelGGL(k_classify, dim3((unsigned)s.n_partial + n_cls), dim3(kBlock), 0, ctx->stream, s.n_partial, n_depth, n_nu, n_lines, dnu_ws,
                               l.doppler, l.gammas, l.gamma_cols, l.alphas, m_max, g.nus, l.line_nus, g.nu_begin, g.nu_count, sel, cls_begin, cls_end, req.far);
        }
        if (req.far.count && s.n_partial > 0) s.far_ranges = true;
    }
    if (ph && ph->phase == 1) {
        auto& c = ctx->classified;
        c.valid = true, c.n_depth = n_depth, c.n_nu = n_nu, c.nu_begin = g.nu_begin, c.nu_count = g.nu_count, c.n_lines = n_lines;
        c.far_ranges = s.far_ranges;
        c.far = far_field_on(ctx, n_nu) && c.far_ranges;
        c.generation = ctx->ws_generation;
        return check_launch("k_classify");
    }
    // the pre-pass launch that follows draws its items from a counter (k_line_prepass_ticket); the list launch zeroes it
    // (worth it where the candidates are many: at 1e6 lines 57 000 of 62 000 candidate blocks are empty and the launch takes 245
    // instead of 292 us on an eighth of the grid; at 1.5e5 lines 9 500 candidates cost less than the counter's round trips)
    const bool ticket = !(cont && !s.continuum_done) && !l.gen && !req.lo_ref && s.n_line_blocks >= ctx->prepass_ticket_min_blocks;
    if (ticket) w.ticket = (int*)((char*)ctx->small_ws + kTicketOffset);
    {
        LaunchScope ls(ctx, "k_hlist");
        ClassSource cs{};
        cs.m_max = m_max, cs.dnu_partial = dnu_ws, cs.n_partial = s.n_partial, cs.n_nu = n_nu;
        launch_line_lists(ctx, cnt, w, s.pre_lines, &cs);
    }
    w.gather = s.n_line_blocks;  // worst case: every line listed; blocks beyond the lists' end return at once
    w.front = 1;
    return SDX_OK;
}

// the pre-pass launch itself: line, pixel and gather blocks, with the continuum tiles behind them unless the classification launch took them
static int prepass_launch(sdx_ctx* ctx, const Grid& g, const Lines& l, const PrepassRequest& req, PrepassLaunch& s)
{
    const int n_depth = g.n_depth, pre_lines = s.pre_lines, n_line_blocks = s.n_line_blocks, n_partial = s.n_partial;
    const int64_t n_nu = g.n_nu, n_lines = l.n_lines;
    const sdx_continuum* const cont = req.cont;
    const bool planned = s.planned != nullptr, scan_in_block = s.scan_in_block;
    const LineParams* const gen = l.gen;
    const LineParams lp = gen ? *gen : LineParams{};
    LineWork& w = s.w;
    const dim3 grid((unsigned)(n_line_blocks + s.n_pixel_blocks + w.gather), (unsigned)((n_depth + kPreDepths - 1) / kPreDepths));
    const bool ticket_launch = w.ticket != nullptr;  // (the counter-driven launch of a culled shard)
    if (w.n_csplit) w.ticket = (int*)((char*)ctx->small_ws + kListTicketOffset);
    if (cont && !s.continuum_done) {
        ContPlan cp;
        if (planned) cp = *s.planned;
        else if (int rc = plan_continuum(ctx, cont, g, kPreBlock, (int64_t)n_line_blocks + s.n_pixel_blocks, &cp)) return rc;
        const ContinuumArgs& ca = cp.ca;
        const int cont_tiles = cp.cont_tiles, stage_table = cp.stage_table;
        const size_t shmem = cp.shmem;
        const unsigned total_blocks = grid.x * grid.y + (unsigned)cont_tiles * cp.cont_rows;
        note_cont_route(ctx, 1, cp, planned, kPreBlock);
        {
        LaunchScope ls(ctx, "k_prepass_continuum", planned ? (w.n_csplit ? "planned + wide-line list" : "planned") : (w.n_csplit ? "+ wide-line list" : nullptr));
#define SDX_PRE_ARGS (int)grid.x, (int)grid.y, cont_tiles, n_depth, n_nu, g.nus,                                                                   \
                     planned ? (const double*)req.plan->d : (scan_in_block ? (const double*)nullptr : (const double*)ctx->small_ws),            \
                     n_partial, n_lines, l.line_nus, l.doppler, l.gammas, l.gamma_cols, l.alphas, w, n_line_blocks, g.nu_begin, g.nu_count, ca, \
                     req.cont_plane, g.nu_count, lp, stage_table
        if (planned && pre_lines == 16) hipLaunchKernelGGL((k_prepass_continuum<false, 16, true>), dim3(total_blocks), dim3(kPreBlock), shmem, ctx->stream, SDX_PRE_ARGS);
        else if (planned) hipLaunchKernelGGL((k_prepass_continuum<false, 32, true>), dim3(total_blocks), dim3(kPreBlock), shmem, ctx->stream, SDX_PRE_ARGS);
        else if (gen && pre_lines == 16) hipLaunchKernelGGL((k_prepass_continuum<true, 16>), dim3(total_blocks), dim3(kPreBlock), shmem, ctx->stream, SDX_PRE_ARGS);
        else if (gen) hipLaunchKernelGGL((k_prepass_continuum<true, 32>), dim3(total_blocks), dim3(kPreBlock), shmem, ctx->stream, SDX_PRE_ARGS);
        else if (pre_lines == 16) hipLaunchKernelGGL((k_prepass_continuum<false, 16>), dim3(total_blocks), dim3(kPreBlock), shmem, ctx->stream, SDX_PRE_ARGS);
        else if (pre_lines == 48) hipLaunchKernelGGL((k_prepass_continuum<false, 48>), dim3(total_blocks), dim3(kPreBlock), shmem, ctx->stream, SDX_PRE_ARGS);
        else if (pre_lines == 54) hipLaunchKernelGGL((k_prepass_continuum<false, 54>), dim3(total_blocks), dim3(kPreBlock), shmem, ctx->stream, SDX_PRE_ARGS);
        else hipLaunchKernelGGL((k_prepass_continuum<false, 32>), dim3(total_blocks), dim3(kPreBlock), shmem, ctx->stream, SDX_PRE_ARGS);
#undef SDX_PRE_ARGS
        }
    } else {
        LaunchScope ls(ctx, cont ? "k_prepass_continuum" : "k_line_prepass", w.n_csplit ? "+ wide-line list" : nullptr);
#define SDX_PRE_ARGS n_depth, n_nu, g.nus, scan_in_block ? (const double*)nullptr : (const double*)ctx->small_ws, n_partial, n_lines, l.line_nus, l.doppler, \
                     l.gammas, l.gamma_cols, l.alphas, w, (int*)req.lo_ref, (int*)req.hi_ref, n_line_blocks, lp
        if (ticket_launch) {
            const dim3 pgrid(std::min<unsigned>(grid.x, 2u * (unsigned)ctx->n_cu), grid.y);
            const double* dnu_arg = scan_in_block ? (const double*)nullptr : (const double*)ctx->small_ws;
#define SDX_TICKET_ARGS n_depth, n_nu, g.nus, dnu_arg, n_partial, n_lines, l.line_nus, l.doppler, l.gammas, l.gamma_cols, l.alphas, w, n_line_blocks, lp
            if (pre_lines == 16) hipLaunchKernelGGL((k_line_prepass_ticket<16>), pgrid, dim3(kPreBlock), 0, ctx->stream, SDX_TICKET_ARGS);
            else if (pre_lines == 48) hipLaunchKernelGGL((k_line_prepass_ticket<48>), pgrid, dim3(kPreBlock), 0, ctx->stream, SDX_TICKET_ARGS);
            else if (pre_lines == 54) hipLaunchKernelGGL((k_line_prepass_ticket<54>), pgrid, dim3(kPreBlock), 0, ctx->stream, SDX_TICKET_ARGS);
            else hipLaunchKernelGGL((k_line_prepass_ticket<32>), pgrid, dim3(kPreBlock), 0, ctx->stream, SDX_TICKET_ARGS);
#undef SDX_TICKET_ARGS
        } else if (pre_lines == 48) hipLaunchKernelGGL((k_line_prepass<false, 48>), grid, dim3(kPreBlock), 0, ctx->stream, SDX_PRE_ARGS);
        else if (pre_lines == 54) hipLaunchKernelGGL((k_line_prepass<false, 54>), grid, dim3(kPreBlock), 0, ctx->stream, SDX_PRE_ARGS);
        else if (gen && pre_lines == 16) hipLaunchKernelGGL((k_line_prepass<true, 16>), grid, dim3(kPreBlock), 0, ctx->stream, SDX_PRE_ARGS);
        else if (gen) hipLaunchKernelGGL((k_line_prepass<true, 32>), grid, dim3(kPreBlock), 0, ctx->stream, SDX_PRE_ARGS);
        else if (pre_lines == 16) hipLaunchKernelGGL((k_line_prepass<false, 16>), grid, dim3(kPreBlock), 0, ctx->stream, SDX_PRE_ARGS);
        else hipLaunchKernelGGL((k_line_prepass<false, 32>), grid, dim3(kPreBlock), 0, ctx->stream, SDX_PRE_ARGS);
#undef SDX_PRE_ARGS
    }
    return check_launch("k_line_prepass");
}

// decides lines per block, culling, a short list's wide-line list, raw narrow records and the planned continuum; then its launches
static int line_prepass(sdx_ctx* ctx, const Grid& g, const Lines& l, const PrepassRequest& req, PrepassResult* out)
{
    PrepassLaunch s{};
    const int n_depth = g.n_depth;
    const int64_t n_nu = g.n_nu, n_lines = l.n_lines;
    const bool fill_work = !req.lo_ref;
    // every pre-pass rewrites the scratch a two-collective phase 1 leaves for its phase 2 (grid spacing, line ranges, lists): only the
    // phase 2 that consumes it may find it valid (phase 1 sets the flag again when its launch is enqueued)
    const bool consumes_classified = req.ph && req.ph->phase == 2;
    if (!consumes_classified) ctx->classified.valid = false;
    int rc = ensure_small(ctx, kSmallHeader);
    if (rc) return rc;
    LineWork& w = s.w;
    s.scan_in_block = n_nu <= 16384;
    // 16 lines per block while all such blocks are resident at once (two 1024-thread blocks per CU), else 32
    s.pre_lines = ((n_lines + 15) / 16) * ((n_depth + kPreDepths - 1) / kPreDepths) <= 2 * (int64_t)ctx->n_cu ? 16 : 32;
    // A culled shard (`cull`, see below) prepares its own line range + the listed lines: at an eighth of 1.5e5
    // lines ~22 000 lines, 690 blocks of 32 on the chip's 512 slots of 1024 threads — a whole second round of the block's chain of
    // round trips for a third of a round's work.  48 lines per block (three items per thread, registers only) are 470 blocks:
    // ONE round, a chain one item longer.
    const bool cull = fill_work && n_lines >= ctx->indexed_min_lines && !req.count_evals && !l.gen && !s.scan_in_block && g.nu_count < n_nu;
    // (lists long enough for the counter-driven launch keep 32: its looping kernel has no registers to spare for a third item)
    // (54 when the model has at most 56 depth points — every MARCS model — and three items per thread still cover the block)
    if (cull && !req.lo_ref && (n_lines + 31) / 32 < ctx->prepass_ticket_min_blocks)
        s.pre_lines = n_depth <= 56 ? 54 : 48;
    s.n_line_blocks = (int)((n_lines + s.pre_lines - 1) / s.pre_lines);
    const CntLayout cnt(n_nu, n_lines);
    if (fill_work) {
        rc = ensure(ctx, &ctx->line_ws, &ctx->line_ws_bytes, line_ws_need(n_depth, n_lines));
        if (rc) return rc;
        rc = ensure(ctx, &ctx->cnt_ws, &ctx->cnt_ws_bytes, cnt.bytes);
        if (rc) return rc;
        w = carve(ctx, n_depth, n_lines, cnt);
        if (n_depth > kPreDepths) HIP_TRY(hipMemsetAsync(w.nhw_max, 0, (size_t)2 * n_lines * sizeof(int), ctx->stream));  // nhw_max and whw_max
        if (req.count_evals) HIP_TRY(hipMemsetAsync(w.evals, 0, sizeof(unsigned long long), ctx->stream));
        else w.evals = nullptr;
        s.n_pixel_blocks = (int)((n_nu + 2 + kPreBlock - 1) / kPreBlock);
    }
    // SHORT lists (never culled, no list launches): the last line block of the pre-pass launch to finish lists the lines with a wide
    // window per line subset of the wide role (LineWork::n_csplit; in the space long lists keep hlist in, the counts and offsets where
    // the list launches keep their per-block counts) and the wide role walks that list instead of every line.  Same hits in the
    // same order: scheduling only (context option "wide_list").  Not in the mixed-precision mode, whose fp32 sums are flushed into
    // the fp64 sums at chunk boundaries: other chunks would move those roundings.
    // Automatic rule: from kListAutoChunks chunks of 64 lines per subset on.  Measured (profiles/EXPERIMENTS.md, "Short lists walk a
    // list of their wide lines"): at S-c2 (16 chunks per subset, 2 listed) the line kernel runs 1.2 us faster and the list is built in
    // the shadow of the launch's continuum tiles; at S-c1 (4 per subset, 1 listed) the line kernel gains nothing and the last block's
    // 3 us show at the end of a pre-pass launch whose continuum tiles are done before its line blocks.
    const int wide_splits = req.wide_splits;
    const int64_t chunks_per_subset = wide_splits > 0 ? ((n_lines + 63) / 64 + wide_splits - 1) / wide_splits : 0;
    if (fill_work && wide_splits > 0 && (ctx->wide_list == 1 || (ctx->wide_list < 0 && chunks_per_subset >= kListAutoChunks)) &&
        !ctx->mixed_precision && n_lines > 0 && n_lines < ctx->indexed_min_lines && (n_lines + 63) / 64 <= kListMaxChunks) {
        w.n_csplit = wide_splits;  // (its counter of finished line blocks: `ticket`, set where the launch is enqueued)
    }
    // VERY dense long fp64 lists (>= 4 lines per grid point: the rule of the narrow role's subsets): no narrow records — the narrow role
    // reads the caller's three tables itself (LineWork::narrow_raw).  Pure scheduling (the same three operations form 1 / dw, y and the
    // amplitude either way).  Measured in round 6 (profiles/r06_raw.txt): 1e6 lines on 120 398 points — pre-pass 904 -> 721 us (a stream:
    // 2.13 GB of traffic counted, 1.31 GB of it these records), line kernel 5.93 -> 6.07 ms (ten more instructions per evaluated line), step
    // 7.27 -> 7.24 ms and 1.35 GB less scratch; 1.5e5 lines: pre-pass 165 -> 149 us, line kernel 1.218 -> 1.241 ms, the step 7 us SLOWER —
    // hence the density in the rule.
    const int narrow_records = (int)ctx->narrow_records;  // (context option: -1 by this rule, 0 never, 1 always)
    const bool very_dense = 2 * n_lines >= 8 * n_nu;
    if (fill_work && !l.gen && !ctx->mixed_precision && n_lines >= ctx->indexed_min_lines && (narrow_records == 0 || (very_dense && narrow_records != 1))) {
        w.narrow_raw = l.gamma_cols > 1 ? n_depth : 1;
        w.n_inv = const_cast<double*>(l.doppler);
        w.n_y = const_cast<double*>(l.gammas);
        w.n_amp = const_cast<double*>(l.alphas);
    }
    // long lists find their wide lines through hlist / wlist: the scan words of a line without a wide window anywhere are never
    // read (needs the line's widest window inside one block: one depth block per line)
    w.skip_unlisted_scan = (fill_work && n_lines >= ctx->indexed_min_lines && n_depth <= kPreDepths) ? 1 : 0;
    w.n_pix = s.n_pixel_blocks;
    w.shard_begin = g.nu_begin;
    w.shard_end = g.nu_begin + g.nu_count;
    // A frequency shard of a long list does not need every line prepared: a streaming classification pass finds the lines
    // that can reach any column (-> hlist), the full pre-pass then runs on the lines centred near the shard plus those.
    // Everything is decided on the device (no host round trip, graph-capturable); which lines a shard prepares does not
    // change what it computes for them.  (`cull`, above)
    REQUIRE(!req.ph || cull, "two-collective mode is for frequency shards of long dense line lists (>= indexed_min_lines lines, a grid of more than "
                             "16384 points, nu_count < n_nu, no evaluation count)");
    // the grid-spacing reduction: a launch of its own, or — culled runs — the first blocks of the classification launch
    // (grid-spacing blocks of a classification launch: four pairs of loads per thread — one trip of their loop — up to 256 blocks)
    if (cull) s.n_partial = (int)std::min<int64_t>(kDnuPartials, std::max<int64_t>(1, (n_nu + kBlock * 4 - 1) / (kBlock * 4)));
    // The grid plan (sdx_grid_plan): honoured on the un-culled pre-pass of a dense list next to the tiled continuum — the launch then has
    // no pixel blocks, its line blocks read centres and spacing from the plan and its tiles the per-frequency values
    // (k_prepass_continuum<false, LINES, true>).  Long grids: the grid-spacing launch stays only where it computes the far ranges.
    ContPlan planned_cp;
    bool planned = req.plan && ctx->grid_plan != 0 && fill_work && !cull && !l.gen && req.cont && !req.lo_ref && (s.pre_lines == 16 || s.pre_lines == 32);
    if (planned) {
        const int pix = s.n_pixel_blocks;
        s.n_pixel_blocks = 0;  // (the tiles are sized for the launch without them)
        if ((rc = plan_continuum(ctx, req.cont, g, kPreBlock, s.n_line_blocks, &planned_cp))) return rc;
        planned = planned_cp.tiled;
        if (!planned) s.n_pixel_blocks = pix;
        w.n_pix = s.n_pixel_blocks;
    }
    if (planned) {
        w.cnt_ge = req.plan->i;
        w.centre = req.plan->i + (n_nu + 2);
        // no table in LDS: the bound-free edges instead
        const size_t n_lev = planned_cp.ca.bf_n_species > 0 ? (size_t)req.cont->bf_n_levels : 0;
        planned_cp.shmem = ((size_t)kContDepths * (n_lev + 6) + n_lev) * sizeof(double);
        s.planned = &planned_cp;
    }
    if (!cull && !s.scan_in_block && !(planned && !req.far.count)) {
        if ((rc = launch_dnu(ctx, n_nu, g.nus, &s.n_partial, req.far))) return rc;
        if (req.far.count) s.far_ranges = true;
    }
    if (cull && (rc = prepass_culled(ctx, g, l, req, cnt, s))) return rc;
    if (!(req.ph && req.ph->phase == 1) && (rc = prepass_launch(ctx, g, l, req, s))) return rc;  // (phase 1 ends behind its classification launch)
    if (out) *out = PrepassResult{s.w, s.far_ranges};
    return SDX_OK;
}

static int check_line_args(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines,
                           const double* line_nus, const double* doppler, const double* gammas, int gamma_cols,
                           const double* alphas)
{
    REQUIRE(ctx, "null context");
    REQUIRE(n_depth > 0 && n_nu >= 0 && n_lines >= 0, "line opacity: negative or zero sizes");
    REQUIRE(n_nu < (int64_t)2147483647, "line opacity: n_nu must fit int32");
    REQUIRE(n_lines < (int64_t)2147483647, "line opacity: n_lines must fit int32");
    REQUIRE(gamma_cols == n_depth || gamma_cols == 1, "line opacity: gammas must have n_depth or 1 columns");
    REQUIRE(n_nu == 0 || nus, "line opacity: null frequency grid");
    REQUIRE(n_lines == 0 || (line_nus && doppler && gammas && alphas), "line opacity: null line arrays");
    return SDX_OK;
}

// number of line subsets: enough single-wave blocks to fill the chip when the (tile, depth) grid alone is small
// (decided from the GLOBAL grid size, not the shard's: the partition fixes the summation order of every grid point,
// which must not depend on how the grid is sharded)
static int choose_splits(int n_depth, int64_t n_nu_global, int64_t n_lines, int R, int min_splits)
{
    const int64_t tiles = (n_nu_global + 64 * R - 1) / (64 * R);
    const int64_t chunks = (n_lines + 63) / 64;
    int64_t target = 2560;  // S-c2: 2 subsets (4 measured the same, 8 slower: 40.4 / 40.7 / 50.1 us — the narrow role shares the workgroup size)
    if (const char* e = knob("SDX_WIDE_BLOCKS")) target = std::max(1, std::atoi(e));  // tuning knob
    // at least two subsets (four for long lists): the choice must not depend on the shard (it fixes the summation order), and
    // a rank that owns 1/8 of a large grid still needs enough, small enough waves — a (tile, depth) of S-c3 is ~2e4
    // instructions per subset at S = 2, and a shard's last generation of such waves is most of its run time
    const int64_t want = std::max<int64_t>(min_splits, (target + tiles * n_depth - 1) / (tiles * n_depth));
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, chunks), 8));  // the subsets are the waves of one workgroup
}

// The (ihi, ilo) pair of every GLOBAL tile that holds columns of the launch: the request a step hands to its pre-pass, whose grid-spacing
// launch (launch_dnu, the classification launch of a culled shard) computes them on the side.
static int far_request(sdx_ctx* ctx, const Grid& g, FarReq* req)
{
    int rc = ensure(ctx, &ctx->far_ws, &ctx->far_ws_bytes, (size_t)((g.n_nu + kFarTile - 1) / kFarTile) * 2 * sizeof(int));
    if (rc) return rc;
    const int64_t t_first = g.nu_begin / kFarTile, t_last = (g.nu_begin + g.nu_count - 1) / kFarTile;
    *req = FarReq{(int*)ctx->far_ws, t_first, t_last - t_first + 1};
    return SDX_OK;
}

// pre-pass + the two gather kernels; leaves n_planes partial planes in part ([planes][n_depth][pld]): the wide subsets in subset order,
// then the narrow-window plane.  With req.cont the continuum plane of the fused step is computed by the same launch as the pre-pass.
// (req: count_evals, cont, ph and plan as the caller wants them; the far ranges and the line subsets are asked for here)
struct LinePlanes {
    const double* part;
    int64_t pld;
    int n_planes;
    LineWork w;
};
static int line_partials(sdx_ctx* ctx, const Grid& grid, const Lines& lines, PrepassRequest req, LinePlanes* out)
{
    const int n_depth = grid.n_depth;
    const int64_t n_nu = grid.n_nu, nu_begin = grid.nu_begin, nu_count = grid.nu_count, n_lines = lines.n_lines;
    const double *const nus = grid.nus, *const line_nus = lines.line_nus;
    // grid points per lane of a wide-role tile (tile = 64 R points), in every mode (fp32 far wings with 8 — twice the points per fetched
    // record — were measured slower: fewer tiles qualify as far wing)
    constexpr int R = 4;
    const bool far = far_field_on(ctx, n_nu) && nu_count > 0;
    int rc;
    // (phase 1 computed the ranges — with the far field on then; if the option was switched on in between, k_far_ranges below does it)
    const bool classified_far = req.ph && req.ph->phase == 2 && ctx->classified.valid && ctx->classified.far && ctx->classified.far_ranges;
    if (far && !classified_far && (rc = far_request(ctx, grid, &req.far))) return rc;
    // (the number of line subsets depends on the global grid and the list alone; the pre-pass of a short list sorts its wide lines by it)
    const int n_split = req.wide_splits = choose_splits(n_depth, n_nu, n_lines, R, n_lines >= ctx->indexed_min_lines ? 4 : 2);
    PrepassResult pre;
    if ((rc = line_prepass(ctx, grid, lines, req, &pre))) return rc;
    LineWork& w = pre.w;
    const bool far_ranges_done = pre.far_ranges || classified_far;  // else k_far_ranges below computes them
    // long line lists: the lines with a window wider than kMediumHalfWidth are listed once (they are scanned by every tile);
    // all others are found by centre range.  Short lists are scanned completely, or — where the pre-pass has listed their wide lines
    // (LineWork::n_csplit, option "wide_list") — through that list: no further launch either way.
    const int indexed = n_lines >= ctx->indexed_min_lines ? 1 : 0;
    if (indexed && !w.hlist) {  // (a culled pre-pass has built the lists already)
        LaunchScope ls(ctx, "k_hlist");
        launch_line_lists(ctx, CntLayout(n_nu, n_lines), w, 32, nullptr);
    }
    if (indexed && !w.sel) {  // the huge lines' scan words in list order (a culled pre-pass has written them itself)
        LaunchScope ls(ctx, "k_hlist");
        hipLaunchKernelGGL(k_hscan, dim3(64, (unsigned)n_depth), dim3(kBlock), 0, ctx->stream, n_depth, n_lines, (const int*)w.hlist, (const int*)w.hcount,
                           (const WideScan*)w.wscan, w.hscan);
    }
    // two planes: [0] wide windows (the S subsets are summed inside their workgroup), [1] narrow windows.  (Twice the line subsets
    // for the deepest, hottest layers — two workgroups per (depth, tile), a third plane for the second halves — was measured in
    // round 4 at S-c3 and on its eight shards with 0 / 14 / 28 such layers: line kernel 2026 / 2048 / 2092 us unsharded, 332 / 344 /
    // 346 us on the slowest shard, no change at S-c2 either: the hit lists fall off by only a factor 4 from the deepest to the
    // shallowest layer, and a launch is bound by its total work, not by its heaviest wave.  Removed.)
    w.far_range = nullptr;
    if (far) {
        if (!far_ranges_done) {  // (no grid-spacing launch in this step: small grids scan the spacing inside the pre-pass blocks)
            LaunchScope ls(ctx, "k_far_ranges");
            hipLaunchKernelGGL(k_far_ranges, dim3((unsigned)((2 * req.far.count + kBlock / 16 - 1) / (kBlock / 16))), dim3(kBlock), 0, ctx->stream, n_nu, nus, req.far);
        }
        w.far_range = (const int*)ctx->far_ws;
    }
    rc = ensure(ctx, &ctx->part_ws, &ctx->part_ws_bytes, (size_t)(far ? 3 : 2) * n_depth * nu_count * sizeof(double));
    if (rc) return rc;
    double* part = (double*)ctx->part_ws;
    const int64_t pld = nu_count;
    // tiles are aligned to the GLOBAL grid (multiples of 64 R points from index 0), whatever the shard: which points share a
    // tile — and with it how a (line, depth, tile) is classified and which points share a reciprocal — is a property of the grid.
    // Order of the wide role's tiles over the XCDs: one contiguous eighth each (groups of g tiles going round them — better balance
    // where an eighth is only a few tiles, a shard's, at the price of fewer neighbouring tiles per L2 — ran the line
    // launch of two such shards 2 - 24 % slower: profiles/r06_roles2.txt).
    // Workgroups of n_split waves, rounded up to whole rounds of the XCD-aware order (surplus workgroups return at once).
    // Narrow role: F consecutive frequencies per wave (a line's records, loaded once, serve F evaluations) for DENSE lists —
    // at least one line per two grid points, where a frequency visits many lines and the walk is bound by its loads and
    // instructions — as long as >= 8192 such waves remain: an eighth of S-c3 (11 000 - 21 000 columns) with F = 4 ran its
    // line kernel 20 % SLOWER (414 against 345 us: a few thousand four-times-longer waves are the launch's tail); sparse lists
    // on small grids (S-c2: 2000 lines on 7634 points, a latency-bound launch) keep one frequency per wave.  Pure scheduling:
    // every frequency adds its lines in the same order whatever F.  (F = 8 was measured slower than 4 at every size.)
    int narrow_f = 1;
    if (2 * n_lines >= n_nu) narrow_f = nu_count >= 32768 ? 4 : (nu_count >= 16384 ? 2 : 1);
    // VERY dense long lists (>= 4 lines per grid point, four line subsets): the four waves of a narrow-role workgroup share one group
    // of four frequencies and split its candidate lines (line_narrow_subsets) — the record sharing of F = 4 with the wave count of
    // F = 1, whatever the width of the launch.  Decided from the global list and grid: it changes the order of a sum.  Measured in
    // round 5: 1e6 lines on 120 398 points (8.3 per point) 10.2 -> 9.9 ms for the whole grid and 1.52 -> 1.36 ms on an eighth; 1.5e5
    // lines (1.25 per point: ~17 lines per wave, less than the wave's start-up and the workgroup's reduction) 2.03 -> 2.20 ms and
    // 311 -> 320 us — hence the density in the rule.
    const int narrow_sub = (2 * n_lines >= 8 * n_nu && n_split == 4) ? 4 : 0;
    if (narrow_sub) narrow_f = 4;
    // (the narrow workgroups come in whole rounds of the XCD-aware order: line_launch_make, sdx_line_geom.h)
    static const bool split_launches = knob("SDX_SPLIT_LAUNCHES") != nullptr;  // analysis knob: time the two roles apart
    size_t shmem = (size_t)n_split * (far && SDX_WIDE_QUEUED ? kWideFarLdsDoubles : kWideLdsDoubles) * sizeof(double);
    // FAR FIELD: units of 4 RF global tiles; RF (1 or 2 node groups per lane) is scheduling only (4 was measured slower than 2 at every
    // size).  Its workgroups are the FIRST of the line kernel's grid (one launch, and a shard's far waves — the launch's longest chains —
    // run beside the other roles instead of alone on the chip: as a launch of their own they lost, profiles/r06_roles.txt).  The number of
    // line subsets fixes the order of a node's sum: n_split, the line kernel's.
    // (round 6: units of 8 tiles at every size — on the eighths of S-c3 / S-c4m, where an earlier rule chose 4, the line launch ran 2 - 5 %
    // faster with 8: half as many waves walk the huge lines' scan words; profiles/r06_far_rf.txt)
    constexpr int far_rf = 2;
    const int64_t far_units = far ? (nu_begin + nu_count - 1) / (64 * R) / (4 * far_rf) - nu_begin / (64 * R) / (4 * far_rf) + 1 : 0;
    if (far) shmem = std::max(shmem, (((size_t)n_split + 2) * far_rf * 64 + (size_t)n_split * kFarWaveLdsDoubles) * sizeof(double));
    // (the far role on a second stream beside the other two — a fork and a join per step — was measured in round 5: S-c3 1.857 -> 1.840 ms,
    // its eighth 0.419 -> 0.420, S-c4m 7.49 -> 7.48: both are bound by their instructions, neither leaves the other idle slots)
    for (int pass = 0; pass < (split_launches ? 2 : 1); ++pass) {
        // (raising the priority of the hot layers' waves with s_setprio was measured in round 4: the instruction has side effects as
        // far as the compiler is concerned, the record fetches of the walk stopped being scalar loads and the kernel ran 37 % slower)
        // The launch's geometry, formed here on the host (sdx_line_geom.h): which block is which role's which unit — tiles aligned to the global
        // grid, the XCD-aware orders of both roles, the narrow role's groups of F frequencies — so that no wave divides by a launch
        // constant.  It also states the range: grid, units and frequency indices stay 32-bit.
        // (split launches: one role live in each; the far role's workgroups are in front of the first, the wide role's, and nowhere in the
        // second: the same units with the same subsets as in the one launch, so the same three planes)
        const bool far_front = far && pass == 0;
        const LineLaunch launch = line_launch_make(nu_begin, nu_count, n_depth, n_split, 64 * R, narrow_f, narrow_sub != 0, 0, 0,
                                                   split_launches ? (pass ? kLineRoleNarrow : kLineRoleWide) : kLineRoleWide | kLineRoleNarrow,
                                                   far_front ? far_units * n_depth : 0);
        REQUIRE(launch.ok, "line opacity: grid too large for one launch");
        const LineGeom& geom = launch.g;
        const dim3 g((unsigned)launch.blocks), blk((unsigned)(64 * n_split));
        LaunchScope ls(ctx, split_launches ? (pass ? "k_line_narrow" : "k_line_wide") : "k_line_all", far_front ? "k_line_all + far role" : nullptr);
        // (the kernels with a far field decode the launch themselves: LineWords, sdx_kernels.h — the same grid and the same units)
        const LineWords words{geom.narrow_first - geom.wide_first, (int)(((nu_begin + nu_count + 64 * R - 1) / (64 * R)) - nu_begin / (64 * R)),
                              (split_launches ? (1 << pass) : 3) | (narrow_f << 8) | ((far_front ? far_rf : 0) << 16), (int)far_units};
#define SDX_LINE_TAIL n_split, n_depth, n_nu, nus, nu_begin, nu_count, n_lines, line_nus, w, part, pld
#define SDX_LINE_ARGS geom, SDX_LINE_TAIL
#define SDX_LINE_FAR_ARGS words, SDX_LINE_TAIL
        if (ctx->mixed_precision && narrow_sub && far) hipLaunchKernelGGL((k_line_all_mixed<R, true, true>), g, blk, shmem, ctx->stream, SDX_LINE_FAR_ARGS);
        else if (ctx->mixed_precision && narrow_sub) hipLaunchKernelGGL((k_line_all_mixed<R, true>), g, blk, shmem, ctx->stream, SDX_LINE_ARGS);
        else if (ctx->mixed_precision && far) hipLaunchKernelGGL((k_line_all_mixed<R, false, true>), g, blk, shmem, ctx->stream, SDX_LINE_FAR_ARGS);
        else if (ctx->mixed_precision) hipLaunchKernelGGL((k_line_all_mixed<R>), g, blk, shmem, ctx->stream, SDX_LINE_ARGS);
        else if (w.n_csplit && narrow_sub && far) hipLaunchKernelGGL((k_line_listed<R, true, true>), g, blk, shmem, ctx->stream, SDX_LINE_FAR_ARGS);
        else if (w.n_csplit && narrow_sub) hipLaunchKernelGGL((k_line_listed<R, true>), g, blk, shmem, ctx->stream, SDX_LINE_ARGS);
        else if (w.n_csplit && far) hipLaunchKernelGGL((k_line_listed<R, false, true>), g, blk, shmem, ctx->stream, SDX_LINE_FAR_ARGS);
        else if (w.n_csplit) hipLaunchKernelGGL((k_line_listed<R>), g, blk, shmem, ctx->stream, SDX_LINE_ARGS);
        else if (narrow_sub && far) hipLaunchKernelGGL((k_line_all<R, true, true>), g, blk, shmem, ctx->stream, SDX_LINE_FAR_ARGS);
        else if (narrow_sub) hipLaunchKernelGGL((k_line_all<R, true>), g, blk, shmem, ctx->stream, SDX_LINE_ARGS);
        else if (far) hipLaunchKernelGGL((k_line_all<R, false, true>), g, blk, shmem, ctx->stream, SDX_LINE_FAR_ARGS);
        else hipLaunchKernelGGL((k_line_all<R>), g, blk, shmem, ctx->stream, SDX_LINE_ARGS);
#undef SDX_LINE_ARGS
#undef SDX_LINE_FAR_ARGS
#undef SDX_LINE_TAIL
    }
    *out = LinePlanes{part, pld, far ? 3 : 2, w};
    return check_launch("line kernels");
}

static int line_opacity_impl(sdx_ctx* ctx, const Grid& g, const Lines& lines, double* out, int64_t out_ld, int accumulate, int64_t* n_evaluations_dev)
{
    int rc;
    const int n_depth = g.n_depth;
    const int64_t nu_count = g.nu_count;
    REQUIRE(g.nu_begin >= 0 && nu_count >= 0 && g.nu_begin + nu_count <= g.n_nu, "line opacity: shard outside the grid");
    REQUIRE(nu_count == 0 || (out && out_ld >= nu_count), "line opacity: bad output buffer");
    if (nu_count == 0) return SDX_OK;
    if (lines.n_lines == 0) {
        if (!accumulate) HIP_TRY(hipMemset2DAsync(out, out_ld * sizeof(double), 0, nu_count * sizeof(double), n_depth, ctx->stream));
        if (n_evaluations_dev) HIP_TRY(hipMemsetAsync(n_evaluations_dev, 0, sizeof(int64_t), ctx->stream));
        return SDX_OK;
    }
    PrepassRequest req{};
    req.count_evals = n_evaluations_dev != nullptr;
    LinePlanes p;
    if ((rc = line_partials(ctx, g, lines, req, &p))) return rc;
    {
        LaunchScope ls(ctx, "k_reduce_partials");
        hipLaunchKernelGGL(k_reduce_partials, grid2(nu_count, n_depth), dim3(kBlock), 0, ctx->stream, n_depth, nu_count, p.n_planes,
                           p.part, p.pld, out, out_ld, accumulate);
    }
    rc = check_launch("k_reduce_partials");
    if (rc) return rc;
    if (n_evaluations_dev)
        HIP_TRY(hipMemcpyAsync(n_evaluations_dev, p.w.evals, sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
    return SDX_OK;
}

int sdx_line_opacity_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                         int64_t n_lines, const double* line_nus, const double* doppler, const double* gammas,
                         int gamma_cols, const double* alphas, double* out, int64_t out_ld, int accumulate,
                         int64_t* n_evaluations_dev)
{
    int rc = check_line_args(ctx, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas);
    if (rc) return rc;
    return line_opacity_impl(ctx, Grid{n_depth, n_nu, nus, nu_begin, nu_count}, Lines{n_lines, line_nus, doppler, gammas, gamma_cols, alphas, nullptr}, out,
                             out_ld, accumulate, n_evaluations_dev);
}

// ---- line parameters generated on the device: an sdx_linelist as the line kernels' description (*lp) and as the lines
// of a call — no dense tables, generated from *lp, which must outlive *lines; gammas in n_depth columns or one
static int to_line_params(const sdx_linelist* ll, int n_depth, LineParams* lp, Lines* lines)
{
    REQUIRE(ll, "line list: null description");
    REQUIRE(ll->n_lines >= 0 && ll->n_lines < (int64_t)2147483647 && n_depth > 0, "line list: bad sizes (n_lines must fit int32)");
    REQUIRE(ll->gamma_mode >= 0 && ll->gamma_mode <= 3, "line list: gamma_mode must be 0..3");
    *lines = Lines{ll->n_lines, ll->nu, nullptr, nullptr, ll->gamma_mode >= 2 ? 1 : n_depth, nullptr, lp};
    if (ll->n_lines == 0) return SDX_OK;
    REQUIRE(ll->nu && ll->e_low_ev && ll->strength && ll->pop_row && ll->pop && ll->mass && ll->temperature,
            "line list: null alpha_line / doppler inputs");
    REQUIRE(ll->n_pop_rows > 0, "line list: n_pop_rows must be positive");
    if (ll->gamma_mode <= 1) {
        REQUIRE(ll->atomic_number && ll->ion_number && ll->ionization_energy && ll->upper_energy && ll->lower_energy && ll->A_ul &&
                    ll->electron_density && ll->h_density,
                "line list: null broadening inputs");
        REQUIRE(ll->gamma_mode == 0 || (ll->stark && ll->waals), "line list: VALD broadening needs stark and waals");
    }
    REQUIRE(ll->gamma_mode != 2 || ll->A_ul, "line list: gamma_mode 2 needs A_ul");
    lp->e_low_ev = ll->e_low_ev;
    lp->g_lo = ll->g_lo;
    lp->strength = ll->strength;
    lp->pop_row = (const int*)ll->pop_row;
    lp->pop = ll->pop;
    lp->alpha_coefficient = ll->alpha_coefficient;
    lp->mass = ll->mass;
    lp->xi = ll->microturbulence;
    lp->gamma_mode = ll->gamma_mode;
    lp->flags = ll->broadening_flags;
    lp->z = (const int*)ll->atomic_number;
    lp->ion = (const int*)ll->ion_number;
    lp->e_ion = ll->ionization_energy;
    lp->e_up = ll->upper_energy;
    lp->e_lo = ll->lower_energy;
    lp->a_ul = ll->A_ul;
    lp->stark = ll->stark;
    lp->waals = ll->waals;
    lp->temps = ll->temperature;
    lp->n_e = ll->electron_density;
    lp->n_h = ll->h_density;
    return SDX_OK;
}

int sdx_line_params_dev(sdx_ctx* ctx, int n_depth, const sdx_linelist* ll, double* alphas, double* gammas, double* doppler)
{
    REQUIRE(ctx, "null context");
    LineParams lp{};
    Lines l;
    int rc = to_line_params(ll, n_depth, &lp, &l);
    if (rc) return rc;
    if (l.n_lines == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_line_params");
        hipLaunchKernelGGL(k_line_params, dim3(blocks1(l.n_lines * n_depth)), dim3(kBlock), 0, ctx->stream, l.n_lines, n_depth, l.line_nus,
                           lp, alphas, gammas, l.gamma_cols, doppler);
    }
    return check_launch("k_line_params");
}

int sdx_alpha_line_levels_dev(sdx_ctx* ctx, int64_t n_lines, int n_depth, int n_levels, const double* level_density,
                              const int32_t* lower_index, const double* stim, const double* f_lu, double alpha_coefficient,
                              double* alphas)
{
    REQUIRE(ctx && n_lines >= 0 && n_depth > 0 && n_levels >= 0, "alpha_line_levels: bad sizes");
    if (n_lines == 0) return SDX_OK;
    REQUIRE(level_density && lower_index && stim && f_lu && alphas && n_levels > 0, "alpha_line_levels: null pointer");
    {
        LaunchScope ls(ctx, "k_alpha_line_levels");
        hipLaunchKernelGGL(k_alpha_line_levels, dim3(blocks1(n_lines * n_depth)), dim3(kBlock), 0, ctx->stream, n_lines, n_depth, level_density,
                           (const int*)lower_index, stim, f_lu, alpha_coefficient, alphas);
    }
    return check_launch("k_alpha_line_levels");
}

int sdx_line_opacity_linelist_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                                  const sdx_linelist* ll, double* out, int64_t out_ld, int accumulate, int64_t* n_evaluations_dev)
{
    REQUIRE(ctx, "null context");
    REQUIRE(n_depth > 0 && n_nu >= 0 && n_nu < (int64_t)2147483647, "line opacity: bad sizes");
    REQUIRE(n_nu == 0 || nus, "line opacity: null frequency grid");
    LineParams lp{};
    Lines lines;
    int rc = to_line_params(ll, n_depth, &lp, &lines);
    if (rc) return rc;
    return line_opacity_impl(ctx, Grid{n_depth, n_nu, nus, nu_begin, nu_count}, lines, out, out_ld, accumulate, n_evaluations_dev);
}

int sdx_line_windows_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                         const double* doppler, const double* gammas, int gamma_cols, const double* alphas, int32_t* lower,
                         int32_t* upper)
{
    int rc = check_line_args(ctx, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas);
    if (rc) return rc;
    REQUIRE(n_lines == 0 || (lower && upper), "line windows: null output");
    if (n_lines == 0) return SDX_OK;
    PrepassRequest req{};  // no continuum, no far ranges
    req.lo_ref = lower, req.hi_ref = upper, req.count_evals = true;
    return line_prepass(ctx, Grid{n_depth, n_nu, nus, 0, n_nu}, Lines{n_lines, line_nus, doppler, gammas, gamma_cols, alphas, nullptr}, req, nullptr);
}

// Host-pointer (*_f64) entry points — what a numpy caller (the reference's calc_alpha_line_at_nu, base.py:432-439) binds.
// Each one is: check, declare the rows of the call in a HostPlan (sdx_host_plan.h: in / out / inout / scratch, in the order they sit
// on the device), stage, the device entry, collect, finish.  The plan's one layout pass gives every row its place and the call its two
// sizes, so what is reserved and what is copied are read from the same rows; absent rows (null host pointers) get a null device
// pointer and take nothing.  The device buffers are sub-allocated from ONE arena owned by the context and the transfers go through ONE
// pinned host buffer, both grown on demand and kept across calls: a call costs no hipMalloc / hipFree and every copy is a DMA from / to
// page-locked memory.  Inputs: memcpy user -> pinned, async DMA pinned -> device (the DMA of array k overlaps the memcpy of
// array k + 1).  Outputs: async DMA device -> pinned, one synchronize, memcpy pinned -> user.  Transfers beyond
// kPinnedStagingMax go straight from / to the caller's pages (the runtime pins them on the fly).
constexpr size_t kPinnedStagingMax = (size_t)512 << 20;

struct HostIo {
    sdx_ctx* ctx;
    struct Pending {
        void* dst;
        const void* src_pin;
        size_t bytes;      // bytes per row
        size_t rows;       // rows of `bytes`, packed in the pinned buffer, dst_pitch apart in the destination
        size_t dst_pitch;
    };
    std::vector<Pending> pending;
    bool finished = false;

    explicit HostIo(sdx_ctx* c) : ctx(c) {}
    HostIo(const HostIo&) = delete;
    HostIo& operator=(const HostIo&) = delete;
    // error exits return before finish(): DMAs out of / into the context's pinned buffer may still be in flight, and the next
    // call would memcpy new data over them
    ~HostIo()
    {
        if (!finished) hipStreamSynchronize(ctx->stream);
    }

    // lays the plan out, grows the arena and the pinned buffer to it, enqueues the uploads and sets every row's device pointer
    // (after growing: the arena may have moved)
    int stage(HostPlan& plan)
    {
        static const bool no_pin = knob("SDX_NO_PINNED_STAGING") != nullptr;
        plan.layout(no_pin ? 0 : kPinnedStagingMax);
        if (ctx->io_dev_bytes < plan.dev_need) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (ctx->io_dev) HIP_TRY(hipFree(ctx->io_dev));
            ctx->io_dev = nullptr;
            ctx->io_dev_bytes = 0;
            const size_t want = plan.dev_need + plan.dev_need / 4;  // head-room: repeated calls with slowly growing sizes do not reallocate each time
            HIP_TRY(hipMalloc(&ctx->io_dev, want));
            ctx->io_dev_bytes = want;
        }
        if (ctx->io_pin_bytes < plan.pin_need) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (ctx->io_pin) HIP_TRY(hipHostFree(ctx->io_pin));
            ctx->io_pin = nullptr;
            ctx->io_pin_bytes = 0;
            const size_t want = plan.pin_need + plan.pin_need / 4;
            HIP_TRY(hipHostMalloc(&ctx->io_pin, want, hipHostMallocDefault));
            ctx->io_pin_bytes = want;
        }
        // the growth above makes this hold; no copy is issued on the strength of that alone
        if (plan.dev_need > ctx->io_dev_bytes || plan.pin_need > ctx->io_pin_bytes)
            return fail(SDX_ERR_OOM, "host staging: the call's plan does not fit the context's buffers");
        plan.bind(ctx->io_dev);
        for (const HostPlan::Row& r : plan.rows) {
            if (!r.uploads()) continue;
            const void* from = r.src;
            if (plan.staged) {
                void* h = (char*)ctx->io_pin + r.up_off;
                std::memcpy(h, r.src, r.bytes);
                from = h;
            }
            HIP_TRY(hipMemcpyAsync((char*)ctx->io_dev + r.dev_off, from, r.bytes, hipMemcpyHostToDevice, ctx->stream));
        }
        return SDX_OK;
    }
    // enqueues the downloads of the plan that was staged
    int collect(const HostPlan& plan)
    {
        for (const HostPlan::Row& r : plan.rows) {
            if (!r.downloads()) continue;
            const void* d = (const char*)ctx->io_dev + r.dev_off;
            if (plan.staged) {
                void* h = (char*)ctx->io_pin + r.down_off;
                HIP_TRY(hipMemcpyAsync(h, d, r.bytes, hipMemcpyDeviceToHost, ctx->stream));
                pending.push_back({r.dst, h, r.bytes / r.rows, r.rows, r.dst_pitch});
            } else if (r.rows == 1) {
                HIP_TRY(hipMemcpyAsync(r.dst, d, r.bytes, hipMemcpyDeviceToHost, ctx->stream));
            } else {
                HIP_TRY(hipMemcpy2DAsync(r.dst, r.dst_pitch, d, r.bytes / r.rows, r.bytes / r.rows, r.rows, hipMemcpyDeviceToHost, ctx->stream));
            }
        }
        return SDX_OK;
    }
    int finish()
    {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        finished = true;
        for (auto& p : pending)
            for (size_t r = 0; r < p.rows; ++r) std::memcpy((char*)p.dst + r * p.dst_pitch, (const char*)p.src_pin + r * p.bytes, p.bytes);
        pending.clear();
        return SDX_OK;
    }
};

static int host_grid_check(int64_t n_nu, const double* nus)
{
    for (int64_t i = 0; i + 1 < n_nu; ++i)
        if (!(nus[i + 1] < nus[i])) return fail(SDX_ERR_ARG, "tracing frequencies must be strictly descending (stardis/base.py:34)");
    return SDX_OK;
}

// The kernels take the line list in ascending frequency (calc_alpha_line_at_nu sorts it, base.py:392-397): cnt_ge is a
// binary search over line_nus and the narrow role walks a contiguous index range per frequency.
// ... and no Doppler width [n_lines][n_depth] may be zero
static int host_lines_check(int64_t n_lines, const double* line_nus, const double* doppler, int n_depth)
{
    for (int64_t l = 0; l + 1 < n_lines; ++l)
        if (!(line_nus[l + 1] >= line_nus[l]))
            return fail(SDX_ERR_ARG, "line_nus must be ascending (sort the line list by frequency, opacities_solvers/base.py:392-397)");
    for (int64_t k = 0; k < n_lines * n_depth; ++k)
        if (doppler[k] == 0.0) return fail(SDX_ERR_ARG, "doppler_width == 0 (ZeroDivisionError in the reference, voigt.py:148)");
    return SDX_OK;
}

int sdx_line_opacity_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                         const double* doppler, const double* gammas, int gamma_cols, const double* alphas, double* out,
                         int64_t* n_evaluations)
{
    int rc = check_line_args(ctx, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas);
    if (rc) return rc;
    REQUIRE(n_nu == 0 || out, "line opacity: null output");
    if ((rc = host_grid_check(n_nu, nus))) return rc;
    if ((rc = host_lines_check(n_lines, line_nus, doppler, n_depth))) return rc;
    if (n_nu == 0) {  // nothing to stage, as for the formal solution and the synthesis on an empty grid
        if (n_evaluations) *n_evaluations = 0;
        return SDX_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), ld = (size_t)n_lines * n_depth * f8;
    const double *d_nus, *d_ln, *d_dw, *d_g, *d_a;
    double* d_out;
    int64_t ev = 0, *d_ev;
    HostPlan plan;
    plan.in(nus, (size_t)n_nu * f8, &d_nus);
    plan.in(line_nus, (size_t)n_lines * f8, &d_ln);
    plan.in(doppler, ld, &d_dw);
    plan.in(gammas, (size_t)n_lines * gamma_cols * f8, &d_g);
    plan.in(alphas, ld, &d_a);
    plan.out(out, (size_t)n_depth * n_nu * f8, &d_out);
    plan.out(&ev, sizeof ev, &d_ev);
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_line_opacity_dev(ctx, n_depth, n_nu, d_nus, 0, n_nu, n_lines, d_ln, d_dw, d_g, gamma_cols, d_a, d_out, n_nu, 0, d_ev))) return rc;
    if ((rc = io.collect(plan)) || (rc = io.finish())) return rc;
    if (n_evaluations) *n_evaluations = ev;
    return SDX_OK;
}

int sdx_faddeeva_dev(sdx_ctx* ctx, int64_t n, const double* z, double* w)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (z && w)), "faddeeva: bad arguments");
    if (n == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_faddeeva");
        hipLaunchKernelGGL(k_faddeeva, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, z, w);
    }
    return check_launch("k_faddeeva");
}

int sdx_voigt_profile_dev(sdx_ctx* ctx, int64_t n, const double* dnu, const double* dw, const double* gamma, double* phi)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (dnu && dw && gamma && phi)), "voigt_profile: bad arguments");
    if (n == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_voigt_profile");
        hipLaunchKernelGGL(k_voigt_profile, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, dnu, dw, gamma, phi);
    }
    return check_launch("k_voigt_profile");
}

int sdx_voigt_term_dev(sdx_ctx* ctx, int64_t n, const double* delta_nu, const double* inv_doppler_width, const double* y,
                       const double* amp, double* out)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (delta_nu && inv_doppler_width && y && amp && out)), "voigt_term: bad arguments");
    if (n == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_voigt_term");
        hipLaunchKernelGGL(k_voigt_term, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, delta_nu, inv_doppler_width, y, amp, out);
    }
    return check_launch("k_voigt_term");
}

int sdx_voigt_term_f32_dev(sdx_ctx* ctx, int64_t n, const double* delta_nu, const double* inv_doppler_width, const double* y,
                           const double* amp, double* out)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (delta_nu && inv_doppler_width && y && amp && out)), "voigt_term_f32: bad arguments");
    if (n == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_voigt_term32");
        hipLaunchKernelGGL(k_voigt_term32, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, delta_nu, inv_doppler_width, y, amp, out);
    }
    return check_launch("k_voigt_term32");
}

int sdx_voigt_grad_dev(sdx_ctx* ctx, int64_t n, const double* delta_nu, const double* inv_doppler_width, const double* y, const double* amp,
                       double* out_k, double* out_kx, double* out_ky)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (delta_nu && inv_doppler_width && y && amp && out_k && out_kx && out_ky)), "voigt_grad: bad arguments");
    if (n == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_voigt_grad");
        hipLaunchKernelGGL(k_voigt_grad, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, delta_nu, inv_doppler_width, y, amp, out_k, out_kx, out_ky);
    }
    return check_launch("k_voigt_grad");
}

// ================================================================================================ broadening
int sdx_calc_gamma_dev(sdx_ctx* ctx, int64_t n_lines, int n_depth, const int32_t* z, const int32_t* ion, const double* e_ion,
                       const double* e_up, const double* e_lo, const double* a_ul, const double* ne, const double* temps,
                       const double* nh, int flags, double* gammas)
{
    REQUIRE(ctx && n_lines >= 0 && n_depth > 0, "calc_gamma: bad sizes");
    if (n_lines == 0) return SDX_OK;
    REQUIRE(z && ion && e_ion && e_up && e_lo && a_ul && ne && temps && nh && gammas, "calc_gamma: null pointer");
    {
        LaunchScope ls(ctx, "k_calc_gamma");
        hipLaunchKernelGGL(k_calc_gamma, dim3(blocks1(n_lines * n_depth)), dim3(kBlock), 0, ctx->stream, n_lines, n_depth,
                           (const int*)z, (const int*)ion, e_ion, e_up, e_lo, a_ul, ne, temps, nh, flags, gammas);
    }
    return check_launch("k_calc_gamma");
}

int sdx_doppler_widths_dev(sdx_ctx* ctx, int64_t n_lines, int n_depth, const double* line_nus, const double* mass,
                           const double* temps, double microturbulence, double* out)
{
    REQUIRE(ctx && n_lines >= 0 && n_depth > 0, "doppler_widths: bad sizes");
    if (n_lines == 0) return SDX_OK;
    REQUIRE(line_nus && mass && temps && out, "doppler_widths: null pointer");
    {
        LaunchScope ls(ctx, "k_doppler_widths");
        hipLaunchKernelGGL(k_doppler_widths, dim3(blocks1(n_lines * n_depth)), dim3(kBlock), 0, ctx->stream, n_lines, n_depth,
                           line_nus, mass, temps, microturbulence, out);
    }
    return check_launch("k_doppler_widths");
}

int sdx_calc_vald_gamma_dev(sdx_ctx* ctx, int64_t n_lines, int n_depth, const int32_t* z, const int32_t* ion,
                            const double* e_ion, const double* e_up, const double* e_lo, const double* a_ul,
                            const double* stark, const double* waals, const double* mass, const double* ne,
                            const double* temps, const double* nh, int flags, double* gammas)
{
    REQUIRE(ctx && n_lines >= 0 && n_depth > 0, "calc_vald_gamma: bad sizes");
    if (n_lines == 0) return SDX_OK;
    REQUIRE(z && ion && e_ion && e_up && e_lo && a_ul && stark && waals && mass && ne && temps && nh && gammas,
            "calc_vald_gamma: null pointer");
    {
        LaunchScope ls(ctx, "k_calc_vald_gamma");
        hipLaunchKernelGGL(k_calc_vald_gamma, dim3(blocks1(n_lines * n_depth)), dim3(kBlock), 0, ctx->stream, n_lines,
                           n_depth, (const int*)z, (const int*)ion, e_ion, e_up, e_lo, a_ul, stark, waals, mass, ne, temps, nh,
                           flags, gammas);
    }
    return check_launch("k_calc_vald_gamma");
}

int sdx_broadening_scalar_dev(sdx_ctx* ctx, int op, int64_t n, const double* a, const double* b, const double* c,
                              const double* d, const double* e, double* out)
{
    REQUIRE(ctx && op >= 0 && op <= 4 && n >= 0, "broadening_scalar: bad arguments");
    if (n == 0) return SDX_OK;
    REQUIRE(a && b && c && out && (op == kOpNEff || op == kOpLinearStark || d) && (op < kOpQuadraticStark || e),
            "broadening_scalar: null pointer");
    {
        LaunchScope ls(ctx, "k_broadening_scalar");
        hipLaunchKernelGGL(k_broadening_scalar, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, op, n, a, b, c, d, e, out);
    }
    return check_launch("k_broadening_scalar");
}

// ================================================================================================ continuum
static int launch_source(sdx_ctx* ctx, const char* name, int src, int n_depth, int64_t n_nu, const double* nus,
                         const ContinuumArgs& a, double* out, int64_t ld)
{
    REQUIRE(n_depth > 0 && n_nu >= 0 && (n_nu == 0 || (out && ld >= n_nu)), "continuum: bad output");
    if (n_nu == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, name);
        hipLaunchKernelGGL(k_continuum_source, grid2(n_nu, n_depth), dim3(kBlock), 0, ctx->stream, src, n_depth, n_nu, nus, a,
                           out, ld);
    }
    return check_launch(name);
}

int sdx_alpha_file_1d_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* lambdas, int n_table, const double* tab_x,
                          const double* tab_y, const double* density, double* out, int64_t ld)
{
    REQUIRE(ctx && lambdas && tab_x && tab_y && density && n_table > 0, "alpha_file_1d: bad arguments");
    ContinuumArgs a{};
    a.lambdas = lambdas;
    a.n_table = n_table;
    a.table_wavelength = tab_x;
    a.table_sigma = tab_y;
    a.table_density = density;
    return launch_source(ctx, "k_alpha_file_1d", kSrcFile1d, n_depth, n_nu, nullptr, a, out, ld);
}

int sdx_alpha_file_2d_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* sigma, int64_t sigma_ld,
                          const double* density, double* out, int64_t ld)
{
    REQUIRE(ctx && n_depth > 0 && n_nu >= 0 && sigma && density && out && sigma_ld >= n_nu && ld >= n_nu,
            "alpha_file_2d: bad arguments");
    if (n_nu == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_scale_rows");
        hipLaunchKernelGGL(k_scale_rows, grid2(n_nu, n_depth), dim3(kBlock), 0, ctx->stream, n_depth, n_nu, sigma, sigma_ld,
                           density, out, ld);
    }
    return check_launch("k_scale_rows");
}

int sdx_sigma_table_2d_dev(sdx_ctx* ctx, int n_x, const double* x_axis, int n_y, const double* y_axis, const int32_t* cell_simplices,
                           const double* transform, const double* simplex_values, int n_depth, int64_t n_nu, const double* lambdas,
                           const double* second, int scale_kind, const double* temperature, double* sigma, int64_t ld,
                           int32_t* zero_rows)
{
    REQUIRE(ctx && n_x >= 2 && n_y >= 2 && n_x <= kTableAxisMax, "sigma_table_2d: table axes must have 2..512 nodes");
    REQUIRE(x_axis && y_axis && cell_simplices && transform && simplex_values, "sigma_table_2d: null table");
    REQUIRE(n_depth > 0 && n_nu >= 0 && scale_kind >= 0 && scale_kind <= 2, "sigma_table_2d: bad sizes");
    REQUIRE(scale_kind != 2 || temperature, "sigma_table_2d: scale_kind 2 needs the temperatures");
    if (n_nu == 0) return SDX_OK;
    REQUIRE(lambdas && second && sigma && ld >= n_nu, "sigma_table_2d: bad query / output");
    if (zero_rows) HIP_TRY(hipMemsetAsync(zero_rows, 0, (size_t)n_depth * sizeof(int32_t), ctx->stream));
    {
        LaunchScope ls(ctx, "k_sigma_table_2d");
        hipLaunchKernelGGL(k_sigma_table_2d, grid2(n_nu, n_depth), dim3(kBlock), 0, ctx->stream, n_x, x_axis, n_y, y_axis,
                           (const int*)cell_simplices, transform, simplex_values, n_depth, n_nu, lambdas, second, scale_kind, temperature,
                           sigma, ld, (int*)zero_rows);
    }
    return check_launch("k_sigma_table_2d");
}

int sdx_alpha_bf_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int n_species, const int32_t* offs,
                     const int32_t* ions, const double* cutoff, const double* level_density, double* out, int64_t ld)
{
    REQUIRE(ctx && nus && n_species >= 0, "alpha_bf: bad arguments");
    ContinuumArgs a{};
    if (n_species > 0) {
        REQUIRE(offs && ions && cutoff && level_density, "alpha_bf: null pointer");
        int32_t n_levels = 0;  // offsets live on the device; the last one is the level count
        HIP_TRY(hipMemcpyAsync(&n_levels, offs + n_species, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        double* coef = nullptr;
        if (n_levels > 0) {
            int rc = launch_bf_coef(ctx, n_depth, n_species, n_levels, offs, ions, cutoff, level_density, &coef);
            if (rc) return rc;
        }
        a.bf_n_species = n_species;
        a.bf_species_offsets = (const int*)offs;
        a.bf_species_ion_number = (const int*)ions;
        a.bf_cutoff = cutoff;
        a.bf_coef = coef;
    }
    return launch_source(ctx, "k_alpha_bf", kSrcBf, n_depth, n_nu, nus, a, out, ld);
}

int sdx_alpha_ff_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, const double* temps, int n_species,
                     const int32_t* ions, const double* number_density, double* out, int64_t ld)
{
    REQUIRE(ctx && nus && temps && n_species >= 0 && (n_species == 0 || (ions && number_density)), "alpha_ff: bad arguments");
    ContinuumArgs a{};
    a.ff_n_species = n_species;
    a.ff_species_ion_number = (const int*)ions;
    a.ff_number_density = number_density;
    a.temperature = temps;
    return launch_source(ctx, "k_alpha_ff", kSrcFf, n_depth, n_nu, nus, a, out, ld);
}

int sdx_alpha_rayleigh_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, double* nus, const double* n_h, const double* n_he,
                           const double* n_h2, double* out, int64_t ld)
{
    REQUIRE(ctx && nus, "alpha_rayleigh: bad arguments");
    if (n_nu == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_rayleigh_clip");
        hipLaunchKernelGGL(k_rayleigh_clip, dim3(blocks1(n_nu)), dim3(kBlock), 0, ctx->stream, n_nu, nus);
    }
    int rc = check_launch("k_rayleigh_clip");
    if (rc) return rc;
    ContinuumArgs a{};
    a.ray_n_h = n_h;
    a.ray_n_he = n_he;
    a.ray_n_h2 = n_h2;
    return launch_source(ctx, "k_alpha_rayleigh", kSrcRayleigh, n_depth, n_nu, nus, a, out, ld);
}

int sdx_alpha_electron_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* ne, double* out, int64_t ld)
{
    REQUIRE(ctx && ne, "alpha_electron: bad arguments");
    ContinuumArgs a{};
    a.electron_density = ne;
    return launch_source(ctx, "k_alpha_electron", kSrcElectron, n_depth, n_nu, nullptr, a, out, ld);
}

int sdx_accumulate_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, double* total, int64_t tld, const double* src, int64_t sld)
{
    REQUIRE(ctx && n_depth > 0 && n_nu >= 0 && (n_nu == 0 || (total && src && tld >= n_nu && sld >= n_nu)),
            "accumulate: bad arguments");
    if (n_nu == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_accumulate");
        hipLaunchKernelGGL(k_accumulate, grid2(n_nu, n_depth), dim3(kBlock), 0, ctx->stream, n_depth, n_nu, total, tld, src, sld);
    }
    return check_launch("k_accumulate");
}

// total = continuum (+ line, where there is one) for the grid's columns
static int launch_total(sdx_ctx* ctx, const Grid& g, const sdx_continuum* cont, const double* line, int64_t line_ld, double* total, int64_t total_ld)
{
    ContinuumArgs a = to_args(cont, nullptr);
    a.bf_level_density = cont->bf_level_density;
    size_t shmem = 8;
    if (a.bf_n_species > 0) {
        REQUIRE(cont->bf_n_levels > 0 && cont->bf_n_levels <= 4096, "total_alphas: bf_n_levels must be set (1..4096)");
        shmem = (size_t)cont->bf_n_levels * sizeof(double);
    }
    {
        LaunchScope ls(ctx, "k_total_alphas");
        hipLaunchKernelGGL(k_total_alphas, grid2(g.nu_count, g.n_depth), dim3(kBlock), shmem, ctx->stream, g.n_depth, g.nu_begin, g.nu_count,
                           g.nus, a, line, line_ld, 1, (double*)nullptr, (int64_t)0, total, total_ld);
    }
    return check_launch("k_total_alphas");
}

int sdx_total_alphas_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                         const sdx_continuum* cont, const double* alpha_line, int64_t line_ld, double* total, int64_t total_ld)
{
    REQUIRE(ctx && cont && nus && n_depth > 0, "total_alphas: bad arguments");
    REQUIRE(nu_begin >= 0 && nu_count >= 0 && nu_begin + nu_count <= n_nu, "total_alphas: shard outside the grid");
    REQUIRE(nu_count == 0 || (total && total_ld >= nu_count && (!alpha_line || line_ld >= nu_count)), "total_alphas: bad buffers");
    if (int rc = check_file_planes(cont, n_nu)) return rc;
    if (nu_count == 0) return SDX_OK;
    return launch_total(ctx, Grid{n_depth, n_nu, nus, nu_begin, nu_count}, cont, alpha_line, line_ld, total, total_ld);
}

// ================================================================================================ formal solution
int sdx_blackbody_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, const double* temps, double* out, int64_t ld)
{
    REQUIRE(ctx && n_depth > 0 && n_nu >= 0 && (n_nu == 0 || (nus && temps && out && ld >= n_nu)), "blackbody: bad arguments");
    if (n_nu == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_blackbody");
        hipLaunchKernelGGL(k_blackbody, grid2(n_nu, n_depth), dim3(kBlock), 0, ctx->stream, n_depth, n_nu, nus, temps, out, ld);
    }
    return check_launch("k_blackbody");
}

int sdx_calc_weights_dev(sdx_ctx* ctx, int64_t n, const double* tau, double* w0, double* w1, double* w2)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (tau && w0 && w1 && w2)), "calc_weights: bad arguments");
    if (n == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_weights");
        hipLaunchKernelGGL(k_weights, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, tau, w0, w1, w2);
    }
    return check_launch("k_weights");
}

// what a formal solution of the grid's columns reads and writes, beyond the grid and the rays
struct RtPlanes {
    const double* alphas;  // total opacity [n_depth][ald], or null with a fused total
    int64_t ald;
    double* F;
    int64_t fld;
    double* I_nus;
    int accumulate, inward;
    const FusedTotal* fused;
    double* Fc;  // the continuum flux beside a fused total
    int64_t fcld;
};
static int raytrace_impl(sdx_ctx* ctx, const Grid& g, const Rays& rays, const RtPlanes& io);

// the tail of spherical geometry: F_nu *= (r[-1] / reference_r)^2 (radiation_field_solvers/base.py:340-344); the continuum flux,
// where there is one, in the same profiled launch scope
static int scale_flux(sdx_ctx* ctx, int n_depth, int64_t n_nu, double* F, int64_t ld, double factor, double* Fc = nullptr, int64_t fcld = 0)
{
    {
        LaunchScope ls(ctx, "k_scale");
        hipLaunchKernelGGL(k_scale, grid2(n_nu, n_depth), dim3(kBlock), 0, ctx->stream, n_depth, n_nu, F, ld, factor);
        if (Fc) hipLaunchKernelGGL(k_scale, grid2(n_nu, n_depth), dim3(kBlock), 0, ctx->stream, n_depth, n_nu, Fc, fcld, factor);
    }
    return check_launch("k_scale");
}

int sdx_raytrace_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                     const double* ray_dist, const double* wts, const double* alphas, int64_t ald, double* F, int64_t fld,
                     double* I_nus, int accumulate)
{
    return raytrace_impl(ctx, Grid{n_depth, n_nu, nus, 0, n_nu}, Rays{n_theta, temps, ray_dist, wts}, RtPlanes{alphas, ald, F, fld, I_nus, accumulate, 0, nullptr, nullptr, 0});
}

int sdx_raytrace_source_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                            const double* ray_dist, const double* wts, const double* alphas, int64_t ald, const double* source,
                            int64_t source_ld, double* F, int64_t fld, double* I_nus, int accumulate, int inward,
                            double photospheric_correction)
{
    REQUIRE(ctx && (n_nu == 0 || !source || source_ld >= n_nu), "raytrace: bad source plane");
    FusedTotal ft{};
    ft.source = source;
    ft.sld = source_ld;
    int rc = raytrace_impl(ctx, Grid{n_depth, n_nu, nus, 0, n_nu}, Rays{n_theta, temps, ray_dist, wts},
                           RtPlanes{alphas, ald, F, fld, I_nus, accumulate, inward ? 1 : 0, source ? &ft : nullptr, nullptr, 0});
    if (rc || !inward || !F || n_nu == 0) return rc;
    return scale_flux(ctx, n_depth, n_nu, F, fld, photospheric_correction);
}

int sdx_raytrace_spherical_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                               const double* ray_dist, const double* wts, const double* alphas, int64_t ald, double* F,
                               int64_t fld, double* I_nus, int accumulate, double photospheric_correction)
{
    int rc = raytrace_impl(ctx, Grid{n_depth, n_nu, nus, 0, n_nu}, Rays{n_theta, temps, ray_dist, wts}, RtPlanes{alphas, ald, F, fld, I_nus, accumulate, 1, nullptr, nullptr, 0});
    if (rc || !F || n_nu == 0) return rc;
    return scale_flux(ctx, n_depth, n_nu, F, fld, photospheric_correction);
}

// (the columns [nu_begin, nu_begin + nu_count) of the grid; which kernel runs is decided from the whole grid, g.n_nu)
static int raytrace_impl(sdx_ctx* ctx, const Grid& g, const Rays& rays, const RtPlanes& io)
{
    const int n_depth = g.n_depth, n_theta = rays.n_theta, accumulate = io.accumulate, inward = io.inward;
    const int64_t n_nu = g.nu_count, nu_global = g.n_nu, ald = io.ald, fld = io.fld, fcld = io.fcld;
    const double *const nus = g.nus + g.nu_begin, *const temps = rays.temps, *const ray_dist = rays.ray_dist, *const wts = rays.wts, *const alphas = io.alphas;
    double *const F = io.F, *const I_nus = io.I_nus, *const Fc = io.Fc;
    FusedTotal ft{};
    if (io.fused) ft = *io.fused;
    REQUIRE(ctx && n_depth >= 2 && n_nu >= 0 && n_theta > 0, "raytrace: need n_depth >= 2, n_theta > 0");
    if (n_nu == 0) return SDX_OK;
    REQUIRE(nus && temps && ray_dist && wts && ((alphas && ald >= n_nu) || ft.cont), "raytrace: null pointer");
    REQUIRE(!ft.cont || n_theta <= 64, "raytrace: the fused total needs all angles in one launch");
    REQUIRE(!ft.source || n_theta <= 64, "raytrace: a caller-provided source plane needs all angles in one launch");
    REQUIRE((F && fld >= n_nu) || I_nus, "raytrace: no output requested");
    // the continuum flux (k_raytrace_cont, or a second k_raytrace_seg) is traced beside a fused total, whose continuum column it reads
    REQUIRE(!Fc || ft.cont, "raytrace: the continuum flux needs a fused total");
    REQUIRE(!Fc || (F && fcld >= n_nu && !accumulate), "raytrace: the continuum flux needs F_nu and continuum_ld >= the columns");
    REQUIRE(!Fc || !ctx->mixed_precision, "raytrace: no continuum flux with mixed_precision = 1 (the fp32 formal solution has no continuum chain)");
    constexpr int kMaxChunk = 64;
    for (int th0 = 0; th0 < n_theta; th0 += kMaxChunk) {
        const int nth = std::min(kMaxChunk, n_theta - th0);
        const double* rd = ray_dist + th0;
        const double* w = wts + th0;
        double* inus = I_nus ? I_nus + th0 : nullptr;
        const int acc = (accumulate || th0 > 0) ? 1 : 0;
        // One lane per (frequency, angle): G = nth lanes per frequency.  (Two and four angles per lane were measured on MI355X at 7.6e3
        // and 1.2e5 frequencies and lost — fewer waves in flight; profiles/EXPERIMENTS.md.)
        // The second argument of a LaunchScope (what sdx_profile_variant returns) is a profile LABEL, not a symbol: the name under which
        // the kernel stands in every recorded benchmark and profile and in the GPU tests.  "k_raytrace<1>", "k_raytrace_cont<1>" and
        // "k_contribution<1>" are the plain kernels k_raytrace, k_raytrace_cont and k_contribution; the labels stay byte for byte.
        const int G = nth;
        const int gpw = rt_fit_gpw<RtColumns>(G, n_depth);  // 0: the columns do not fit LDS
        const unsigned blocks_basic = (unsigned)((n_nu + (int64_t)(64 / G) * (kBlock / 64) - 1) / ((int64_t)(64 / G) * (kBlock / 64)));
        // plane-parallel, one angle per lane, nothing to add to, a small grid: the gaps of a ray split over the 8 waves of a
        // workgroup (k_raytrace_seg)
        const RtSegments seg = seg_layout(n_depth, nth);
        const int seg_gpw = seg.gpw();
        // the launch geometry of the XCD-aware order, handed to the kernel: workgroups, workgroups per XCD, whole rounds of eight
        const unsigned seg_wg = (unsigned)((n_nu + seg_gpw - 1) / seg_gpw), seg_per_xcd = (seg_wg + 7) / 8, seg_blocks = seg_per_xcd * 8;
        if (use_segmented_raytrace(ctx, n_depth, nu_global, n_theta, !inward && !acc)) {
            // the shape of the fused synthesis step — a fused total of 0, 2 or 3 line planes, the Planck source, flux only — has a kernel
            // of its own (k_raytrace_seg_step: the same bits); "segmented_raytrace" = 1 keeps the general kernel
            const int step_planes = ft.planes ? ft.n_planes : 0;
            const bool step_shape = segmented_mode(ctx) != 1 && ft.cont && !ft.source && ft.n_extra == 0 && !ft.line_out && !inus && F &&
                                    (step_planes == 0 || step_planes == 2 || step_planes == 3) && fld <= (int64_t)UINT32_MAX;
            SegStepGeom geo{};
            geo.gpw = seg_gpw, geo.g_recip = lane_recip(nth), geo.per = 64 / nth, geo.L = seg.segment();
            geo.rstride = seg.rstride(), geo.sp_off = seg.pairs_from_table(), geo.gpw_magic = small_div_magic(seg_gpw);
            geo.n_wg = seg_wg, geo.per_xcd = seg_per_xcd;
            geo.fx_pairs = seg_step_flux_pairs(seg);
            auto launch_step = [&](int planes_n, const double* planes, double* total_out, double* flux, int64_t flux_ld) {
                geo.fld = (unsigned)flux_ld;  // (the caller has asked that it fits)
#define SDX_STEP_LAUNCH(NP, KEEP)                                                                                                              \
    hipLaunchKernelGGL((k_raytrace_seg_step<8, 7, NP, KEEP>), dim3(seg_blocks), dim3(512), seg.bytes(), ctx->stream, n_depth, n_nu, nth, \
                       n_theta, nus, temps, rd, w, ft.cont, ft.cld, planes, ft.pld, total_out, ft.out_ld, flux, geo)
                if (planes_n == 0) {
                    if (total_out) SDX_STEP_LAUNCH(0, true);
                    else SDX_STEP_LAUNCH(0, false);
                } else if (planes_n == 2) {
                    if (total_out) SDX_STEP_LAUNCH(2, true);
                    else SDX_STEP_LAUNCH(2, false);
                } else {
                    if (total_out) SDX_STEP_LAUNCH(3, true);
                    else SDX_STEP_LAUNCH(3, false);
                }
#undef SDX_STEP_LAUNCH
            };
            // the general kernel: the total as the caller asked for it, or the continuum plane alone
            auto launch_seg = [&](const double* a, int64_t a_ld, double* flux, int64_t flux_ld, double* intensity, const FusedTotal& fused_total) {
                hipLaunchKernelGGL((k_raytrace_seg<8, 7>), dim3(seg_blocks), dim3(512), seg.bytes(), ctx->stream, n_depth, n_nu, nth, n_theta, nus, temps, rd, w,
                                   a, a_ld, flux, flux_ld, intensity, seg_gpw, lane_recip(nth), seg_wg, seg_per_xcd, fused_total);
            };
            if (step_shape) {
                LaunchScope ls(ctx, "k_raytrace", "k_raytrace_seg_step<8,7>");
                launch_step(step_planes, ft.planes, ft.total_out, F, fld);
            } else {
                LaunchScope ls(ctx, "k_raytrace", "k_raytrace_seg<8,7>");
                launch_seg(alphas, ald, F, fld, inus, ft);
            }
            int rc = check_launch("k_raytrace_seg");
            if (rc) return rc;
            if (Fc) {
                // the continuum on the small grids: k_raytrace_seg once more, on the continuum plane alone (the zero-line run's own
                // launch, so its bits).  A fused k_raytrace_seg_cont (both chains over one staging, four waves per SIMD) was built and
                // measured at S-c2: 81 us against 36 for this kernel, 45 us extra per step against 44 for a whole zero-line synthesis
                // (DESIGN.md).  Removed.
                FusedTotal fc{};
                fc.cont = ft.cont, fc.cld = ft.cld, fc.source = ft.source, fc.sld = ft.sld;
                if (segmented_mode(ctx) != 1 && !ft.source && fcld <= (int64_t)UINT32_MAX) {  // (this launch has the step kernel's shape whatever the first one had)
                    LaunchScope ls(ctx, "k_raytrace", "k_raytrace_seg_step<8,7> (continuum)");
                    launch_step(0, nullptr, nullptr, Fc, fcld);
                } else {
                    LaunchScope ls(ctx, "k_raytrace", "k_raytrace_seg<8,7> (continuum)");
                    launch_seg(nullptr, 0, Fc, fcld, nullptr, fc);
                }
                if ((rc = check_launch("k_raytrace_seg"))) return rc;
            }
            continue;
        }
        // the tolerance path (mixed_precision = 1): plane-parallel, all angles in one launch, flux only -> the fp32 recurrence
        if (ctx->mixed_precision && !inward && !acc && !inus && F && n_theta <= 64) {
            const int g32 = 64 / G;
            const RtF32Columns lay32(nth, G, n_depth, g32);
            if (n_depth <= kRtMaxDepth && lay32.bytes() <= kLdsBytes) {
                {
                    LaunchScope ls(ctx, "k_raytrace", "k_raytrace_f32");
                    hipLaunchKernelGGL(k_raytrace_f32, dim3(rt_blocks(n_nu, g32)), dim3(kRtBlock), lay32.bytes(), ctx->stream, n_depth, n_nu, nth, n_theta, G, nus, temps, rd,
                                       w, alphas, ald, F, fld, g32, ft);
                }
                int rc = check_launch("k_raytrace_f32");
                if (rc) return rc;
                continue;
            }
        }
        if (Fc) {
            REQUIRE(gpw > 0, "raytrace: no continuum flux for models this deep (the columns do not fit LDS)");
            const int gpwc = rt_fit_gpw<RtContColumns>(G, n_depth);
            REQUIRE(gpwc > 0, "raytrace: no continuum flux for models this deep (the columns do not fit LDS)");
            {
                LaunchScope ls(ctx, "k_raytrace", "k_raytrace_cont<1>");
                hipLaunchKernelGGL(k_raytrace_cont, dim3(rt_blocks(n_nu, gpwc)), dim3(kRtBlock), RtContColumns(G, n_depth, gpwc).bytes(), ctx->stream, n_depth, n_nu,
                                   nth, n_theta, G, nus, temps, rd, w, F, fld, Fc, fcld, inus, inward, gpwc, ft);
            }
            int rc = check_launch("k_raytrace_cont");
            if (rc) return rc;
            continue;
        }
        {
            LaunchScope ls(ctx, "k_raytrace", gpw > 0 ? "k_raytrace<1>" : "k_raytrace_basic");
            if (gpw > 0) {
                hipLaunchKernelGGL(k_raytrace, dim3(rt_blocks(n_nu, gpw)), dim3(kRtBlock), RtColumns(G, n_depth, gpw).bytes(), ctx->stream, n_depth, n_nu, nth, n_theta,
                                   G, nus, temps, rd, w, alphas, ald, F, fld, inus, acc, inward, gpw, ft);
            } else {  // very deep models: the column does not fit LDS, recompute per lane instead
                REQUIRE(!ft.cont && !ft.source, "raytrace: fused total / caller's source plane not available for models this deep");
                REQUIRE(!inward, "raytrace: spherical geometry needs (3*n_depth*64/n_theta + 2*n_depth*n_theta) doubles of LDS per wave; model too deep");
                hipLaunchKernelGGL(k_raytrace_basic, dim3(blocks_basic), dim3(kBlock), 0, ctx->stream, n_depth, n_nu, nth, n_theta, G, nus, temps, rd, w, alphas, ald, F,
                                   fld, inus, acc);
            }
        }
        int rc = check_launch("k_raytrace");
        if (rc) return rc;
    }
    return SDX_OK;
}

// ---- the products of the formal solution over the grid's columns ------------------------------------------------------------------
// The contribution function, the emergent intensities, the response functions, the mean intensity, the scattering source and the two
// scattering adjoints solve one problem (Columns).  Every device entry passes the gate, then checks its own scalars (tol, max_iter),
// then its pointers and outputs: everything before anything is enqueued, and the gate and the scalars also for an empty grid, so that
// a caller can ask at set-up time whether this context and shape are served (the engine does).  Every host-buffer twin makes the same
// refusals in the same order on its host pointers, before any copy, and runs the one skeleton (columns_host) around its device entry.
extern "C++" {
namespace {
struct Plane {  // [n_depth][ld]
    const double* p;
    int64_t ld;
};
struct Columns {  // the grid, the rays, the total opacity and the source (or thermal) plane — null: the Planck function of rays.temps
    Grid g;
    Rays rays;
    Plane alphas, source;
};
Columns columns(int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist, const double* wts,
                Plane alphas, Plane source)
{
    return Columns{Grid{n_depth, n_nu, nus, 0, n_nu}, Rays{n_theta, temps, ray_dist, wts}, alphas, source};
}

// What the gate says under each entry's name: to a context with mixed_precision = 1, and to a model whose columns do not fit LDS
struct ColumnEntry {
    const char *name, *mixed, *deep;
};
constexpr const char* kResponseMixed = "no response functions with mixed_precision = 1 (they differentiate the fp64 formal solution)";
constexpr const char* kResponseDeep = "no response functions for models this deep (the columns and the stashed intensities do not fit LDS)";
constexpr const char* kLambdaMixed = "not with mixed_precision = 1 (the mean intensity is that of the fp64 formal solution)";
constexpr const char* kLambdaDeep = "models this deep are not served (the columns of one frequency do not fit LDS)";
constexpr const char* kAdjointDeep = "models this deep are not served (the columns and stashed values of one frequency do not fit LDS)";
constexpr ColumnEntry kContribution{"contribution", "no contribution function with mixed_precision = 1 (it decomposes the fp64 formal solution)",
                                    "no contribution function for models this deep (the columns do not fit LDS)"},
    kEmergentIntensity{"emergent_intensity", "no emergent intensities with mixed_precision = 1 (they are the fp64 formal solution's last row)",
                       "no emergent intensities for models this deep (the columns do not fit LDS)"},
    kResponse{"response", kResponseMixed, kResponseDeep}, kResponseAngles{"response_angles", kResponseMixed, kResponseDeep},
    kMeanIntensity{"mean_intensity", kLambdaMixed, kLambdaDeep}, kScatterSource{"scatter_source", kLambdaMixed, kLambdaDeep},
    kMeanIntensityAdjoint{"mean_intensity_adjoint", kLambdaMixed, kAdjointDeep}, kScatterResponse{"scatter_response", kLambdaMixed, kAdjointDeep},
    kScatterSourceNg{"scatter_source_ng", kLambdaMixed,
                     "models this deep are not served with acceleration (the history columns of one frequency do not fit LDS beside the "
                     "iteration's; sdx_scatter_source_dev, the plain iteration, serves deeper models)"};

int refuse(const ColumnEntry& e, const std::string& why) { return fail(SDX_ERR_ARG, std::string(e.name) + ": " + why); }

// The gate: the refusals all products share -> the frequencies per wave of the launch (Layout: the kernel's LDS layout), or the error code
static_assert(SDX_ERR_ARG < 0, "column_gate returns a count or an error code");
template <class Layout>
int column_gate(const sdx_ctx* ctx, const ColumnEntry& e, int n_depth, int64_t n_nu, int n_theta)
{
    if (!(ctx && n_depth >= 2 && n_nu >= 0 && n_theta > 0)) return refuse(e, "need n_depth >= 2, n_theta > 0");
    if (ctx->mixed_precision) return refuse(e, e.mixed);
    if (n_theta > 64) return refuse(e, "more than 64 angles are not supported (all angles are traced in one launch)");
    const int gpw = rt_fit_gpw<Layout>(n_theta, n_depth);
    return gpw > 0 ? gpw : refuse(e, e.deep);
}
// the scalars of the two iterations
int iteration_check(const ColumnEntry& e, double tol, int max_iter)
{
    return tol >= 0.0 && max_iter >= 1 ? SDX_OK : refuse(e, "need tol >= 0 (not NaN) and max_iter >= 1");
}
// the scalars of the accelerated iterations
int acceleration_check(const ColumnEntry& e, int ng_start, int ng_period)
{
    return ng_start >= 4 && ng_period >= 1 ? SDX_OK : refuse(e, "need ng_start >= 4 (an extrapolation reads four iterates) and ng_period >= 1");
}
// a source plane (`kind`: "source", or "thermal") that is wide enough, or temperatures
int source_or_temps(const ColumnEntry& e, const std::string& kind, const Columns& c)
{
    if (c.source.p ? c.source.ld >= c.g.n_nu : c.rays.temps != nullptr) return SDX_OK;
    return refuse(e, "bad " + kind + " plane (" + kind + "_ld < n_nu), or neither a " + kind + " plane nor temperatures");
}
// an optional plane: absent, or its leading dimension at least n_nu
bool fits(const double* p, int64_t ld, int64_t n_nu) { return !p || ld >= n_nu; }
// the inputs every product needs: the grid, the ray table, the opacity plane and — where the entry reads them — weights and temperatures
bool columns_given(const Columns& c, bool wts = true, bool temps = false)
{
    return c.g.nus && c.rays.ray_dist && (c.rays.wts || !wts) && (c.rays.temps || !temps) && c.alphas.p && c.alphas.ld >= c.g.n_nu;
}

// The host-buffer twin of an entry, after its refusals.  The five rows every twin uploads — n_wts doubles of weights: [n_theta], a
// cotangent plane, or none (h.rays.wts null) — then rows(plan, plane, d): the entry's own rows, `plane` the bytes of [n_depth][n_nu], the
// source plane's slot d.source.p; then stage -> launch(d) -> collect -> finish, d the problem on device addresses, every ld = n_nu.
template <class Rows, class Launch>
int columns_host(sdx_ctx* ctx, const Columns& h, size_t n_wts, Rows rows, Launch launch)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const int n_depth = h.g.n_depth, n_theta = h.rays.n_theta;
    const int64_t n_nu = h.g.n_nu;
    const double *const nus = h.g.nus, *const temps = h.rays.temps, *const ray_dist = h.rays.ray_dist, *const wts = h.rays.wts;
    const size_t f8 = sizeof(double), plane = (size_t)n_depth * n_nu * f8;
    Columns d{h.g, h.rays, {nullptr, n_nu}, {nullptr, n_nu}};
    HostPlan plan;
    plan.in(nus, (size_t)n_nu * f8, &d.g.nus);
    plan.in(temps, (size_t)n_depth * f8, &d.rays.temps);
    plan.in(ray_dist, (size_t)(n_depth - 1) * n_theta * f8, &d.rays.ray_dist);
    plan.in(wts, n_wts * f8, &d.rays.wts);
    plan.in(h.alphas.p, plane, &d.alphas.p);
    rows(plan, plane, d);
    HostIo io{ctx};
    int rc;
    if ((rc = io.stage(plan))) return rc;
    if ((rc = launch(d))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}
}  // namespace
}  // extern "C++"

int sdx_raytrace_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                     const double* ray_dist, const double* wts, const double* alphas, double* F, double* I_nus)
{
    REQUIRE(ctx && n_depth >= 2 && n_nu >= 0 && n_theta > 0, "raytrace: need n_depth >= 2, n_theta > 0");
    REQUIRE(n_nu == 0 || (nus && temps && ray_dist && wts && alphas && F), "raytrace: null pointer");
    if (n_nu == 0) return SDX_OK;
    double *d_f, *d_i;
    const auto rows = [&](HostPlan& plan, size_t plane, Columns&) {
        plan.inout(F, plane, &d_f);  // F_nu is accumulated into (base.py:336)
        plan.out(I_nus, plane * n_theta, &d_i);
    };
    return columns_host(ctx, columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, wts, {alphas, n_nu}, {}), n_theta, rows, [&](const Columns& d) {
        return sdx_raytrace_dev(ctx, n_depth, n_nu, n_theta, d.g.nus, d.rays.temps, d.rays.ray_dist, d.rays.wts, d.alphas.p, n_nu, d_f, n_nu, d_i, 1);
    });
}

// ---- flux contribution function and formation depth (k_contribution, k_formation_mean) ------------------------------------
int sdx_contribution_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                         const double* ray_dist, const double* wts, const double* alphas, int64_t ald, const double* source,
                         int64_t source_ld, double* C, int64_t cld)
{
    const int G = n_theta, gpw = column_gate<RtColumns>(ctx, kContribution, n_depth, n_nu, n_theta);  // (k_raytrace's budget)
    if (gpw < 0) return gpw;
    if (n_nu == 0) return SDX_OK;
    const Columns c = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, wts, {alphas, ald}, {source, source_ld});
    REQUIRE(columns_given(c) && C && cld >= n_nu, "contribution: null pointer or leading dimension below n_nu");
    if (int rc = source_or_temps(kContribution, "source", c)) return rc;
    {
        LaunchScope ls(ctx, "k_contribution", "k_contribution<1>");
        hipLaunchKernelGGL(k_contribution, dim3(rt_blocks(n_nu, gpw)), dim3(kRtBlock), RtColumns(G, n_depth, gpw).bytes(), ctx->stream, n_depth, n_nu, n_theta, n_theta, G,
                           nus, temps, ray_dist, wts, alphas, ald, source, source_ld, C, cld, gpw);
    }
    return check_launch("k_contribution");
}

int sdx_formation_mean_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* C, int64_t cld, const double* x, double* out)
{
    REQUIRE(ctx && n_depth >= 2 && n_nu >= 0, "formation_mean: need n_depth >= 2");
    if (n_nu == 0) return SDX_OK;
    REQUIRE(C && cld >= n_nu && x && out, "formation_mean: null pointer or C_ld below n_nu");
    {
        LaunchScope ls(ctx, "k_formation_mean");
        hipLaunchKernelGGL(k_formation_mean, dim3(blocks1(n_nu)), dim3(kBlock), 0, ctx->stream, n_depth, n_nu, C, cld, x, out);
    }
    return check_launch("k_formation_mean");
}

int sdx_contribution_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                         const double* ray_dist, const double* wts, const double* alphas, const double* source, double* C)
{
    if (const int no = column_gate<RtColumns>(ctx, kContribution, n_depth, n_nu, n_theta); no < 0) return no;
    if (n_nu == 0) return SDX_OK;
    const Columns h = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, wts, {alphas, n_nu}, {source, n_nu});
    REQUIRE(columns_given(h, true, true) && C, "contribution: null pointer");
    double* d_c;
    const auto rows = [&](HostPlan& plan, size_t plane, Columns& d) {
        plan.in(source, plane, &d.source.p);
        plan.out(C, plane, &d_c);
    };
    return columns_host(ctx, h, n_theta, rows, [&](const Columns& d) {
        return sdx_contribution_dev(ctx, n_depth, n_nu, n_theta, d.g.nus, d.rays.temps, d.rays.ray_dist, d.rays.wts, d.alphas.p, n_nu, d.source.p, n_nu, d_c, n_nu);
    });
}

// ---- emergent intensity of every ray, the surface row alone (k_emergent_intensity) -----------------------------------------
int sdx_emergent_intensity_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                               const double* ray_dist, const double* alphas, int64_t ald, const double* source, int64_t source_ld, int inward,
                               double* I_out, int64_t I_ld)
{
    const int G = n_theta, gpw = column_gate<RtColumns>(ctx, kEmergentIntensity, n_depth, n_nu, n_theta);  // (k_raytrace's budget)
    if (gpw < 0) return gpw;
    for (const double* in : {nus, temps, ray_dist, alphas, source})
        REQUIRE(!I_out || I_out != in, "emergent_intensity: not in place (I_out must not be one of the inputs)");
    if (n_nu == 0) return SDX_OK;
    const Columns c = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, nullptr, {alphas, ald}, {source, source_ld});
    REQUIRE(columns_given(c, false) && I_out && I_ld >= n_nu, "emergent_intensity: null pointer or leading dimension below n_nu");
    if (int rc = source_or_temps(kEmergentIntensity, "source", c)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    {
        LaunchScope ls(ctx, "k_emergent_intensity");
        hipLaunchKernelGGL(k_emergent_intensity, dim3(rt_blocks(n_nu, gpw)), dim3(kRtBlock), RtColumns(G, n_depth, gpw).bytes(), ctx->stream, n_depth, n_nu, n_theta,
                           n_theta, G, nus, temps, ray_dist, alphas, ald, source, source_ld, inward ? 1 : 0, I_out, I_ld, gpw);
    }
    return check_launch("k_emergent_intensity");
}

int sdx_emergent_intensity_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                               const double* ray_dist, const double* alphas, const double* source, int inward, double* I_out)
{
    if (const int no = column_gate<RtColumns>(ctx, kEmergentIntensity, n_depth, n_nu, n_theta); no < 0) return no;
    if (n_nu == 0) return SDX_OK;
    const Columns h = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, nullptr, {alphas, n_nu}, {source, n_nu});
    REQUIRE(columns_given(h, false, true) && I_out, "emergent_intensity: null pointer");
    double* d_i;
    const auto rows = [&](HostPlan& plan, size_t plane, Columns& d) {
        plan.in(source, plane, &d.source.p);
        plan.out(I_out, (size_t)n_theta * n_nu * sizeof(double), &d_i);
    };
    return columns_host(ctx, h, 0, rows, [&](const Columns& d) {
        return sdx_emergent_intensity_dev(ctx, n_depth, n_nu, n_theta, d.g.nus, d.rays.temps, d.rays.ray_dist, d.alphas.p, n_nu, d.source.p, n_nu, inward, d_i, n_nu);
    });
}

// ---- response functions (k_response, k_response_project) -------------------------------------------------------------------
// c.rays.wts: the flux weights [n_theta], or with `angles` the cotangent plane [n_theta][wld] (k_response_angles)
static int response_launch(sdx_ctx* ctx, bool angles, const Columns& c, int64_t wld, double* R_alpha, int64_t R_alpha_ld, double* R_source,
                           int64_t R_source_ld)
{
    const ColumnEntry& e = angles ? kResponseAngles : kResponse;
    const char* const stage = angles ? "k_response_angles" : "k_response";
    const auto msg = [&](const char* text) { return std::string(e.name) + text; };
    const int n_depth = c.g.n_depth, n_theta = c.rays.n_theta;
    const int64_t n_nu = c.g.n_nu, ald = c.alphas.ld, source_ld = c.source.ld;
    const double *const nus = c.g.nus, *const temps = c.rays.temps, *const ray_dist = c.rays.ray_dist, *const wts = c.rays.wts, *const alphas = c.alphas.p,
                 *const source = c.source.p;
    const int G = n_theta, gpw = column_gate<RtResponse>(ctx, e, n_depth, n_nu, n_theta);
    if (gpw < 0) return gpw;
    if (n_nu == 0) return SDX_OK;
    REQUIRE(R_alpha || R_source, msg(": no output requested"));
    REQUIRE(columns_given(c), msg(": null pointer or alpha_ld below n_nu"));
    REQUIRE(!angles || wld >= n_nu, msg(": cot_ld below n_nu"));
    REQUIRE(fits(R_alpha, R_alpha_ld, n_nu) && fits(R_source, R_source_ld, n_nu), msg(": leading dimension of an output below n_nu"));
    if (int rc = source_or_temps(e, "source", c)) return rc;
    for (const double* o : {(const double*)R_alpha, (const double*)R_source})
        REQUIRE(!angles || !o || o != wts, msg(": not in place (an output must not be the cotangent)"));
    {
        LaunchScope ls(ctx, stage);
        if (angles)
            hipLaunchKernelGGL(k_response_angles, dim3(response_blocks(n_nu, gpw)), dim3(kRespBlock), RtResponse(G, n_depth, gpw).bytes(), ctx->stream, n_depth,
                               n_nu, n_theta, n_theta, G, nus, temps, ray_dist, wts, wld, alphas, ald, source, source_ld, R_alpha, R_alpha_ld, R_source, R_source_ld,
                               gpw);
        else
            hipLaunchKernelGGL(k_response, dim3(response_blocks(n_nu, gpw)), dim3(kRespBlock), RtResponse(G, n_depth, gpw).bytes(), ctx->stream, n_depth, n_nu,
                               n_theta, n_theta, G, nus, temps, ray_dist, wts, alphas, ald, source, source_ld, R_alpha, R_alpha_ld, R_source, R_source_ld, gpw);
    }
    return check_launch(stage);
}

int sdx_response_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                     const double* wts, const double* alphas, int64_t ald, const double* source, int64_t source_ld, double* R_alpha,
                     int64_t R_alpha_ld, double* R_source, int64_t R_source_ld)
{
    return response_launch(ctx, false, columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, wts, {alphas, ald}, {source, source_ld}), 0, R_alpha, R_alpha_ld,
                           R_source, R_source_ld);
}

int sdx_response_angles_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                            const double* cotangent, int64_t cot_ld, const double* alphas, int64_t ald, const double* source, int64_t source_ld,
                            double* R_alpha, int64_t R_alpha_ld, double* R_source, int64_t R_source_ld)
{
    return response_launch(ctx, true, columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, cotangent, {alphas, ald}, {source, source_ld}), cot_ld, R_alpha,
                           R_alpha_ld, R_source, R_source_ld);
}

int sdx_response_project_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* R_alpha, int64_t R_ld, const double* part, int64_t part_ld,
                             const double* total, int64_t total_ld, double* out)
{
    REQUIRE(ctx && n_depth >= 2 && n_nu >= 0, "response_project: need n_depth >= 2");
    if (n_nu == 0) return SDX_OK;
    REQUIRE(R_alpha && part && total && out && R_ld >= n_nu && part_ld >= n_nu && total_ld >= n_nu, "response_project: null pointer or leading dimension below n_nu");
    {
        LaunchScope ls(ctx, "k_response_project");
        hipLaunchKernelGGL(k_response_project, dim3(blocks1(n_nu)), dim3(kBlock), 0, ctx->stream, n_depth, n_nu, R_alpha, R_ld, part, part_ld, total, total_ld, out);
    }
    return check_launch("k_response_project");
}

// wts: [n_theta], or with `angles` the cotangent [n_theta][n_nu]
static int response_host(sdx_ctx* ctx, bool angles, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                         const double* ray_dist, const double* wts, const double* alphas, const double* source, double* R_alpha, double* R_source)
{
    REQUIRE(ctx && n_depth >= 2 && n_nu >= 0 && n_theta > 0, "response: need n_depth >= 2, n_theta > 0");  // (both twins say this, and what follows the gate, as "response")
    if (const int no = column_gate<RtResponse>(ctx, angles ? kResponseAngles : kResponse, n_depth, n_nu, n_theta); no < 0) return no;
    if (n_nu == 0) return SDX_OK;
    const Columns h = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, wts, {alphas, n_nu}, {source, n_nu});
    REQUIRE(columns_given(h, true, true), "response: null pointer");
    REQUIRE(R_alpha || R_source, "response: no output requested");
    double *d_ra, *d_rs;
    const auto rows = [&](HostPlan& plan, size_t plane, Columns& d) {
        plan.in(source, plane, &d.source.p);
        plan.out(R_alpha, plane, &d_ra);
        plan.out(R_source, plane, &d_rs);
    };
    return columns_host(ctx, h, angles ? (size_t)n_theta * n_nu : (size_t)n_theta, rows,
                        [&](const Columns& d) { return response_launch(ctx, angles, d, n_nu, d_ra, n_nu, d_rs, n_nu); });
}

int sdx_response_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                     const double* wts, const double* alphas, const double* source, double* R_alpha, double* R_source)
{
    return response_host(ctx, false, n_depth, n_nu, n_theta, nus, temps, ray_dist, wts, alphas, source, R_alpha, R_source);
}

int sdx_response_angles_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                            const double* cotangent, const double* alphas, const double* source, double* R_alpha, double* R_source)
{
    return response_host(ctx, true, n_depth, n_nu, n_theta, nus, temps, ray_dist, cotangent, alphas, source, R_alpha, R_source);
}

// ---- mean intensity and the scattering source function (k_lambda) ----------------------------------------------------------
int sdx_mean_intensity_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                           const double* mean_weights, const double* alphas, int64_t ald, const double* source, int64_t source_ld, double* J,
                           int64_t J_ld, double* lambda_diag, int64_t L_ld)
{
    const int gpw = column_gate<RtLambda>(ctx, kMeanIntensity, n_depth, n_nu, n_theta);
    if (gpw < 0) return gpw;
    if (n_nu == 0) return SDX_OK;
    const Columns c = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, {alphas, ald}, {source, source_ld});
    REQUIRE(J || lambda_diag, "mean_intensity: no output requested");
    REQUIRE(columns_given(c), "mean_intensity: null pointer or alpha_ld below n_nu");
    REQUIRE(fits(J, J_ld, n_nu) && fits(lambda_diag, L_ld, n_nu), "mean_intensity: leading dimension of an output below n_nu");
    if (int rc = source_or_temps(kMeanIntensity, "source", c)) return rc;
    const int waves = lambda_waves(n_theta, n_depth, gpw);
    {
        LaunchScope ls(ctx, "k_lambda", "k_lambda<false>");
        hipLaunchKernelGGL(k_lambda<false>, dim3(lambda_blocks(n_nu, gpw, waves)), dim3(64 * waves), waves * RtLambda(n_theta, n_depth, gpw).bytes(), ctx->stream,
                           n_depth, n_nu, n_theta, n_theta, n_theta, nus, temps, ray_dist, mean_weights, alphas, ald, source, source_ld, J, J_ld, lambda_diag, L_ld,
                           gpw, waves, LambdaIteration{});
    }
    return check_launch("k_lambda");
}

// The scattering source iteration, plain (ng null) or with Ng acceleration: one set of refusals, one launch
extern "C++" {
namespace {
struct NgOptions {
    int start, period;
    int* accelerations;
};
int scatter_source_device(sdx_ctx* ctx, const NgOptions* ng, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                          const double* ray_dist, const double* mean_weights, const double* alphas, int64_t ald, const double* alpha_scatter,
                          int64_t scatter_ld, const double* thermal, int64_t thermal_ld, double tol, int max_iter, double* S, int64_t S_ld, double* J,
                          int64_t J_ld, int* iterations, int* status, double* change)
{
    const ColumnEntry& e = ng ? kScatterSourceNg : kScatterSource;
    const int gpw = ng ? column_gate<RtLambdaNg>(ctx, e, n_depth, n_nu, n_theta) : column_gate<RtLambda>(ctx, e, n_depth, n_nu, n_theta);
    if (gpw < 0) return gpw;
    if (int rc = iteration_check(e, tol, max_iter)) return rc;
    if (n_nu == 0) return SDX_OK;
    const Columns c = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, {alphas, ald}, {thermal, thermal_ld});
    REQUIRE(columns_given(c) && alpha_scatter && S, "scatter_source: null pointer or alpha_ld below n_nu");
    REQUIRE((scatter_ld == 0 || scatter_ld >= n_nu) && S_ld >= n_nu && fits(J, J_ld, n_nu), "scatter_source: a leading dimension below n_nu (scatter_ld: 0 or >= n_nu)");
    if (int rc = source_or_temps(e, "thermal", c)) return rc;
    const LambdaIteration it{alpha_scatter, scatter_ld, tol, max_iter, S, S_ld, iterations, status, change};
    if (ng) {
        const int waves = lambda_waves_of<RtLambdaNg>(n_theta, n_depth, gpw);
        LaunchScope ls(ctx, "k_lambda", "k_lambda_ng");
        hipLaunchKernelGGL(k_lambda_ng, dim3(lambda_blocks(n_nu, gpw, waves)), dim3(64 * waves), waves * RtLambdaNg(n_theta, n_depth, gpw).bytes(), ctx->stream,
                           n_depth, n_nu, n_theta, n_theta, n_theta, nus, temps, ray_dist, mean_weights, alphas, ald, thermal, thermal_ld, J, J_ld, gpw, waves,
                           LambdaIterationNg{it, ng->start, ng->period, ng->accelerations});
    } else {
        const int waves = lambda_waves(n_theta, n_depth, gpw);
        LaunchScope ls(ctx, "k_lambda", "k_lambda<true>");
        hipLaunchKernelGGL(k_lambda<true>, dim3(lambda_blocks(n_nu, gpw, waves)), dim3(64 * waves), waves * RtLambda(n_theta, n_depth, gpw).bytes(), ctx->stream,
                           n_depth, n_nu, n_theta, n_theta, n_theta, nus, temps, ray_dist, mean_weights, alphas, ald, thermal, thermal_ld, J, J_ld, (double*)nullptr,
                           (int64_t)0, gpw, waves, it);
    }
    return check_launch("k_lambda");
}
}  // namespace
}  // extern "C++"

int sdx_scatter_source_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                           const double* mean_weights, const double* alphas, int64_t ald, const double* alpha_scatter, int64_t scatter_ld,
                           const double* thermal, int64_t thermal_ld, double tol, int max_iter, double* S, int64_t S_ld, double* J, int64_t J_ld,
                           int* iterations, int* status, double* change)
{
    return scatter_source_device(ctx, nullptr, n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, alphas, ald, alpha_scatter, scatter_ld, thermal,
                                 thermal_ld, tol, max_iter, S, S_ld, J, J_ld, iterations, status, change);
}

int sdx_scatter_source_ng_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                              const double* mean_weights, const double* alphas, int64_t ald, const double* alpha_scatter, int64_t scatter_ld,
                              const double* thermal, int64_t thermal_ld, double tol, int max_iter, double* S, int64_t S_ld, double* J, int64_t J_ld,
                              int* iterations, int* status, double* change, int ng_start, int ng_period, int* accelerations)
{
    if (int rc = acceleration_check(kScatterSourceNg, ng_start, ng_period)) return rc;  // (its own scalars first: they need no context)
    const NgOptions ng{ng_start, ng_period, accelerations};
    return scatter_source_device(ctx, &ng, n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, alphas, ald, alpha_scatter, scatter_ld, thermal,
                                 thermal_ld, tol, max_iter, S, S_ld, J, J_ld, iterations, status, change);
}

int sdx_mean_intensity_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                           const double* mean_weights, const double* alphas, const double* source, double* J, double* lambda_diag)
{
    if (const int no = column_gate<RtLambda>(ctx, kMeanIntensity, n_depth, n_nu, n_theta); no < 0) return no;
    if (n_nu == 0) return SDX_OK;
    const Columns h = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, {alphas, n_nu}, {source, n_nu});
    REQUIRE(columns_given(h, true, true), "mean_intensity: null pointer");
    REQUIRE(J || lambda_diag, "mean_intensity: no output requested");
    double *d_j, *d_l;
    const auto rows = [&](HostPlan& plan, size_t plane, Columns& d) {
        plan.in(source, plane, &d.source.p);
        plan.out(J, plane, &d_j);
        plan.out(lambda_diag, plane, &d_l);
    };
    return columns_host(ctx, h, n_theta, rows, [&](const Columns& d) {
        return sdx_mean_intensity_dev(ctx, n_depth, n_nu, n_theta, d.g.nus, d.rays.temps, d.rays.ray_dist, d.rays.wts, d.alphas.p, n_nu, d.source.p, n_nu, d_j, n_nu, d_l, n_nu);
    });
}

extern "C++" {
namespace {
int scatter_source_host(sdx_ctx* ctx, const NgOptions* ng, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                        const double* ray_dist, const double* mean_weights, const double* alphas, const double* alpha_scatter, int scatter_per_frequency,
                        const double* thermal, double tol, int max_iter, double* S, double* J, int* iterations, int* status, double* change)
{
    const ColumnEntry& e = ng ? kScatterSourceNg : kScatterSource;
    if (const int no = ng ? column_gate<RtLambdaNg>(ctx, e, n_depth, n_nu, n_theta) : column_gate<RtLambda>(ctx, e, n_depth, n_nu, n_theta); no < 0) return no;
    if (int rc = iteration_check(e, tol, max_iter)) return rc;
    if (n_nu == 0) return SDX_OK;
    const Columns h = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, {alphas, n_nu}, {thermal, n_nu});
    REQUIRE(columns_given(h, true, true) && alpha_scatter && S, "scatter_source: null pointer");
    const double* d_sc;
    double *d_s, *d_j, *d_c;
    int *d_it, *d_st, *d_acc = nullptr;
    const auto rows = [&](HostPlan& plan, size_t plane, Columns& d) {
        plan.in(alpha_scatter, scatter_per_frequency ? plane : (size_t)n_depth * sizeof(double), &d_sc);
        plan.in(thermal, plane, &d.source.p);
        plan.out(S, plane, &d_s);
        plan.out(J, plane, &d_j);
        plan.out(iterations, (size_t)n_nu * sizeof(int), &d_it);
        plan.out(status, (size_t)n_nu * sizeof(int), &d_st);
        plan.out(change, (size_t)n_nu * sizeof(double), &d_c);
        if (ng) plan.out(ng->accelerations, (size_t)n_nu * sizeof(int), &d_acc);
    };
    return columns_host(ctx, h, n_theta, rows, [&](const Columns& d) {
        const NgOptions on_device{ng ? ng->start : 0, ng ? ng->period : 0, d_acc};
        return scatter_source_device(ctx, ng ? &on_device : nullptr, n_depth, n_nu, n_theta, d.g.nus, d.rays.temps, d.rays.ray_dist, d.rays.wts, d.alphas.p, n_nu,
                                     d_sc, scatter_per_frequency ? n_nu : 0, d.source.p, n_nu, tol, max_iter, d_s, n_nu, d_j, n_nu, d_it, d_st, d_c);
    });
}
}  // namespace
}  // extern "C++"

int sdx_scatter_source_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                           const double* mean_weights, const double* alphas, const double* alpha_scatter, int scatter_per_frequency,
                           const double* thermal, double tol, int max_iter, double* S, double* J, int* iterations, int* status, double* change)
{
    return scatter_source_host(ctx, nullptr, n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, alphas, alpha_scatter, scatter_per_frequency, thermal,
                               tol, max_iter, S, J, iterations, status, change);
}

int sdx_scatter_source_ng_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                              const double* mean_weights, const double* alphas, const double* alpha_scatter, int scatter_per_frequency,
                              const double* thermal, double tol, int max_iter, double* S, double* J, int* iterations, int* status, double* change,
                              int ng_start, int ng_period, int* accelerations)
{
    if (int rc = acceleration_check(kScatterSourceNg, ng_start, ng_period)) return rc;  // (its own scalars first: they need no context)
    const NgOptions ng{ng_start, ng_period, accelerations};
    return scatter_source_host(ctx, &ng, n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, alphas, alpha_scatter, scatter_per_frequency, thermal,
                               tol, max_iter, S, J, iterations, status, change);
}

// ---- the adjoint of the mean intensity and of the scattering solve (k_lambda_adjoint) ---------------------------------------
int sdx_mean_intensity_adjoint_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                                   const double* ray_dist, const double* mean_weights, const double* alphas, int64_t ald, const double* z, int64_t z_ld,
                                   const double* source, int64_t source_ld, double* Lt, int64_t Lt_ld, double* G, int64_t G_ld)
{
    const int gpw = column_gate<RtLambdaAdjoint>(ctx, kMeanIntensityAdjoint, n_depth, n_nu, n_theta);
    if (gpw < 0) return gpw;
    if (n_nu == 0) return SDX_OK;
    const Columns c = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, {alphas, ald}, {source, source_ld});
    REQUIRE(Lt || G, "mean_intensity_adjoint: no output requested");
    REQUIRE(columns_given(c) && z && z_ld >= n_nu, "mean_intensity_adjoint: null pointer or a leading dimension of an input below n_nu");
    REQUIRE(fits(Lt, Lt_ld, n_nu) && fits(G, G_ld, n_nu), "mean_intensity_adjoint: leading dimension of an output below n_nu");
    if (int rc = source_or_temps(kMeanIntensityAdjoint, "source", c)) return rc;
    const RtLambdaAdjoint lay(n_theta, n_depth, gpw);
    const int waves = lay.waves();
    {
        LaunchScope ls(ctx, "k_lambda_adjoint", "k_lambda_adjoint<false>");
        hipLaunchKernelGGL(k_lambda_adjoint<false>, dim3(lay.blocks(n_nu)), dim3(64 * waves), waves * lay.bytes(), ctx->stream, n_depth, n_nu, n_theta, n_theta,
                           n_theta, nus, temps, ray_dist, mean_weights, alphas, ald, source, source_ld, z, z_ld, Lt, Lt_ld, G, G_ld, gpw, waves, LambdaAdjointSolve{});
    }
    return check_launch("k_lambda_adjoint");
}

int sdx_scatter_response_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                             const double* mean_weights, const double* alphas, int64_t ald, const double* alpha_scatter, int64_t scatter_ld,
                             const double* thermal, int64_t thermal_ld, const double* S, int64_t S_ld, const double* cotangent, int64_t cotangent_ld,
                             const double* direct, int64_t direct_ld, double tol, int max_iter, double* y, int64_t y_ld, double* R_thermal,
                             int64_t R_thermal_ld, double* R_absorption, int64_t R_absorption_ld, double* R_scatter, int64_t R_scatter_ld,
                             int* iterations, int* status, double* change)
{
    const int gpw = column_gate<RtLambdaAdjoint>(ctx, kScatterResponse, n_depth, n_nu, n_theta);
    if (gpw < 0) return gpw;
    if (int rc = iteration_check(kScatterResponse, tol, max_iter)) return rc;
    if (n_nu == 0) return SDX_OK;
    const Columns c = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, {alphas, ald}, {thermal, thermal_ld});
    REQUIRE(y || R_thermal || R_absorption || R_scatter, "scatter_response: no output requested");
    REQUIRE(columns_given(c) && alpha_scatter && S && cotangent, "scatter_response: null pointer or alpha_ld below n_nu");
    REQUIRE((scatter_ld == 0 || scatter_ld >= n_nu) && S_ld >= n_nu && cotangent_ld >= n_nu && fits(direct, direct_ld, n_nu),
            "scatter_response: a leading dimension of an input below n_nu (scatter_ld: 0 or >= n_nu)");
    REQUIRE(fits(y, y_ld, n_nu) && fits(R_thermal, R_thermal_ld, n_nu) && fits(R_absorption, R_absorption_ld, n_nu) && fits(R_scatter, R_scatter_ld, n_nu),
            "scatter_response: leading dimension of an output below n_nu");
    if (int rc = source_or_temps(kScatterResponse, "thermal", c)) return rc;
    const RtLambdaAdjoint lay(n_theta, n_depth, gpw);
    const int waves = lay.waves();
    {
        LaunchScope ls(ctx, "k_lambda_adjoint", "k_lambda_adjoint<true>");
        hipLaunchKernelGGL(k_lambda_adjoint<true>, dim3(lay.blocks(n_nu)), dim3(64 * waves), waves * lay.bytes(), ctx->stream, n_depth, n_nu, n_theta, n_theta,
                           n_theta, nus, temps, ray_dist, mean_weights, alphas, ald, S, S_ld, (const double*)nullptr, (int64_t)0, (double*)nullptr, (int64_t)0,
                           (double*)nullptr, (int64_t)0, gpw, waves,
                           LambdaAdjointSolve{alpha_scatter, scatter_ld, thermal, thermal_ld, cotangent, cotangent_ld, direct, direct_ld, tol, max_iter, y, y_ld,
                                              R_thermal, R_thermal_ld, R_absorption, R_absorption_ld, R_scatter, R_scatter_ld, iterations, status, change});
    }
    return check_launch("k_lambda_adjoint");
}

int sdx_mean_intensity_adjoint_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps,
                                   const double* ray_dist, const double* mean_weights, const double* alphas, const double* z, const double* source,
                                   double* Lt, double* G)
{
    if (const int no = column_gate<RtLambdaAdjoint>(ctx, kMeanIntensityAdjoint, n_depth, n_nu, n_theta); no < 0) return no;
    if (n_nu == 0) return SDX_OK;
    const Columns h = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, {alphas, n_nu}, {source, n_nu});
    REQUIRE(columns_given(h, true, true) && z, "mean_intensity_adjoint: null pointer");
    REQUIRE(Lt || G, "mean_intensity_adjoint: no output requested");
    const double* d_z;
    double *d_lt, *d_g;
    const auto rows = [&](HostPlan& plan, size_t plane, Columns& d) {
        plan.in(z, plane, &d_z);
        plan.in(source, plane, &d.source.p);
        plan.out(Lt, plane, &d_lt);
        plan.out(G, plane, &d_g);
    };
    return columns_host(ctx, h, n_theta, rows, [&](const Columns& d) {
        return sdx_mean_intensity_adjoint_dev(ctx, n_depth, n_nu, n_theta, d.g.nus, d.rays.temps, d.rays.ray_dist, d.rays.wts, d.alphas.p, n_nu, d_z, n_nu,
                                              d.source.p, n_nu, d_lt, n_nu, d_g, n_nu);
    });
}

int sdx_scatter_response_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                             const double* mean_weights, const double* alphas, const double* alpha_scatter, int scatter_per_frequency,
                             const double* thermal, const double* S, const double* cotangent, const double* direct, double tol, int max_iter, double* y,
                             double* R_thermal, double* R_absorption, double* R_scatter, int* iterations, int* status, double* change)
{
    if (const int no = column_gate<RtLambdaAdjoint>(ctx, kScatterResponse, n_depth, n_nu, n_theta); no < 0) return no;
    if (int rc = iteration_check(kScatterResponse, tol, max_iter)) return rc;
    if (n_nu == 0) return SDX_OK;
    const Columns h = columns(n_depth, n_nu, n_theta, nus, temps, ray_dist, mean_weights, {alphas, n_nu}, {thermal, n_nu});
    REQUIRE(columns_given(h, true, true) && alpha_scatter && S && cotangent, "scatter_response: null pointer");
    REQUIRE(y || R_thermal || R_absorption || R_scatter, "scatter_response: no output requested");
    const double *d_sc, *d_s, *d_c, *d_d;
    double *d_y, *d_rt, *d_ra, *d_rs, *d_ch;
    int *d_it, *d_st;
    const auto rows = [&](HostPlan& plan, size_t plane, Columns& d) {
        plan.in(alpha_scatter, scatter_per_frequency ? plane : (size_t)n_depth * sizeof(double), &d_sc);
        plan.in(thermal, plane, &d.source.p);
        plan.in(S, plane, &d_s);
        plan.in(cotangent, plane, &d_c);
        plan.in(direct, plane, &d_d);
        plan.out(y, plane, &d_y);
        plan.out(R_thermal, plane, &d_rt);
        plan.out(R_absorption, plane, &d_ra);
        plan.out(R_scatter, plane, &d_rs);
        plan.out(iterations, (size_t)n_nu * sizeof(int), &d_it);
        plan.out(status, (size_t)n_nu * sizeof(int), &d_st);
        plan.out(change, (size_t)n_nu * sizeof(double), &d_ch);
    };
    return columns_host(ctx, h, n_theta, rows, [&](const Columns& d) {
        return sdx_scatter_response_dev(ctx, n_depth, n_nu, n_theta, d.g.nus, d.rays.temps, d.rays.ray_dist, d.rays.wts, d.alphas.p, n_nu, d_sc,
                                        scatter_per_frequency ? n_nu : 0, d.source.p, n_nu, d_s, n_nu, d_c, n_nu, d_d, n_nu, tol, max_iter, d_y, n_nu, d_rt, n_nu, d_ra,
                                        n_nu, d_rs, n_nu, d_it, d_st, d_ch);
    });
}

// ---- per-line flux sensitivities (k_response_weight, k_line_adjoint) --------------------------------------------------------
int sdx_response_weight_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* R_alpha, int64_t R_ld, const double* total, int64_t total_ld,
                            const double* nu_weight, double* weight, int64_t weight_ld)
{
    REQUIRE(ctx && n_depth >= 1 && n_depth <= 65535 && n_nu >= 0, "response_weight: need 1 <= n_depth <= 65535, n_nu >= 0");
    if (n_nu == 0) return SDX_OK;
    REQUIRE(R_alpha && total && weight && R_ld >= n_nu && total_ld >= n_nu && weight_ld >= n_nu, "response_weight: null pointer or leading dimension below n_nu");
    {
        LaunchScope ls(ctx, "k_response_weight");
        hipLaunchKernelGGL(k_response_weight, grid2(n_nu, n_depth), dim3(kBlock), 0, ctx->stream, n_depth, n_nu, R_alpha, R_ld, total, total_ld, nu_weight, weight,
                           weight_ld);
    }
    return check_launch("k_response_weight");
}

// ---- what the two line adjoints and the line tangent share -------------------------------------------------------------------------
// The refusals of all three device entries, under the entry's name (`what` and `kind`: the words of its mixed_precision message).
// Everything is checked before anything is enqueued, also for an empty grid.
static int line_entry_check(const char* name, const char* what, const char* kind, const sdx_ctx* ctx, int n_depth, int64_t n_nu, int64_t n_lines,
                            int gamma_cols, int64_t nu_begin, int64_t nu_count)
{
    const std::string s = std::string(name) + ": ";
    REQUIRE(ctx, s + "null context");
    REQUIRE(!ctx->mixed_precision, s + "no " + what + " with mixed_precision = 1 (the " + kind + " is that of the fp64 direct sum)");
    REQUIRE(n_depth > 0 && n_depth <= 65535 && n_nu >= 0 && n_lines >= 0 && n_nu < (int64_t)2147483647, s + "need 1 <= n_depth <= 65535, sizes >= 0 and n_nu within int32");
    REQUIRE(n_lines * (int64_t)n_depth < (int64_t)2147483647 - 64, s + "n_lines * n_depth must fit int32");
    REQUIRE(gamma_cols == n_depth || gamma_cols == 1, s + "gammas must have n_depth or 1 columns");
    REQUIRE(nu_begin >= 0 && nu_count >= 0 && nu_begin + nu_count <= n_nu, s + "frequency shard outside the grid");
    return SDX_OK;
}

// adj_ws: the head that k_line_adjoint_setup writes (pd, counters, centre) into `w`, then `tail` bytes of the entry's own -> *rest
static int adj_scratch(sdx_ctx* ctx, int n_depth, int64_t n_lines, size_t tail, AdjWork& w, char** rest)
{
    const size_t b_cnt = HostPlan::pad(4 * (size_t)(4 + n_depth)), b_lines = HostPlan::pad(4 * (size_t)n_lines);
    int rc = ensure(ctx, &ctx->adj_ws, &ctx->adj_ws_bytes, 256 + b_cnt + b_lines + tail);
    if (rc) return rc;
    char* p = (char*)ctx->adj_ws;
    w.pd = (double*)p, p += 256;
    w.counters = (int*)p, p += b_cnt;
    w.centre = (int*)p, p += b_lines;
    *rest = p;
    return SDX_OK;
}

static void launch_adjoint_setup(sdx_ctx* ctx, const AdjLines& a, const AdjWork& w)
{
    hipLaunchKernelGGL(k_line_adjoint_setup, dim3(1 + (unsigned)((a.n_lines + kPreBlock - 1) / kPreBlock)), dim3(kPreBlock), 0, ctx->stream, a, w);
}

// One adjoint of k_sums sums per item: the scratch behind the head (the four item tables, sld [k_sums][items] unless the caller's `sld`
// is given, partial [cap][k_sums]) and six launches under the stage name `stage`: the grid spacing and the centres, the item lists, the
// short, the long and the tiled items, the sums per line.
using AdjWalk = void (*)(AdjLines, AdjWork, const double*, int64_t);
using AdjTiledWalk = void (*)(AdjLines, AdjWork, const double*, int64_t, int);
extern "C++" template <class GatherArg>
static int line_adjoint_launch(sdx_ctx* ctx, const char* stage, int k_sums, const AdjLines& a, const double* weight, int64_t weight_ld, double* sld,
                               AdjWalk k_short, AdjWalk k_long, AdjTiledWalk k_tiled, void (*k_gather)(AdjLines, AdjWork, GatherArg), GatherArg gather_arg)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t n_items = a.n_lines * a.n_depth;
    AdjWork w{};
    w.n_tiles = (int)((a.nu_count + kAdjTile - 1) / kAdjTile);
    w.cap = std::min<int64_t>(std::max<int64_t>(ctx->adjoint_partials / k_sums, n_items), n_items * w.n_tiles);
    const size_t b_int = HostPlan::pad(4 * (size_t)n_items), b_sums = sld ? 0 : HostPlan::pad(8 * (size_t)n_items * k_sums);
    char* p;
    int rc = adj_scratch(ctx, a.n_depth, a.n_lines, 4 * b_int + b_sums + HostPlan::pad(8 * (size_t)w.cap * k_sums), w, &p);
    if (rc) return rc;
    w.list_short = (int*)p, p += b_int;
    w.list_long = (int*)p, p += b_int;
    w.list_tiled = (int*)p, p += b_int;
    w.tslot = (int*)p, p += b_int;
    w.sld = sld ? sld : (double*)p, p += b_sums;
    w.partial = (double*)p;
    const int64_t cap = (int64_t)ctx->n_cu * 32;  // blocks of a list walk: the lists' lengths are known on the device only
    const unsigned nb_short = (unsigned)std::min<int64_t>(cap, (n_items + 63) / 64);
    const unsigned nb_long = (unsigned)std::min<int64_t>(cap, (n_items + 3) / 4);
    // the tiled role: a wave per (depth, supertile, line subset); the line subsets fill the chip where depths x tiles alone do not
    const int64_t dt = (int64_t)a.n_depth * w.n_tiles;
    const int J = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)32, a.n_lines, ((int64_t)ctx->n_cu * 32 + dt - 1) / dt}));
    {
        LaunchScope ls(ctx, stage);
        launch_adjoint_setup(ctx, a, w);
        hipLaunchKernelGGL(k_line_adjoint_plan, dim3(blocks1(n_items)), dim3(kBlock), 0, ctx->stream, a, w);
        hipLaunchKernelGGL(k_short, dim3(nb_short), dim3(kBlock), 0, ctx->stream, a, w, weight, weight_ld);
        hipLaunchKernelGGL(k_long, dim3(nb_long), dim3(kBlock), 0, ctx->stream, a, w, weight, weight_ld);
        hipLaunchKernelGGL(k_tiled, dim3((unsigned)((dt * J + 3) / 4)), dim3(kBlock), 0, ctx->stream, a, w, weight, weight_ld, J);
        hipLaunchKernelGGL(k_gather, dim3((unsigned)((a.n_lines + 3) / 4)), dim3(kBlock), 0, ctx->stream, a, w, gather_arg);
    }
    return check_launch(stage);
}

// nus and the four line tables of a host-buffer twin into its plan, in the order of the arena
struct LineTables {
    const double *nus, *line_nus, *doppler, *gammas, *alphas;
};
static void plan_line_tables(HostPlan& plan, LineTables& d, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                             const double* doppler, const double* gammas, int gamma_cols, const double* alphas)
{
    const size_t f8 = sizeof(double), items = (size_t)n_lines * n_depth * f8;
    plan.in(nus, (size_t)n_nu * f8, &d.nus);
    plan.in(line_nus, (size_t)n_lines * f8, &d.line_nus);
    plan.in(doppler, items, &d.doppler);
    plan.in(gammas, (size_t)n_lines * gamma_cols * f8, &d.gammas);
    plan.in(alphas, items, &d.alphas);
}

int sdx_line_adjoint_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count, int64_t n_lines,
                         const double* line_nus, const double* doppler, const double* gammas, int gamma_cols, const double* alphas,
                         const double* weight, int64_t weight_ld, double* out_line, double* out_line_depth)
{
    int rc = line_entry_check("line_adjoint", "per-line sensitivities", "adjoint", ctx, n_depth, n_nu, n_lines, gamma_cols, nu_begin, nu_count);
    if (rc) return rc;
    REQUIRE(out_line || out_line_depth, "line_adjoint: no output requested");
    if (n_nu == 0 || n_lines == 0 || nu_count == 0) return SDX_OK;
    REQUIRE(nus && line_nus && doppler && gammas && alphas && weight && weight_ld >= nu_count, "line_adjoint: null pointer or weight_ld below nu_count");
    REQUIRE((int64_t)n_depth * ((nu_count + kAdjTile - 1) / kAdjTile) < ((int64_t)1 << 26), "line_adjoint: n_depth * nu_count too large for one launch");
    const AdjLines a{n_depth, gamma_cols, n_nu, nu_begin, nu_count, n_lines, nus, line_nus, doppler, gammas, alphas};
    return line_adjoint_launch(ctx, "k_line_adjoint", StrengthSums::kSums, a, weight, weight_ld, out_line_depth, k_line_adjoint<4>, k_line_adjoint<64>, k_line_adjoint_tiled,
                               k_line_adjoint_gather, out_line);
}

int sdx_line_adjoint_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus, const double* doppler,
                         const double* gammas, int gamma_cols, const double* alphas, const double* weight, double* out_line, double* out_line_depth)
{
    int rc;
    if ((rc = sdx_line_adjoint_dev(ctx, n_depth, 0, nullptr, 0, 0, n_lines, nullptr, nullptr, nullptr, gamma_cols, nullptr, nullptr, 0, out_line, out_line_depth)))
        return rc;  // refusals before any copy
    REQUIRE(n_nu >= 0, "line_adjoint: negative n_nu");
    if (n_nu == 0 || n_lines == 0) return SDX_OK;
    REQUIRE(nus && line_nus && doppler && gammas && alphas && weight, "line_adjoint: null pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), items = (size_t)n_lines * n_depth * f8;
    const double* d_wt;
    LineTables t;
    double *d_line, *d_ld;
    HostPlan plan;
    plan_line_tables(plan, t, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas);
    plan.in(weight, (size_t)n_depth * n_nu * f8, &d_wt);
    plan.out(out_line, (size_t)n_lines * f8, &d_line);
    plan.out(out_line_depth, items, &d_ld);
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_line_adjoint_dev(ctx, n_depth, n_nu, t.nus, 0, n_nu, n_lines, t.line_nus, t.doppler, t.gammas, gamma_cols, t.alphas, d_wt, n_nu, d_line, d_ld))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ---- line-profile sensitivities (k_line_param_adjoint) ----------------------------------------------------------------------
int sdx_line_param_adjoint_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count, int64_t n_lines,
                               const double* line_nus, const double* doppler, const double* gammas, int gamma_cols, const double* alphas,
                               const double* weight, int64_t weight_ld, double* out_damping, double* out_doppler, double* out_centre,
                               double* out_damping_depth, double* out_doppler_depth, double* out_centre_depth)
{
    int rc = line_entry_check("line_param_adjoint", "line-profile sensitivities", "adjoint", ctx, n_depth, n_nu, n_lines, gamma_cols, nu_begin, nu_count);
    if (rc) return rc;
    REQUIRE(out_damping || out_doppler || out_centre || out_damping_depth || out_doppler_depth || out_centre_depth, "line_param_adjoint: no output requested");
    if (n_nu == 0 || n_lines == 0 || nu_count == 0) return SDX_OK;
    REQUIRE(nus && line_nus && doppler && gammas && alphas && weight && weight_ld >= nu_count, "line_param_adjoint: null pointer or weight_ld below nu_count");
    REQUIRE((int64_t)n_depth * ((nu_count + kAdjTile - 1) / kAdjTile) < ((int64_t)1 << 26), "line_param_adjoint: n_depth * nu_count too large for one launch");
    const AdjLines a{n_depth, gamma_cols, n_nu, nu_begin, nu_count, n_lines, nus, line_nus, doppler, gammas, alphas};
    const ParamOut o{out_damping, out_doppler, out_centre, out_damping_depth, out_doppler_depth, out_centre_depth};
    return line_adjoint_launch(ctx, "k_line_param_adjoint", ProfileSums::kSums, a, weight, weight_ld, nullptr, k_line_param_adjoint<4>, k_line_param_adjoint<64>,
                               k_line_param_adjoint_tiled, k_line_param_adjoint_gather, o);
}

int sdx_line_param_adjoint_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus, const double* doppler,
                               const double* gammas, int gamma_cols, const double* alphas, const double* weight, double* out_damping,
                               double* out_doppler, double* out_centre, double* out_damping_depth, double* out_doppler_depth, double* out_centre_depth)
{
    int rc;
    if ((rc = sdx_line_param_adjoint_dev(ctx, n_depth, 0, nullptr, 0, 0, n_lines, nullptr, nullptr, nullptr, gamma_cols, nullptr, nullptr, 0, out_damping,
                                         out_doppler, out_centre, out_damping_depth, out_doppler_depth, out_centre_depth)))
        return rc;  // refusals before any copy
    REQUIRE(n_nu >= 0, "line_param_adjoint: negative n_nu");
    if (n_nu == 0 || n_lines == 0) return SDX_OK;
    REQUIRE(nus && line_nus && doppler && gammas && alphas && weight, "line_param_adjoint: null pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), items = (size_t)n_lines * n_depth * f8;
    const double* d_wt;
    LineTables t;
    double* d_out[6];
    double* const host_out[6] = {out_damping, out_doppler, out_centre, out_damping_depth, out_doppler_depth, out_centre_depth};
    HostPlan plan;
    plan_line_tables(plan, t, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas);
    plan.in(weight, (size_t)n_depth * n_nu * f8, &d_wt);
    for (int k = 0; k < 6; ++k) plan.out(host_out[k], k < 3 ? (size_t)n_lines * f8 : items, &d_out[k]);
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_line_param_adjoint_dev(ctx, n_depth, n_nu, t.nus, 0, n_nu, n_lines, t.line_nus, t.doppler, t.gammas, gamma_cols, t.alphas, d_wt, n_nu, d_out[0], d_out[1], d_out[2],
                                         d_out[3], d_out[4], d_out[5])))
        return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ---- isolated-line equivalent widths (k_line_ew) -----------------------------------------------------------------------------------
// The adjoints' checks (line_entry_check) and its own, all before anything is enqueued.  Five launches under the stage name k_line_ew: the
// grid spacing and the centres (k_line_adjoint_setup), the unions and unit counts, their prefix sums, the walk, the gather.  The scratch
// is the adjoints' (adj_scratch: their head, then the unions, the unit offsets and one (W, depth) pair per unit).  The number of units
// is known on the device only; the host bounds it from the shapes — no item has more segments than the shard — sizes `partial` by the
// bound and lets the walk's blocks stride the units, so nothing is read back and the entry can be captured once its scratch exists.
int sdx_line_equivalent_widths_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count, const double* x,
                                   int64_t n_lines, const double* line_nus, const double* doppler, const double* gammas, int gamma_cols,
                                   const double* alphas, int64_t n_sel, const int64_t* line_index, int n_scale, const double* scale,
                                   const double* background, int64_t background_ld, int n_theta, const double* temps, const double* ray_dist,
                                   const double* wts, double* out_W, double* out_depth)
{
    // the model's own limits first (whatever the tables look like), then what the line adjoints check
    REQUIRE(ctx, "line_equivalent_widths: null context");
    REQUIRE(n_depth >= 2, "line_equivalent_widths: need n_depth >= 2 (the formal solution has no gap to walk)");
    REQUIRE(n_theta > 0 && n_theta <= 64, "line_equivalent_widths: need 1 <= n_theta <= 64 (all angles are traced in one launch)");
    const int G = n_theta;
    const int gpw = rt_fit_gpw<EwColumns>(G, n_depth);
    REQUIRE(gpw > 0, "line_equivalent_widths: no equivalent widths for models this deep (the columns do not fit LDS at one frequency per wave)");
    int rc = line_entry_check("line_equivalent_widths", "equivalent widths", "line's term", ctx, n_depth, n_nu, n_lines, gamma_cols, nu_begin, nu_count);
    if (rc) return rc;
    REQUIRE(n_sel >= 0 && n_scale >= 1, "line_equivalent_widths: need n_sel >= 0 and n_scale >= 1");
    REQUIRE(line_index || n_sel == n_lines, "line_equivalent_widths: without line_index every line is selected, n_sel = n_lines");
    REQUIRE(out_W || out_depth, "line_equivalent_widths: no output requested");
    if (n_sel == 0 || nu_count == 0) return SDX_OK;
    REQUIRE(n_lines > 0, "line_equivalent_widths: lines selected from an empty list");
    REQUIRE(nus && x && line_nus && doppler && gammas && alphas && background && background_ld >= nu_count && temps && ray_dist && wts,
            "line_equivalent_widths: null pointer or background_ld below nu_count");
    const int64_t n_items = n_sel * (int64_t)n_scale;
    const int64_t seg_max = (nu_count + kEwSegment - 1) / kEwSegment;
    REQUIRE(n_items < ((int64_t)1 << 26) / seg_max, "line_equivalent_widths: n_sel * n_scale * nu_count too large for one call (select fewer lines)");
    const int64_t unit_max = n_items * seg_max;
    HIP_TRY(hipSetDevice(ctx->device));
    AdjWork head{};
    char* p;
    const size_t b_int = HostPlan::pad(4 * (size_t)(n_items + 1));
    if ((rc = adj_scratch(ctx, n_depth, n_lines, 3 * b_int + HostPlan::pad(16 * (size_t)unit_max), head, &p))) return rc;
    EwWork w{};
    w.pd = head.pd, w.centre = head.centre;
    w.ulo = (int*)p, p += b_int;
    w.uhi = (int*)p, p += b_int;
    w.uoff = (int*)p, p += b_int;
    w.partial = (double2*)p;
    const AdjLines lines{n_depth, gamma_cols, n_nu, nu_begin, nu_count, n_lines, nus, line_nus, doppler, gammas, alphas};
    const EwArgs a{n_depth, gamma_cols, n_scale, n_theta, n_nu, nu_begin, nu_count, n_lines, n_sel, nus, x, line_nus, doppler, gammas, alphas,
                   line_index, scale, background, background_ld, temps, ray_dist, wts};
    const unsigned walk_blocks = (unsigned)std::min<int64_t>(unit_max, (int64_t)ctx->n_cu * 16);
    {
        LaunchScope ls(ctx, "k_line_ew");
        launch_adjoint_setup(ctx, lines, head);
        hipLaunchKernelGGL(k_ew_plan, dim3(blocks1(n_items)), dim3(kBlock), 0, ctx->stream, a, w);
        hipLaunchKernelGGL(k_ew_scan, dim3(1), dim3(kPreBlock), 0, ctx->stream, n_items, w.uoff);
        hipLaunchKernelGGL(k_ew_walk, dim3(walk_blocks), dim3(kRtBlock), EwColumns(G, n_depth, gpw).bytes(), ctx->stream, a, w, G, gpw);
        hipLaunchKernelGGL(k_ew_gather, dim3(blocks1(n_items)), dim3(kBlock), 0, ctx->stream, n_items, w, out_W, out_depth);
    }
    return check_launch("k_line_ew");
}

// ---- the tangent of the line-opacity sum (k_line_tangent) ---------------------------------------------------------------------
// The adjoints' checks (line_entry_check) and its own.  Five launches under the stage name k_line_tangent: the grid spacing and the centres
// (k_line_adjoint_setup), the windows, the prefix of the wide items per depth, their lists, the plane.  The scratch is the adjoints'
// (adj_scratch: their head, then the tangent's tables).
int sdx_line_tangent_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count, int64_t n_lines,
                         const double* line_nus, const double* doppler, const double* gammas, int gamma_cols, const double* alphas,
                         const double* d_strength, const double* d_damping, const double* d_doppler, const double* d_centre, int dir_cols,
                         double* out, int64_t out_ld)
{
    int rc = line_entry_check("line_tangent", "line tangent", "tangent", ctx, n_depth, n_nu, n_lines, gamma_cols, nu_begin, nu_count);
    if (rc) return rc;
    REQUIRE(d_strength || d_damping || d_doppler || d_centre, "line_tangent: no direction given");
    REQUIRE(dir_cols == n_depth || dir_cols == 1, "line_tangent: the directions must have n_depth or 1 columns");
    if (n_nu == 0 || nu_count == 0) return SDX_OK;
    REQUIRE(nus && out && out_ld >= nu_count, "line_tangent: null pointer or out_ld below nu_count");
    REQUIRE(n_lines == 0 || (line_nus && doppler && gammas && alphas), "line_tangent: null pointer");
    const int n_tiles = (int)((nu_count + kTanTile - 1) / kTanTile);
    REQUIRE((int64_t)n_depth * n_tiles < ((int64_t)1 << 30), "line_tangent: n_depth * nu_count too large for one launch");
    HIP_TRY(hipSetDevice(ctx->device));
    TanWork w{};
    w.n_chunks = (int)((n_lines + kBlock - 1) / kBlock);
    const size_t b_int = HostPlan::pad(4 * (size_t)n_lines * n_depth), b_chunk = HostPlan::pad(4 * (size_t)w.n_chunks * n_depth);
    AdjWork setup{};  // what k_line_adjoint_setup writes: d_nu, the centres (and the adjoint's counters, not read here)
    char* p;
    if ((rc = adj_scratch(ctx, n_depth, n_lines, 3 * b_int + b_chunk + HostPlan::pad(4 * (size_t)n_depth), setup, &p))) return rc;
    w.pd = setup.pd, w.centre = setup.centre;
    w.win_lo = (int*)p, p += b_int;
    w.win_hi = (int*)p, p += b_int;
    w.list = (int*)p, p += b_int;
    w.chunk = (int*)p, p += b_chunk;
    w.n_wide = (int*)p;
    const AdjLines a{n_depth, gamma_cols, n_nu, nu_begin, nu_count, n_lines, nus, line_nus, doppler, gammas, alphas};
    const TanDirs dir{d_strength, d_damping, d_doppler, d_centre, dir_cols};
    {
        LaunchScope ls(ctx, "k_line_tangent");
        if (n_lines > 0) {
            const dim3 plan_grid((unsigned)w.n_chunks, (unsigned)n_depth);
            launch_adjoint_setup(ctx, a, setup);
            hipLaunchKernelGGL(k_line_tangent_plan, plan_grid, dim3(kBlock), 0, ctx->stream, a, dir, w);
            hipLaunchKernelGGL(k_line_tangent_scan, dim3((unsigned)n_depth), dim3(64), 0, ctx->stream, w);
            hipLaunchKernelGGL(k_line_tangent_list, plan_grid, dim3(kBlock), 0, ctx->stream, a, w);
        }
        const dim3 grid((unsigned)(((int64_t)n_depth * n_tiles + 3) / 4));
        if (d_damping || d_doppler || d_centre) hipLaunchKernelGGL(k_line_tangent<true>, grid, dim3(kBlock), 0, ctx->stream, a, dir, w, out, out_ld, n_tiles);
        else hipLaunchKernelGGL(k_line_tangent<false>, grid, dim3(kBlock), 0, ctx->stream, a, dir, w, out, out_ld, n_tiles);
    }
    return check_launch("k_line_tangent");
}

int sdx_line_tangent_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus, const double* doppler,
                         const double* gammas, int gamma_cols, const double* alphas, const double* d_strength, const double* d_damping,
                         const double* d_doppler, const double* d_centre, int dir_cols, double* out)
{
    int rc;
    if ((rc = sdx_line_tangent_dev(ctx, n_depth, 0, nullptr, 0, 0, n_lines, nullptr, nullptr, nullptr, gamma_cols, nullptr, d_strength, d_damping, d_doppler,
                                   d_centre, dir_cols, nullptr, 0)))
        return rc;  // refusals before any copy
    REQUIRE(n_nu >= 0, "line_tangent: negative n_nu");
    if (n_nu == 0) return SDX_OK;
    REQUIRE(nus && out && (n_lines == 0 || (line_nus && doppler && gammas && alphas)), "line_tangent: null pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), dirs = (size_t)n_lines * dir_cols * f8;
    const double* d_dir[4];
    LineTables t;
    const double* const host_dir[4] = {d_strength, d_damping, d_doppler, d_centre};
    double* d_out;
    HostPlan plan;
    plan_line_tables(plan, t, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas);
    for (int k = 0; k < 4; ++k) plan.in(host_dir[k], dirs, &d_dir[k]);
    plan.out(out, (size_t)n_depth * n_nu * f8, &d_out);
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_line_tangent_dev(ctx, n_depth, n_nu, t.nus, 0, n_nu, n_lines, t.line_nus, t.doppler, t.gammas, gamma_cols, t.alphas, d_dir[0], d_dir[1], d_dir[2], d_dir[3], dir_cols,
                                   d_out, n_nu)))
        return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ================================================================================================ post-processing
int sdx_convolve1d_reflect_dev(sdx_ctx* ctx, int64_t n, const double* in, int m, const double* weights, int symmetric, double* out)
{
    REQUIRE(ctx && n >= 0 && m > 0 && (m & 1), "convolve1d: need an odd kernel length");
    if (n == 0) return SDX_OK;
    REQUIRE(in && weights && out && in != out, "convolve1d: null or aliased pointer");
    {
        LaunchScope ls(ctx, "k_convolve1d_reflect");
        hipLaunchKernelGGL(k_convolve1d_reflect, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, in, m, weights, symmetric, out);
    }
    return check_launch("k_convolve1d_reflect");
}

int sdx_flux_nu_to_lambda_dev(sdx_ctx* ctx, int64_t n, const double* f_nu, const double* nus, const double* lambdas, double* out)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (f_nu && nus && lambdas && out)), "flux_nu_to_lambda: bad arguments");
    if (n == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_flux_nu_to_lambda");
        hipLaunchKernelGGL(k_flux_nu_to_lambda, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, f_nu, nus, lambdas, out);
    }
    return check_launch("k_flux_nu_to_lambda");
}

int sdx_divide_dev(sdx_ctx* ctx, int64_t n, const double* a, const double* b, double* out)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (a && b && out)), "divide: bad arguments");
    if (n == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_divide");
        hipLaunchKernelGGL(k_divide, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, a, b, out);
    }
    return check_launch("k_divide");
}

// ---- checks the instrument entries share ---------------------------------------------------------------------------------------------
// An output is none of the inputs and none of the other outputs (null pointers are no buffers).  With `own`, the entry's one message
// for both; without, the two messages of the tangent entries.
static int distinct_buffers(const char* name, const double* const* ins, int n_ins, const double* const* outs, int n_outs,
                            const char* own = nullptr)
{
    for (int a = 0; a < n_outs; ++a) {
        if (!outs[a]) continue;
        for (int b = 0; b < n_ins; ++b)
            if (outs[a] == ins[b]) return fail(SDX_ERR_ARG, std::string(name) + (own ? own : ": not in place (an output must not be one of the inputs)"));
        for (int b = a + 1; b < n_outs; ++b)
            if (outs[a] == outs[b]) return fail(SDX_ERR_ARG, std::string(name) + (own ? own : ": the outputs must be buffers of their own"));
    }
    return SDX_OK;
}

// what no kernel can check: the host-buffer twins do, before any upload
static int ascending_check(const char* name, const char* what, int64_t n, const double* x)
{
    for (int64_t i = 0; i < n; ++i)
        if (!(std::isfinite(x[i]) && (i == 0 || x[i - 1] < x[i])))
            return fail(SDX_ERR_ARG, std::string(name) + ": " + what + " must be finite and strictly ascending");
    return SDX_OK;
}

// ---- the instrument model (k_observe): Doppler shift, line-spread function and pixel integration in one launch ------------------
int sdx_observe_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                    const double* edges, const double* sigma, const double* doppler_dev, double* out)
{
    REQUIRE(ctx && n_pix >= 0, "observe: null context or n_pix < 0");
    if (n_pix == 0) return SDX_OK;
    REQUIRE(n >= 2, "observe: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && flux && edges && sigma && out, "observe: null pointer (lambdas, flux, edges, sigma and out are required)");
    REQUIRE((n_pix + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31), "observe: too many pixels for one launch");
    {
        // one wave per pixel (the last group's waves included: a short group is done by its first wave alone)
        const int64_t waves = (n_pix + kObsGroup - 1) / kObsGroup * kObsGroup;
        LaunchScope ls(ctx, "k_observe");
        hipLaunchKernelGGL(k_observe, dim3((unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, ctx->stream, n, lambdas, flux,
                           reference, n_pix, edges, sigma, doppler_dev, out);
    }
    return check_launch("k_observe");
}

// what the kernel cannot check: the host-buffer twin does, before any upload
static int observe_host_check(int64_t n, const double* lambdas, int64_t n_pix, const double* edges, const double* sigma, double doppler)
{
    REQUIRE(std::isfinite(doppler) && doppler > 0.0, "observe: doppler must be finite and > 0");
    int rc;
    if ((rc = ascending_check("observe", "lambdas", n, lambdas))) return rc;
    if ((rc = ascending_check("observe", "edges", n_pix + 1, edges))) return rc;
    for (int64_t j = 0; j < n_pix; ++j) REQUIRE(std::isfinite(sigma[j]) && sigma[j] > 0.0, "observe: sigma must be finite and > 0");
    return SDX_OK;
}

int sdx_observe_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                    const double* edges, const double* sigma, double doppler, double* out)
{
    REQUIRE(ctx && n_pix >= 0, "observe: null context or n_pix < 0");
    if (n_pix == 0) return SDX_OK;
    REQUIRE(n >= 2, "observe: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && flux && edges && sigma && out, "observe: null pointer (lambdas, flux, edges, sigma and out are required)");
    int rc;
    if ((rc = observe_host_check(n, lambdas, n_pix, edges, sigma, doppler))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), grid = (size_t)n * f8;
    const double *d_l, *d_f, *d_r, *d_e, *d_s, *d_D;
    double* d_o;
    HostPlan plan;
    plan.in(lambdas, grid, &d_l);
    plan.in(flux, grid, &d_f);
    plan.in(reference, grid, &d_r);
    plan.in(edges, (size_t)(n_pix + 1) * f8, &d_e);
    plan.in(sigma, (size_t)n_pix * f8, &d_s);
    plan.in(&doppler, f8, &d_D);
    plan.out(out, (size_t)n_pix * f8, &d_o);
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_observe_dev(ctx, n, d_l, d_f, d_r, n_pix, d_e, d_s, d_D, d_o))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ---- the tangent of the instrument model (k_observe_tangent): k_observe's launch geometry, one pass over the same windows ------
static int observe_tangent_check(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                                 const double* edges, const double* sigma, const double* dflux, const double* dreference, const double* out,
                                 const double* dout_velocity, const double* dout_lsf, const double* dout_flux)
{
    REQUIRE(ctx && n_pix >= 0, "observe_tangent: null context or n_pix < 0");
    if (n_pix == 0) return SDX_OK;
    REQUIRE(n >= 2, "observe_tangent: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && flux && edges && sigma, "observe_tangent: null pointer (lambdas, flux, edges and sigma are required)");
    REQUIRE(reference || !dreference, "observe_tangent: dreference needs a reference");
    REQUIRE(!dflux == !dout_flux, "observe_tangent: dflux and dout_flux go together");
    const double* const ins[7] = {lambdas, flux, reference, edges, sigma, dflux, dreference};
    const double* const outs[4] = {out, dout_velocity, dout_lsf, dout_flux};
    return distinct_buffers("observe_tangent", ins, 7, outs, 4);
}

int sdx_observe_tangent_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                            const double* edges, const double* sigma, const double* doppler_dev, const double* dflux,
                            const double* dreference, double* out, double* dout_velocity, double* dout_lsf, double* dout_flux)
{
    int rc;
    if ((rc = observe_tangent_check(ctx, n, lambdas, flux, reference, n_pix, edges, sigma, dflux, dreference, out, dout_velocity, dout_lsf, dout_flux)))
        return rc;
    if (n_pix == 0 || !(out || dout_velocity || dout_lsf || dout_flux)) return SDX_OK;
    REQUIRE((n_pix + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31), "observe_tangent: too many pixels for one launch");
    {
        // one wave per pixel (the last group's waves included: a short group is done by its first wave alone)
        const int64_t waves = (n_pix + kObsGroup - 1) / kObsGroup * kObsGroup;
        LaunchScope ls(ctx, "k_observe_tangent");
        hipLaunchKernelGGL(k_observe_tangent, dim3((unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, ctx->stream, n, lambdas,
                           flux, reference, n_pix, edges, sigma, doppler_dev, dflux, dflux ? dreference : nullptr, out, dout_velocity, dout_lsf,
                           dout_flux);
    }
    return check_launch("k_observe_tangent");
}

int sdx_observe_tangent_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                            const double* edges, const double* sigma, double doppler, const double* dflux, const double* dreference,
                            double* out, double* dout_velocity, double* dout_lsf, double* dout_flux)
{
    int rc;
    if ((rc = observe_tangent_check(ctx, n, lambdas, flux, reference, n_pix, edges, sigma, dflux, dreference, out, dout_velocity, dout_lsf, dout_flux)))
        return rc;
    if (n_pix == 0) return SDX_OK;
    if ((rc = observe_host_check(n, lambdas, n_pix, edges, sigma, doppler))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), grid = (size_t)n * f8, pix = (size_t)n_pix * f8;
    const double *d_l, *d_f, *d_r, *d_e, *d_s, *d_D, *d_df, *d_dr;
    double *d_o, *d_v, *d_k, *d_t;
    HostPlan plan;
    plan.in(lambdas, grid, &d_l);
    plan.in(flux, grid, &d_f);
    plan.in(reference, grid, &d_r);
    plan.in(edges, (size_t)(n_pix + 1) * f8, &d_e);
    plan.in(sigma, pix, &d_s);
    plan.in(&doppler, f8, &d_D);
    plan.in(dflux, grid, &d_df);
    plan.in(dreference, grid, &d_dr);
    plan.out(out, pix, &d_o);
    plan.out(dout_velocity, pix, &d_v);
    plan.out(dout_lsf, pix, &d_k);
    plan.out(dout_flux, pix, &d_t);
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_observe_tangent_dev(ctx, n, d_l, d_f, d_r, n_pix, d_e, d_s, d_D, d_df, d_dr, d_o, d_v, d_k, d_t))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// the pixel response and its two partials, point by point (k_observe_response_grad): what the tangent's loop evaluates
int sdx_observe_response_grad_dev(sdx_ctx* ctx, int64_t n, const double* e0, const double* e1, const double* x, const double* sigma,
                                  double* out_r, double* out_rx, double* out_rs)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (e0 && e1 && x && sigma && out_r && out_rx && out_rs)), "observe_response_grad: bad arguments");
    if (n == 0) return SDX_OK;
    {
        LaunchScope ls(ctx, "k_observe_response_grad");
        hipLaunchKernelGGL(k_observe_response_grad, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, e0, e1, x, sigma, out_r, out_rx, out_rs);
    }
    return check_launch("k_observe_response_grad");
}

int sdx_observe_response_grad_f64(sdx_ctx* ctx, int64_t n, const double* e0, const double* e1, const double* x, const double* sigma,
                                  double* out_r, double* out_rx, double* out_rs)
{
    REQUIRE(ctx && n >= 0 && (n == 0 || (e0 && e1 && x && sigma && out_r && out_rx && out_rs)), "observe_response_grad: bad arguments");
    if (n == 0) return SDX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * sizeof(double);
    const double *d_e0, *d_e1, *d_x, *d_s;
    double *d_r, *d_rx, *d_rs;
    HostPlan plan;
    plan.in(e0, bytes, &d_e0);
    plan.in(e1, bytes, &d_e1);
    plan.in(x, bytes, &d_x);
    plan.in(sigma, bytes, &d_s);
    plan.out(out_r, bytes, &d_r);
    plan.out(out_rx, bytes, &d_rx);
    plan.out(out_rs, bytes, &d_rs);
    HostIo io{ctx};
    int rc;
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_observe_response_grad_dev(ctx, n, d_e0, d_e1, d_x, d_s, d_r, d_rx, d_rs))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ---- the adjoint of the instrument model: pixel weights pulled back to the grid (k_observe_adjoint) ---------------------------
// Everything is checked before anything is enqueued.  Four launches under the stage name k_observe_adjoint: the per-pixel factors, the
// two scans (the tiles' partials, then the tiles), the gather per grid point.
int sdx_observe_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                            const double* edges, const double* sigma, const double* doppler_dev, const double* pixel_weight, const double* nus,
                            double* w_flux, double* w_reference)
{
    REQUIRE(ctx && n_pix >= 0, "observe_adjoint: null context or n_pix < 0");
    REQUIRE(n >= 2, "observe_adjoint: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && w_flux, "observe_adjoint: null pointer (lambdas and w_flux are required)");
    REQUIRE(n_pix == 0 || (edges && sigma && pixel_weight), "observe_adjoint: null pointer (edges, sigma and pixel_weight are required)");
    REQUIRE(reference || !w_reference, "observe_adjoint: w_reference needs a reference");
    REQUIRE(!reference || flux, "observe_adjoint: a reference needs the flux (out_j enters the cotangent of the reference)");
    REQUIRE((n_pix + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31) && (n + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31),
            "observe_adjoint: too many pixels or points for one launch");
    HIP_TRY(hipSetDevice(ctx->device));
    if (n_pix == 0) {
        HIP_TRY(hipMemsetAsync(w_flux, 0, (size_t)n * sizeof(double), ctx->stream));
        if (w_reference) HIP_TRY(hipMemsetAsync(w_reference, 0, (size_t)n * sizeof(double), ctx->stream));
        return SDX_OK;
    }
    const size_t row = ((size_t)n_pix * sizeof(double) + 255) & ~(size_t)255;
    const int64_t n_tiles = (n_pix + kObsScanTile - 1) / kObsScanTile;
    const size_t tile_row = (2 * (size_t)n_tiles * sizeof(double) + 255) & ~(size_t)255;
    int rc = ensure(ctx, &ctx->obs_ws, &ctx->obs_ws_bytes, 4 * row + tile_row);
    if (rc) return rc;
    double* const a = (double*)ctx->obs_ws;
    double* const b = (double*)((char*)ctx->obs_ws + row);
    double* const PH = (double*)((char*)ctx->obs_ws + 2 * row);
    double* const SL = (double*)((char*)ctx->obs_ws + 3 * row);
    double* const tiles = (double*)((char*)ctx->obs_ws + 4 * row);
    {
        // one wave per pixel, then one per grid point (a short group is done by its first wave alone)
        const int64_t pix_waves = (n_pix + kObsGroup - 1) / kObsGroup * kObsGroup, pt_waves = (n + kObsGroup - 1) / kObsGroup * kObsGroup;
        const int per = kBlock / 64;
        LaunchScope ls(ctx, "k_observe_adjoint");
        hipLaunchKernelGGL(k_observe_adjoint_pixels, dim3((unsigned)((pix_waves + per - 1) / per)), dim3(kBlock), 0, ctx->stream, n, lambdas, flux,
                           reference, n_pix, edges, sigma, doppler_dev, pixel_weight, a, b);
        hipLaunchKernelGGL(k_observe_adjoint_tiles, dim3((unsigned)n_tiles, 2), dim3(kBlock), 0, ctx->stream, n_pix, edges, sigma, n_tiles, tiles);
        hipLaunchKernelGGL(k_observe_adjoint_scan, dim3((unsigned)n_tiles, 2), dim3(kBlock), 0, ctx->stream, n_pix, edges, sigma, n_tiles,
                           (const double*)tiles, PH, SL);
        hipLaunchKernelGGL(k_observe_adjoint, dim3((unsigned)((pt_waves + per - 1) / per)), dim3(kBlock), 0, ctx->stream, n, lambdas, n_pix, edges,
                           sigma, doppler_dev, (const double*)a, reference ? (const double*)b : nullptr, (const double*)PH, (const double*)SL, nus,
                           w_flux, w_reference);
    }
    return check_launch("k_observe_adjoint");
}

int sdx_observe_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, int64_t n_pix,
                            const double* edges, const double* sigma, double doppler, const double* pixel_weight, const double* nus,
                            double* w_flux, double* w_reference)
{
    int rc;
    // the device entry's refusals, then what only the host can check, all before any copy
    REQUIRE(ctx && n_pix >= 0, "observe_adjoint: null context or n_pix < 0");
    REQUIRE(n >= 2, "observe_adjoint: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && w_flux && edges, "observe_adjoint: null pointer (lambdas, edges and w_flux are required)");
    REQUIRE(n_pix == 0 || (sigma && pixel_weight), "observe_adjoint: null pointer (sigma and pixel_weight are required)");
    REQUIRE(reference || !w_reference, "observe_adjoint: w_reference needs a reference");
    REQUIRE(!reference || flux, "observe_adjoint: a reference needs the flux (out_j enters the cotangent of the reference)");
    if ((rc = observe_host_check(n, lambdas, n_pix, edges, sigma, doppler))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), grid = (size_t)n * f8;
    const double *d_l, *d_f, *d_r, *d_e, *d_s, *d_D, *d_pw, *d_nus;
    double *d_wf, *d_wr;
    HostPlan plan;
    plan.in(lambdas, grid, &d_l);
    plan.in(reference ? flux : nullptr, grid, &d_f);  // (the flux enters only through the reference's cotangent)
    plan.in(reference, grid, &d_r);
    plan.in(edges, (size_t)(n_pix + 1) * f8, &d_e);
    plan.in(n_pix ? sigma : nullptr, (size_t)n_pix * f8, &d_s);
    plan.in(&doppler, f8, &d_D);
    plan.in(n_pix ? pixel_weight : nullptr, (size_t)n_pix * f8, &d_pw);
    plan.in(nus, grid, &d_nus);
    plan.out(w_flux, grid, &d_wf);
    plan.out(w_reference, grid, &d_wr);
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_observe_adjoint_dev(ctx, n, d_l, d_f, d_r, n_pix, d_e, d_s, d_D, d_pw, d_nus, d_wf, d_wr))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ---- the broadening stages: rotation (k_rotate, k_rotate_tangent), the cell-integrated profile (k_rotate_integrated) and
// radial-tangential macroturbulence (k_macroturbulence), each with its adjoint (k_*_adjoint_den, k_*_adjoint) ---------------------------
// one wave per grid point (the last group's waves included: a short group is done by its first wave alone)
static unsigned rotate_blocks(int64_t n)
{
    const int64_t waves = (n + kObsGroup - 1) / kObsGroup * kObsGroup;
    return (unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64));
}

// The adjoint of a stage, under its stage name ("k_" and the entry's name): a = u / den into the context's scratch, then the gather.
// An adjoint consumes its rows between its own two launches on the context's one stream, so the stages share the scratch.
typedef void (*StageDenKernel)(int64_t, const double*, const double*, const double*, const double*, double*, double*);
typedef void (*StageGatherKernel)(int64_t, const double*, const double*, const double*, const double*, const double*, double*, double*);
static int stage_adjoint(sdx_ctx* ctx, const char* stage, const char* scalars_name, StageDenKernel den, StageGatherKernel gather, int64_t n,
                         const double* lambdas, const double* scalars, const double* u, const double* u_reference, const double* nus, double* w,
                         double* w_reference)
{
    const auto msg = [&](const char* text) { return std::string(stage + 2) + text; };
    REQUIRE(ctx, msg(": null context"));
    REQUIRE(n >= 2, msg(": the grid needs at least two points (n >= 2)"));
    REQUIRE(lambdas && scalars && u && w, msg(": null pointer (lambdas, ") + scalars_name + ", u and w are required)");
    REQUIRE(!u_reference == !w_reference, msg(": u_reference and w_reference go together"));
    REQUIRE((n + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31), msg(": too many points for one launch"));
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t row = ((size_t)n * sizeof(double) + 255) & ~(size_t)255;
    int rc = ensure(ctx, &ctx->stage_ws, &ctx->stage_ws_bytes, 2 * row);
    if (rc) return rc;
    double* const a = (double*)ctx->stage_ws;
    double* const a_ref = (double*)((char*)ctx->stage_ws + row);
    {
        LaunchScope ls(ctx, stage);
        hipLaunchKernelGGL(den, dim3(rotate_blocks(n)), dim3(kBlock), 0, ctx->stream, n, lambdas, scalars, u, u_reference, a, a_ref);
        hipLaunchKernelGGL(gather, dim3(rotate_blocks(n)), dim3(kBlock), 0, ctx->stream, n, lambdas, scalars, (const double*)a,
                           u_reference ? (const double*)a_ref : nullptr, nus, w, w_reference);
    }
    return check_launch(stage);
}

// The host-buffer twin of a stage's forward entry: the grid, flux, reference and the stage's scalars (a device row) go up, up to six
// grid-sized outputs, each optional, come back.  dev: the device entry, on device addresses, its outputs in the order of outs.
typedef int (*StageForwardDev)(sdx_ctx*, int64_t, const double*, const double*, const double*, const double*, double* const*);
static int stage_forward_host(sdx_ctx* ctx, StageForwardDev dev, int64_t n, const double* lambdas, const double* flux, const double* reference,
                              const double* scalars, int n_scalars, double* const* outs, int n_outs)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), grid = (size_t)n * f8;
    const double *d_l, *d_f, *d_r, *d_s;
    double* d_o[6];
    HostPlan plan;
    plan.in(lambdas, grid, &d_l);
    plan.in(flux, grid, &d_f);
    plan.in(reference, grid, &d_r);
    plan.in(scalars, (size_t)n_scalars * f8, &d_s);
    for (int k = 0; k < n_outs; ++k) plan.out(outs[k], grid, &d_o[k]);
    HostIo io{ctx};
    int rc;
    if ((rc = io.stage(plan))) return rc;
    if ((rc = dev(ctx, n, d_l, d_f, d_r, d_s, d_o))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// The twin of a stage's adjoint entry (the three have one signature)
typedef int (*StageAdjointDev)(sdx_ctx*, int64_t, const double*, const double*, const double*, const double*, const double*, double*, double*);
static int stage_adjoint_host(sdx_ctx* ctx, StageAdjointDev dev, int64_t n, const double* lambdas, const double* scalars, int n_scalars,
                              const double* u, const double* u_reference, const double* nus, double* w, double* w_reference)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), grid = (size_t)n * f8;
    const double *d_l, *d_s, *d_u, *d_ur, *d_nus;
    double *d_w, *d_wr;
    HostPlan plan;
    plan.in(lambdas, grid, &d_l);
    plan.in(scalars, (size_t)n_scalars * f8, &d_s);
    plan.in(u, grid, &d_u);
    plan.in(u_reference, grid, &d_ur);
    plan.in(nus, grid, &d_nus);
    plan.out(w, grid, &d_w);
    plan.out(w_reference, grid, &d_wr);
    HostIo io{ctx};
    int rc;
    if ((rc = io.stage(plan))) return rc;
    if ((rc = dev(ctx, n, d_l, d_s, d_u, d_ur, d_nus, d_w, d_wr))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ---- rotational broadening (k_rotate) and its adjoint
int sdx_rotate_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, const double* rot_dev,
                   double* out, double* out_reference)
{
    REQUIRE(ctx, "rotate: null context");
    REQUIRE(n >= 2, "rotate: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && flux && rot_dev && out, "rotate: null pointer (lambdas, flux, rot_dev and out are required)");
    REQUIRE(!reference == !out_reference, "rotate: reference and out_reference go together");
    const double* const ins[2] = {flux, reference};
    const double* const outs[2] = {out, out_reference};
    int rc;
    if ((rc = distinct_buffers("rotate", ins, 2, outs, 2, ": not in place (out and out_reference must be buffers of their own)"))) return rc;
    REQUIRE((n + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31), "rotate: too many points for one launch");
    HIP_TRY(hipSetDevice(ctx->device));
    {
        LaunchScope ls(ctx, "k_rotate");
        hipLaunchKernelGGL(k_rotate, dim3(rotate_blocks(n)), dim3(kBlock), 0, ctx->stream, n, lambdas, flux, reference, rot_dev, out, out_reference);
    }
    return check_launch("k_rotate");
}

int sdx_rotate_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* rot_dev, const double* u, const double* u_reference,
                           const double* nus, double* w, double* w_reference)
{
    return stage_adjoint(ctx, "k_rotate_adjoint", "rot_dev", k_rotate_adjoint_den, k_rotate_adjoint, n, lambdas, rot_dev, u, u_reference, nus, w,
                         w_reference);
}

// what the kernels cannot check: the host-buffer twins do, before any upload
static int rotate_host_check(int64_t n, const double* lambdas, double v_rot, double limb_darkening)
{
    REQUIRE(std::isfinite(v_rot) && v_rot >= 0.0 && v_rot < 3000.0, "rotate: v_rot must be finite with 0 <= v_rot < 3000 km/s");
    REQUIRE(limb_darkening >= 0.0 && limb_darkening <= 1.0, "rotate: limb_darkening must lie in [0, 1]");
    return ascending_check("rotate", "lambdas", n, lambdas);
}

int sdx_rotate_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, double v_rot,
                   double limb_darkening, double* out, double* out_reference)
{
    REQUIRE(ctx, "rotate: null context");
    REQUIRE(n >= 2, "rotate: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && flux && out, "rotate: null pointer (lambdas, flux and out are required)");
    REQUIRE(!reference == !out_reference, "rotate: reference and out_reference go together");
    int rc;
    if ((rc = rotate_host_check(n, lambdas, v_rot, limb_darkening))) return rc;
    const double pair[2] = {v_rot, limb_darkening};
    double* const outs[2] = {out, out_reference};
    return stage_forward_host(
        ctx,
        [](sdx_ctx* c, int64_t m, const double* l, const double* f, const double* r, const double* rot, double* const* o) {
            return sdx_rotate_dev(c, m, l, f, r, rot, o[0], o[1]);
        },
        n, lambdas, flux, reference, pair, 2, outs, 2);
}

int sdx_rotate_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, double v_rot, double limb_darkening, const double* u,
                           const double* u_reference, const double* nus, double* w, double* w_reference)
{
    REQUIRE(ctx, "rotate_adjoint: null context");
    REQUIRE(n >= 2, "rotate_adjoint: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && u && w, "rotate_adjoint: null pointer (lambdas, u and w are required)");
    REQUIRE(!u_reference == !w_reference, "rotate_adjoint: u_reference and w_reference go together");
    int rc;
    if ((rc = rotate_host_check(n, lambdas, v_rot, limb_darkening))) return rc;
    const double pair[2] = {v_rot, limb_darkening};
    return stage_adjoint_host(ctx, sdx_rotate_adjoint_dev, n, lambdas, pair, 2, u, u_reference, nus, w, w_reference);
}

// ---- rotation with its derivative to the limb-darkening coefficient (k_rotate_tangent: k_rotate's body with the derivative flag) ----
static int rotate_tangent_check(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, const double* out,
                                const double* out_reference, const double* dout_eps, const double* dout_eps_reference)
{
    REQUIRE(ctx, "rotate_tangent: null context");
    REQUIRE(n >= 2, "rotate_tangent: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && flux && out && dout_eps, "rotate_tangent: null pointer (lambdas, flux, out and dout_eps are required)");
    REQUIRE(!reference == !out_reference, "rotate_tangent: reference and out_reference go together");
    REQUIRE(!dout_eps_reference || reference, "rotate_tangent: dout_eps_reference needs a reference");
    const double* const ins[3] = {lambdas, flux, reference};
    const double* const outs[4] = {out, out_reference, dout_eps, dout_eps_reference};
    return distinct_buffers("rotate_tangent", ins, 3, outs, 4);
}

int sdx_rotate_tangent_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, const double* rot_dev,
                           double* out, double* out_reference, double* dout_eps, double* dout_eps_reference)
{
    int rc;
    if ((rc = rotate_tangent_check(ctx, n, lambdas, flux, reference, out, out_reference, dout_eps, dout_eps_reference))) return rc;
    REQUIRE(rot_dev, "rotate_tangent: null pointer (rot_dev is required)");
    REQUIRE((n + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31), "rotate_tangent: too many points for one launch");
    HIP_TRY(hipSetDevice(ctx->device));
    {
        LaunchScope ls(ctx, "k_rotate_tangent");
        hipLaunchKernelGGL(k_rotate_tangent, dim3(rotate_blocks(n)), dim3(kBlock), 0, ctx->stream, n, lambdas, flux, reference, rot_dev, out,
                           out_reference, dout_eps, dout_eps_reference);
    }
    return check_launch("k_rotate_tangent");
}

int sdx_rotate_tangent_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, double v_rot,
                           double limb_darkening, double* out, double* out_reference, double* dout_eps, double* dout_eps_reference)
{
    int rc;
    if ((rc = rotate_tangent_check(ctx, n, lambdas, flux, reference, out, out_reference, dout_eps, dout_eps_reference))) return rc;
    if ((rc = rotate_host_check(n, lambdas, v_rot, limb_darkening))) return rc;
    const double pair[2] = {v_rot, limb_darkening};
    double* const outs[4] = {out, out_reference, dout_eps, dout_eps_reference};
    return stage_forward_host(
        ctx,
        [](sdx_ctx* c, int64_t m, const double* l, const double* f, const double* r, const double* rot, double* const* o) {
            return sdx_rotate_tangent_dev(c, m, l, f, r, rot, o[0], o[1], o[2], o[3]);
        },
        n, lambdas, flux, reference, pair, 2, outs, 4);
}

// ---- the cell-integrated rotation profile (k_rotate_integrated), its adjoint and the moments' test entry ------------------------------
static int rotate_integrated_check(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, const double* out,
                                   const double* out_reference, const double* dout_lnv, const double* dout_lnv_reference,
                                   const double* dout_eps, const double* dout_eps_reference)
{
    REQUIRE(ctx, "rotate_integrated: null context");
    REQUIRE(n >= 2, "rotate_integrated: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && flux && out, "rotate_integrated: null pointer (lambdas, flux and out are required)");
    REQUIRE(!reference == !out_reference, "rotate_integrated: reference and out_reference go together");
    REQUIRE((!dout_lnv_reference && !dout_eps_reference) || reference,
            "rotate_integrated: dout_lnv_reference and dout_eps_reference need a reference");
    const double* const ins[3] = {lambdas, flux, reference};
    const double* const outs[6] = {out, out_reference, dout_lnv, dout_lnv_reference, dout_eps, dout_eps_reference};
    return distinct_buffers("rotate_integrated", ins, 3, outs, 6);
}

int sdx_rotate_integrated_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference,
                              const double* rot_dev, double* out, double* out_reference, double* dout_lnv, double* dout_lnv_reference,
                              double* dout_eps, double* dout_eps_reference)
{
    int rc;
    if ((rc = rotate_integrated_check(ctx, n, lambdas, flux, reference, out, out_reference, dout_lnv, dout_lnv_reference, dout_eps,
                                      dout_eps_reference)))
        return rc;
    REQUIRE(rot_dev, "rotate_integrated: null pointer (rot_dev is required)");
    REQUIRE((n + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31), "rotate_integrated: too many points for one launch");
    HIP_TRY(hipSetDevice(ctx->device));
    {
        LaunchScope ls(ctx, "k_rotate_integrated");
        if (dout_lnv || dout_lnv_reference || dout_eps || dout_eps_reference)
            hipLaunchKernelGGL(k_rotate_integrated<true>, dim3(rotate_blocks(n)), dim3(kBlock), 0, ctx->stream, n, lambdas, flux, reference, rot_dev,
                               out, out_reference, dout_lnv, dout_lnv_reference, dout_eps, dout_eps_reference);
        else
            hipLaunchKernelGGL(k_rotate_integrated<false>, dim3(rotate_blocks(n)), dim3(kBlock), 0, ctx->stream, n, lambdas, flux, reference, rot_dev,
                               out, out_reference, (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr);
    }
    return check_launch("k_rotate_integrated");
}

int sdx_rotate_integrated_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* rot_dev, const double* u,
                                      const double* u_reference, const double* nus, double* w, double* w_reference)
{
    return stage_adjoint(ctx, "k_rotate_integrated_adjoint", "rot_dev", k_rotate_integrated_adjoint_den, k_rotate_integrated_adjoint, n, lambdas,
                         rot_dev, u, u_reference, nus, w, w_reference);
}

int sdx_rotate_integrated_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, double v_rot,
                              double limb_darkening, double* out, double* out_reference, double* dout_lnv, double* dout_lnv_reference,
                              double* dout_eps, double* dout_eps_reference)
{
    int rc;
    if ((rc = rotate_integrated_check(ctx, n, lambdas, flux, reference, out, out_reference, dout_lnv, dout_lnv_reference, dout_eps,
                                      dout_eps_reference)))
        return rc;
    if ((rc = rotate_host_check(n, lambdas, v_rot, limb_darkening))) return rc;
    const double pair[2] = {v_rot, limb_darkening};
    double* const outs[6] = {out, out_reference, dout_lnv, dout_lnv_reference, dout_eps, dout_eps_reference};
    return stage_forward_host(
        ctx,
        [](sdx_ctx* c, int64_t m, const double* l, const double* f, const double* r, const double* rot, double* const* o) {
            return sdx_rotate_integrated_dev(c, m, l, f, r, rot, o[0], o[1], o[2], o[3], o[4], o[5]);
        },
        n, lambdas, flux, reference, pair, 2, outs, 6);
}

int sdx_rotate_integrated_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, double v_rot, double limb_darkening, const double* u,
                                      const double* u_reference, const double* nus, double* w, double* w_reference)
{
    REQUIRE(ctx, "rotate_integrated_adjoint: null context");
    REQUIRE(n >= 2, "rotate_integrated_adjoint: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && u && w, "rotate_integrated_adjoint: null pointer (lambdas, u and w are required)");
    REQUIRE(!u_reference == !w_reference, "rotate_integrated_adjoint: u_reference and w_reference go together");
    int rc;
    if ((rc = rotate_host_check(n, lambdas, v_rot, limb_darkening))) return rc;
    const double pair[2] = {v_rot, limb_darkening};
    return stage_adjoint_host(ctx, sdx_rotate_integrated_adjoint_dev, n, lambdas, pair, 2, u, u_reference, nus, w, w_reference);
}

// the moments of one cell, point by point (k_rotate_moments): what rot_cell evaluates
int sdx_rotate_moments_dev(sdx_ctx* ctx, int64_t n, const double* ya, const double* yb, const double* eps, double* out_m0, double* out_m1)
{
    REQUIRE(ctx, "rotate_moments: null context");
    REQUIRE(n >= 0 && (n == 0 || (ya && yb && eps && out_m0 && out_m1)), "rotate_moments: bad arguments");
    if (n == 0) return SDX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    {
        LaunchScope ls(ctx, "k_rotate_moments");
        hipLaunchKernelGGL(k_rotate_moments, dim3(blocks1(n)), dim3(kBlock), 0, ctx->stream, n, ya, yb, eps, out_m0, out_m1);
    }
    return check_launch("k_rotate_moments");
}

int sdx_rotate_moments_f64(sdx_ctx* ctx, int64_t n, const double* ya, const double* yb, const double* eps, double* out_m0, double* out_m1)
{
    REQUIRE(ctx, "rotate_moments: null context");
    REQUIRE(n >= 0 && (n == 0 || (ya && yb && eps && out_m0 && out_m1)), "rotate_moments: bad arguments");
    if (n == 0) return SDX_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * sizeof(double);
    const double *d_a, *d_b, *d_e;
    double *d_m0, *d_m1;
    HostPlan plan;
    plan.in(ya, bytes, &d_a);
    plan.in(yb, bytes, &d_b);
    plan.in(eps, bytes, &d_e);
    plan.out(out_m0, bytes, &d_m0);
    plan.out(out_m1, bytes, &d_m1);
    HostIo io{ctx};
    int rc;
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_rotate_moments_dev(ctx, n, d_a, d_b, d_e, d_m0, d_m1))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ---- disk integration with rigid rotation (k_disk_integrate): per-ring spectra, the arcsine density of each ring integrated cell by cell --
static int disk_integrate_check(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale, const double* ring_weights,
                                const double* I, const double* I_reference, const double* rot, const double* out, const double* out_reference)
{
    REQUIRE(ctx, "disk_integrate: null context");
    REQUIRE(n >= 2, "disk_integrate: the grid needs at least two points (n >= 2)");
    REQUIRE(n_rings >= 1 && n_rings <= 64, "disk_integrate: n_rings must lie in 1 .. 64");
    REQUIRE(lambdas && ring_scale && ring_weights && I && out, "disk_integrate: null pointer (lambdas, ring_scale, ring_weights, I and out are required)");
    REQUIRE(!I_reference == !out_reference, "disk_integrate: I_reference and out_reference go together");
    const double* const ins[6] = {lambdas, ring_scale, ring_weights, I, I_reference, rot};
    const double* const outs[2] = {out, out_reference};
    return distinct_buffers("disk_integrate", ins, 6, outs, 2);
}

// deriv: k_disk_integrate<true>, which also writes d out / d ln V (dout_lnv required, dout_lnv_reference optional with a reference)
static int disk_integrate_launch(sdx_ctx* ctx, bool deriv, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                                 const double* ring_weights, const double* I, int64_t I_ld, const double* I_reference, const double* rot_dev,
                                 double* out, double* out_reference, double* dout_lnv, double* dout_lnv_reference)
{
    int rc;
    if ((rc = disk_integrate_check(ctx, n, lambdas, n_rings, ring_scale, ring_weights, I, I_reference, rot_dev, out, out_reference))) return rc;
    REQUIRE(rot_dev, "disk_integrate: null pointer (rot_dev is required)");
    REQUIRE(I_ld >= n, "disk_integrate: I_ld below n");
    if (deriv) {
        REQUIRE(dout_lnv, "disk_integrate: null pointer (dout_lnv is required)");
        REQUIRE(!dout_lnv_reference || I_reference, "disk_integrate: dout_lnv_reference needs I_reference");
        const double* const ins[6] = {lambdas, ring_scale, ring_weights, I, I_reference, rot_dev};
        const double* const outs[4] = {out, out_reference, dout_lnv, dout_lnv_reference};
        if ((rc = distinct_buffers("disk_integrate", ins, 6, outs, 4))) return rc;
    }
    REQUIRE((n + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31), "disk_integrate: too many points for one launch");
    HIP_TRY(hipSetDevice(ctx->device));
    {
        LaunchScope ls(ctx, "k_disk_integrate");
        if (deriv)
            hipLaunchKernelGGL(k_disk_integrate<true>, dim3(rotate_blocks(n)), dim3(kBlock), 0, ctx->stream, n, lambdas, n_rings, ring_scale, ring_weights, I,
                               I_ld, I_reference, rot_dev, out, out_reference, dout_lnv, dout_lnv_reference);
        else
            hipLaunchKernelGGL(k_disk_integrate<false>, dim3(rotate_blocks(n)), dim3(kBlock), 0, ctx->stream, n, lambdas, n_rings, ring_scale, ring_weights, I,
                               I_ld, I_reference, rot_dev, out, out_reference, (double*)nullptr, (double*)nullptr);
    }
    return check_launch("k_disk_integrate");
}

int sdx_disk_integrate_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale, const double* ring_weights,
                           const double* I, int64_t I_ld, const double* I_reference, const double* rot_dev, double* out, double* out_reference)
{
    return disk_integrate_launch(ctx, false, n, lambdas, n_rings, ring_scale, ring_weights, I, I_ld, I_reference, rot_dev, out, out_reference, nullptr,
                                 nullptr);
}

int sdx_disk_integrate_deriv_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale, const double* ring_weights,
                                 const double* I, int64_t I_ld, const double* I_reference, const double* rot_dev, double* out, double* out_reference,
                                 double* dout_lnv, double* dout_lnv_reference)
{
    return disk_integrate_launch(ctx, true, n, lambdas, n_rings, ring_scale, ring_weights, I, I_ld, I_reference, rot_dev, out, out_reference, dout_lnv,
                                 dout_lnv_reference);
}

// what the kernels cannot check: the disk twins do, before any upload
static int disk_host_check(int64_t n, const double* lambdas, int n_rings, const double* ring_scale, double v_rot)
{
    int rc;
    if ((rc = rotate_host_check(n, lambdas, v_rot, 0.0))) return rc;
    for (int r = 0; r < n_rings; ++r) REQUIRE(ring_scale[r] >= 0.0 && ring_scale[r] <= 1.0, "disk_integrate: ring_scale must lie in [0, 1]");
    return SDX_OK;
}

static int disk_integrate_host(sdx_ctx* ctx, bool deriv, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                               const double* ring_weights, const double* I, const double* I_reference, double v_rot, double* out,
                               double* out_reference, double* dout_lnv, double* dout_lnv_reference)
{
    int rc;
    if ((rc = disk_integrate_check(ctx, n, lambdas, n_rings, ring_scale, ring_weights, I, I_reference, nullptr, out, out_reference))) return rc;
    REQUIRE(!deriv || dout_lnv, "disk_integrate: null pointer (dout_lnv is required)");
    REQUIRE(!dout_lnv_reference || I_reference, "disk_integrate: dout_lnv_reference needs I_reference");
    if ((rc = disk_host_check(n, lambdas, n_rings, ring_scale, v_rot))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), grid = (size_t)n * f8, rings = (size_t)n_rings * f8;
    const double pair[2] = {v_rot, 0.0};
    const double *d_l, *d_s, *d_w, *d_i, *d_r, *d_p;
    double *d_o, *d_or, *d_d = nullptr, *d_dr = nullptr;
    HostPlan plan;
    plan.in(lambdas, grid, &d_l);
    plan.in(ring_scale, rings, &d_s);
    plan.in(ring_weights, rings, &d_w);
    plan.in(I, grid * n_rings, &d_i);
    plan.in(I_reference, grid * n_rings, &d_r);
    plan.in(pair, 2 * f8, &d_p);
    plan.out(out, grid, &d_o);
    plan.out(out_reference, grid, &d_or);
    if (deriv) {
        plan.out(dout_lnv, grid, &d_d);
        plan.out(dout_lnv_reference, grid, &d_dr);
    }
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    if ((rc = disk_integrate_launch(ctx, deriv, n, d_l, n_rings, d_s, d_w, d_i, n, d_r, d_p, d_o, d_or, d_d, d_dr))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

int sdx_disk_integrate_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale, const double* ring_weights,
                           const double* I, const double* I_reference, double v_rot, double* out, double* out_reference)
{
    return disk_integrate_host(ctx, false, n, lambdas, n_rings, ring_scale, ring_weights, I, I_reference, v_rot, out, out_reference, nullptr, nullptr);
}

int sdx_disk_integrate_deriv_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale, const double* ring_weights,
                                 const double* I, const double* I_reference, double v_rot, double* out, double* out_reference, double* dout_lnv,
                                 double* dout_lnv_reference)
{
    return disk_integrate_host(ctx, true, n, lambdas, n_rings, ring_scale, ring_weights, I, I_reference, v_rot, out, out_reference, dout_lnv,
                               dout_lnv_reference);
}

// ---- the transpose of the disk integration (k_disk_integrate_adjoint_den, k_disk_integrate_adjoint): the broadening stages' pair per ring
static int disk_adjoint_check(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale, const double* ring_weights,
                              const double* rot, const double* u, const double* u_reference, const double* nus, const double* W,
                              const double* W_reference)
{
    REQUIRE(ctx, "disk_integrate_adjoint: null context");
    REQUIRE(n >= 2, "disk_integrate_adjoint: the grid needs at least two points (n >= 2)");
    REQUIRE(n_rings >= 1 && n_rings <= 64, "disk_integrate_adjoint: n_rings must lie in 1 .. 64");
    REQUIRE(lambdas && ring_scale && ring_weights && u && W, "disk_integrate_adjoint: null pointer (lambdas, ring_scale, ring_weights, u and W are required)");
    REQUIRE(!u_reference == !W_reference, "disk_integrate_adjoint: u_reference and W_reference go together");
    const double* const ins[7] = {lambdas, ring_scale, ring_weights, u, u_reference, nus, rot};
    const double* const outs[2] = {W, W_reference};
    return distinct_buffers("disk_integrate_adjoint", ins, 7, outs, 2);
}

int sdx_disk_integrate_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                                   const double* ring_weights, const double* rot_dev, const double* u, const double* u_reference,
                                   const double* nus, double* W, int64_t W_ld, double* W_reference)
{
    int rc;
    if ((rc = disk_adjoint_check(ctx, n, lambdas, n_rings, ring_scale, ring_weights, rot_dev, u, u_reference, nus, W, W_reference))) return rc;
    REQUIRE(rot_dev, "disk_integrate_adjoint: null pointer (rot_dev is required)");
    REQUIRE(W_ld >= n, "disk_integrate_adjoint: W_ld below n");
    REQUIRE((n + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31), "disk_integrate_adjoint: too many points for one launch");
    HIP_TRY(hipSetDevice(ctx->device));
    // a_r = u / den_r: two blocks of n_rings rows in the stages' scratch (stage_adjoint), consumed between this call's two launches
    const size_t row = ((size_t)n * sizeof(double) + 255) & ~(size_t)255, block = row * (size_t)n_rings;
    if ((rc = ensure(ctx, &ctx->stage_ws, &ctx->stage_ws_bytes, 2 * block))) return rc;
    double* const a = (double*)ctx->stage_ws;
    double* const a_ref = (double*)((char*)ctx->stage_ws + block);
    const int64_t row_doubles = (int64_t)(row / sizeof(double));
    {
        LaunchScope ls(ctx, "k_disk_integrate_adjoint");
        const dim3 grid(rotate_blocks(n), (unsigned)n_rings);
        hipLaunchKernelGGL(k_disk_integrate_adjoint_den, grid, dim3(kBlock), 0, ctx->stream, n, lambdas, ring_scale, ring_weights, rot_dev, u, u_reference, a,
                           a_ref, row_doubles);
        hipLaunchKernelGGL(k_disk_integrate_adjoint, grid, dim3(kBlock), 0, ctx->stream, n, lambdas, ring_scale, ring_weights, rot_dev, (const double*)a,
                           u_reference ? (const double*)a_ref : nullptr, row_doubles, nus, W, W_reference, W_ld);
    }
    return check_launch("k_disk_integrate_adjoint");
}

int sdx_disk_integrate_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, int n_rings, const double* ring_scale,
                                   const double* ring_weights, double v_rot, const double* u, const double* u_reference, const double* nus,
                                   double* W, double* W_reference)
{
    int rc;
    if ((rc = disk_adjoint_check(ctx, n, lambdas, n_rings, ring_scale, ring_weights, nullptr, u, u_reference, nus, W, W_reference))) return rc;
    if ((rc = disk_host_check(n, lambdas, n_rings, ring_scale, v_rot))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t f8 = sizeof(double), grid = (size_t)n * f8, rings = (size_t)n_rings * f8;
    const double pair[2] = {v_rot, 0.0};
    const double *d_l, *d_s, *d_w, *d_p, *d_u, *d_ur, *d_nus;
    double *d_W, *d_Wr;
    HostPlan plan;
    plan.in(lambdas, grid, &d_l);
    plan.in(ring_scale, rings, &d_s);
    plan.in(ring_weights, rings, &d_w);
    plan.in(pair, 2 * f8, &d_p);
    plan.in(u, grid, &d_u);
    plan.in(u_reference, grid, &d_ur);
    plan.in(nus, grid, &d_nus);
    plan.out(W, grid * n_rings, &d_W);
    plan.out(W_reference, grid * n_rings, &d_Wr);
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    if ((rc = sdx_disk_integrate_adjoint_dev(ctx, n, d_l, n_rings, d_s, d_w, d_p, d_u, d_ur, d_nus, d_W, n, d_Wr))) return rc;
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ---- radial-tangential macroturbulence (k_macroturbulence) and its adjoint -------------------------------------------------------------
int sdx_macroturbulence_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, const double* mac_dev,
                            double* out, double* out_reference, double* dout, double* dout_reference)
{
    REQUIRE(ctx, "macroturbulence: null context");
    REQUIRE(n >= 2, "macroturbulence: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && flux && mac_dev && out, "macroturbulence: null pointer (lambdas, flux, mac_dev and out are required)");
    REQUIRE(!reference == !out_reference, "macroturbulence: reference and out_reference go together");
    REQUIRE(!dout_reference || reference, "macroturbulence: dout_reference needs a reference");
    const double* const ins[4] = {lambdas, flux, reference, mac_dev};
    const double* const outs[4] = {out, out_reference, dout, dout_reference};
    int rc;
    if ((rc = distinct_buffers("macroturbulence", ins, 4, outs, 4,
                               ": not in place (out, out_reference, dout and dout_reference must be buffers of their own)")))
        return rc;
    REQUIRE((n + kObsGroup - 1) / (kBlock / 64) < ((int64_t)1 << 31), "macroturbulence: too many points for one launch");
    HIP_TRY(hipSetDevice(ctx->device));
    {
        LaunchScope ls(ctx, "k_macroturbulence");
        hipLaunchKernelGGL(k_macroturbulence, dim3(rotate_blocks(n)), dim3(kBlock), 0, ctx->stream, n, lambdas, flux, reference, mac_dev, out,
                           out_reference, dout, dout_reference);
    }
    return check_launch("k_macroturbulence");
}

// (this adjoint alone refuses outputs that alias its inputs; the rotation adjoints never did)
int sdx_macroturbulence_adjoint_dev(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* mac_dev, const double* u,
                                    const double* u_reference, const double* nus, double* w, double* w_reference)
{
    const double* const ins[5] = {lambdas, mac_dev, u, u_reference, nus};
    const double* const outs[2] = {w, w_reference};
    int rc;
    if ((rc = distinct_buffers("macroturbulence_adjoint", ins, 5, outs, 2, ": not in place (w and w_reference must be buffers of their own)")))
        return rc;
    return stage_adjoint(ctx, "k_macroturbulence_adjoint", "mac_dev", k_macroturbulence_adjoint_den, k_macroturbulence_adjoint, n, lambdas, mac_dev,
                         u, u_reference, nus, w, w_reference);
}

// what the kernels cannot check: the host-buffer twins do, before any upload
static int macroturbulence_host_check(int64_t n, const double* lambdas, double zeta)
{
    REQUIRE(std::isfinite(zeta) && zeta >= 0.0 && zeta < 500.0, "macroturbulence: zeta must be finite with 0 <= zeta < 500 km/s");
    return ascending_check("macroturbulence", "lambdas", n, lambdas);
}

int sdx_macroturbulence_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, const double* flux, const double* reference, double zeta,
                            double* out, double* out_reference, double* dout, double* dout_reference)
{
    REQUIRE(ctx, "macroturbulence: null context");
    REQUIRE(n >= 2, "macroturbulence: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && flux && out, "macroturbulence: null pointer (lambdas, flux and out are required)");
    REQUIRE(!reference == !out_reference, "macroturbulence: reference and out_reference go together");
    REQUIRE(!dout_reference || reference, "macroturbulence: dout_reference needs a reference");
    int rc;
    if ((rc = macroturbulence_host_check(n, lambdas, zeta))) return rc;
    double* const outs[4] = {out, out_reference, dout, dout_reference};
    return stage_forward_host(
        ctx,
        [](sdx_ctx* c, int64_t m, const double* l, const double* f, const double* r, const double* mac, double* const* o) {
            return sdx_macroturbulence_dev(c, m, l, f, r, mac, o[0], o[1], o[2], o[3]);
        },
        n, lambdas, flux, reference, &zeta, 1, outs, 4);
}

int sdx_macroturbulence_adjoint_f64(sdx_ctx* ctx, int64_t n, const double* lambdas, double zeta, const double* u, const double* u_reference,
                                    const double* nus, double* w, double* w_reference)
{
    REQUIRE(ctx, "macroturbulence_adjoint: null context");
    REQUIRE(n >= 2, "macroturbulence_adjoint: the grid needs at least two points (n >= 2)");
    REQUIRE(lambdas && u && w, "macroturbulence_adjoint: null pointer (lambdas, u and w are required)");
    REQUIRE(!u_reference == !w_reference, "macroturbulence_adjoint: u_reference and w_reference go together");
    int rc;
    if ((rc = macroturbulence_host_check(n, lambdas, zeta))) return rc;
    return stage_adjoint_host(ctx, sdx_macroturbulence_adjoint_dev, n, lambdas, &zeta, 1, u, u_reference, nus, w, w_reference);
}

// ================================================================================================ fused synthesis
// the planes a synthesis writes ([n_depth][ld], the shard's columns) and the optional ones it reads.  synthesize_impl: device pointers.
// synthesize_host_shard reads the three output planes and n_evaluations alone, as HOST pointers: whole-grid planes [n_depth][n_nu]
// (ld = n_nu) of which it fills the shard's columns
struct SynthPlanes {
    double *alpha_line_out, *total_alphas, *F_nu;
    int64_t ld;
    int64_t* n_evaluations;
    double* I_nus;
    const double* source;
    int64_t source_ld;
};
static int synthesize_impl(sdx_ctx* ctx, const Grid& g, const Lines& lines, const sdx_continuum* cont, const Rays& rays, const SynthPlanes& io,
                           const sdx_synthesis_options* opt)
{
    int rc;
    const int n_depth = g.n_depth, n_theta = rays.n_theta;
    const int64_t n_nu = g.n_nu, nu_begin = g.nu_begin, nu_count = g.nu_count, n_lines = lines.n_lines, ld = io.ld;
    double *const alpha_line_out = io.alpha_line_out, *const total_alphas = io.total_alphas, *const F_nu = io.F_nu;
    REQUIRE(cont && rays.temps && rays.ray_dist && rays.wts && n_theta > 0 && n_depth >= 2, "synthesize: bad arguments");
    REQUIRE(nu_begin >= 0 && nu_count >= 0 && nu_begin + nu_count <= n_nu, "synthesize: shard outside the grid");
    REQUIRE(nu_count == 0 || (F_nu && ld >= nu_count), "synthesize: bad output buffers");
    if ((rc = check_file_planes(cont, n_nu))) return rc;
    const int inward = opt && opt->inward_rays ? 1 : 0;
    const int n_extra = opt ? opt->n_line_planes : 0;
    REQUIRE(n_extra >= 0 && n_extra <= 2, "synthesize: n_line_planes must be 0..2");
    // (a plan is for dense lists: the generating pre-pass ignores it, and so do culled shards and the two-collective mode)
    const sdx_grid_plan* const plan = opt && !lines.gen ? opt->grid_plan : nullptr;
    if (plan && (rc = check_grid_plan(ctx, plan, g, lines, cont))) return rc;
    double* const Fc = opt ? opt->F_nu_continuum : nullptr;
    REQUIRE(!Fc || opt->continuum_ld >= nu_count, "synthesize: continuum_ld must cover the columns");
    for (int k = 0; k < n_extra; ++k) REQUIRE(opt->line_plane[k] && opt->line_plane_ld >= nu_count, "synthesize: bad line plane");
    // the formal solution forms total = continuum + line planes while staging its columns when those fit LDS
    // (k_raytrace at G = 64: one frequency per wave and the flux terms of 64 lanes, the worst case whatever n_theta is)
    const bool fuse = n_theta <= 64 && rt_fit_gpw<RtColumns>(64, n_depth) > 0;
    // a continuum request that cannot be served is refused here, before anything is enqueued (k_raytrace_cont, also at G = 64:
    // deliberately the conservative limit, not the layout at this n_theta)
    REQUIRE(!Fc || !ctx->mixed_precision, "synthesize: no continuum flux with mixed_precision = 1 (the fp32 formal solution has no continuum chain)");
    REQUIRE(!Fc || fuse, "synthesize: the continuum flux needs the fused total (n_theta <= 64 and the model's columns in LDS)");
    REQUIRE(!Fc || rt_fit_gpw<RtContColumns>(64, n_depth) > 0, "synthesize: no continuum flux for models this deep (the columns do not fit LDS)");
    if (nu_count == 0) return SDX_OK;
    // Three launches on one stream: [pre-pass + continuum plane] -> [wide + narrow line kernels] -> [raytrace, which
    // forms total = continuum + line while staging its columns].  Independent work shares a launch instead of a
    // second stream: inter-queue edges cost ~12 us each on this platform, a whole kernel's worth at this size.
    int rc2 = ensure(ctx, &ctx->cont_ws, &ctx->cont_ws_bytes, (size_t)n_depth * nu_count * sizeof(double));
    if (rc2) return rc2;
    double* cont_plane = (double*)ctx->cont_ws;
    // spherical geometry (opt->inward_rays): the inward sweep before the outward one, then F_nu *= (r[-1] / reference_r)^2
    // (radiation_field_solvers/base.py:141-198, :340-344)
    auto finish = [&](int rc_trace) -> int {
        if (rc_trace || !inward) return rc_trace;
        return scale_flux(ctx, n_depth, nu_count, F_nu, ld, opt->photospheric_correction, Fc, Fc ? opt->continuum_ld : 0);
    };
    LinePlanes p{};  // (no lines: no planes)
    // two-collective mode: the classification launch ran already (sdx_synthesize_classify_dev), the per-line maxima were gathered
    const ClassifyPhase second{2, 0, 0, opt ? const_cast<double*>(opt->line_m_max) : nullptr};
    REQUIRE(!second.m_max || (n_lines > 0 && !lines.gen), "synthesize: options->line_m_max goes with a dense line list");
    if (!second.m_max) ctx->classified.valid = false;  // (this step rewrites the continuum plane a phase 1 left behind)
    if (n_lines > 0) {
        PrepassRequest req{};
        req.count_evals = io.n_evaluations != nullptr, req.cont = cont, req.cont_plane = cont_plane, req.ph = second.m_max ? &second : nullptr, req.plan = plan;
        if ((rc = line_partials(ctx, g, lines, req, &p))) return rc;
        if (io.n_evaluations)
            HIP_TRY(hipMemcpyAsync(io.n_evaluations, p.w.evals, sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        rc = launch_total(ctx, g, cont, nullptr, 0, cont_plane, nu_count);
        if (rc) return rc;
        if (io.n_evaluations) HIP_TRY(hipMemsetAsync(io.n_evaluations, 0, sizeof(int64_t), ctx->stream));  // (an empty list evaluates nothing)
        if (alpha_line_out)
            HIP_TRY(hipMemset2DAsync(alpha_line_out, ld * sizeof(double), 0, nu_count * sizeof(double), n_depth, ctx->stream));
    }
    if (!fuse) {
        // total = continuum (+ line planes), element-wise; without a caller buffer the continuum plane becomes the total in place
        double* total = total_alphas ? total_alphas : cont_plane;
        const int64_t tld = total_alphas ? ld : nu_count;
        {
            LaunchScope ls(ctx, "k_reduce_partials");
            if (total_alphas)
                HIP_TRY(hipMemcpy2DAsync(total_alphas, ld * sizeof(double), cont_plane, nu_count * sizeof(double), nu_count * sizeof(double),
                                         n_depth, hipMemcpyDeviceToDevice, ctx->stream));
            if (p.part) {
                if (alpha_line_out)
                    hipLaunchKernelGGL(k_reduce_partials, grid2(nu_count, n_depth), dim3(kBlock), 0, ctx->stream, n_depth, nu_count,
                                       p.n_planes, p.part, p.pld, alpha_line_out, ld, 0);
                hipLaunchKernelGGL(k_reduce_partials, grid2(nu_count, n_depth), dim3(kBlock), 0, ctx->stream, n_depth, nu_count, p.n_planes,
                                   p.part, p.pld, total, tld, 1);
            }
        }
        rc = check_launch("k_reduce_partials");
        if (rc) return rc;
        for (int k = 0; k < n_extra; ++k)
            if ((rc = sdx_accumulate_dev(ctx, n_depth, nu_count, total, tld, opt->line_plane[k], opt->line_plane_ld))) return rc;
        FusedTotal only_source{};  // (no fused total: the formal solution reads `total`; the caller's source plane still applies)
        only_source.source = io.source;
        only_source.sld = io.source_ld;
        return finish(raytrace_impl(ctx, g, rays, RtPlanes{total, tld, F_nu, ld, io.I_nus, 0, inward, io.source ? &only_source : nullptr, nullptr, 0}));
    }
    FusedTotal ft{};
    ft.source = io.source;
    ft.sld = io.source_ld;
    ft.cont = cont_plane;
    ft.cld = nu_count;
    ft.planes = p.part;
    ft.n_planes = p.n_planes;
    ft.pld = p.pld;
    ft.total_out = total_alphas;
    ft.line_out = p.part ? alpha_line_out : nullptr;
    ft.out_ld = ld;
    ft.n_extra = n_extra;
    for (int k = 0; k < n_extra; ++k) ft.extra[k] = opt->line_plane[k];
    ft.eld = n_extra ? opt->line_plane_ld : 0;
    return finish(raytrace_impl(ctx, g, rays, RtPlanes{nullptr, 0, F_nu, ld, io.I_nus, 0, inward, &ft, Fc, Fc ? opt->continuum_ld : 0}));
}

int sdx_synthesize_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                       int64_t n_lines, const double* line_nus, const double* doppler, const double* gammas, int gamma_cols,
                       const double* alphas, const sdx_continuum* cont, int n_theta, const double* temps,
                       const double* ray_dist, const double* wts, double* alpha_line_out, double* total_alphas, double* F_nu,
                       int64_t ld, int64_t* n_evaluations_dev)
{
    return sdx_synthesize_ex_dev(ctx, n_depth, n_nu, nus, nu_begin, nu_count, n_lines, line_nus, doppler, gammas, gamma_cols, alphas, cont, n_theta, temps, ray_dist,
                                 wts, alpha_line_out, total_alphas, F_nu, ld, nullptr, 0, nullptr, n_evaluations_dev);  // (no source plane, no intensities)
}

int sdx_synthesize_ex_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                          int64_t n_lines, const double* line_nus, const double* doppler, const double* gammas, int gamma_cols,
                          const double* alphas, const sdx_continuum* cont, int n_theta, const double* temps,
                          const double* ray_dist, const double* wts, double* alpha_line_out, double* total_alphas, double* F_nu,
                          int64_t ld, const double* source, int64_t source_ld, double* I_nus, int64_t* n_evaluations_dev)
{
    int rc = check_line_args(ctx, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas);
    if (rc) return rc;
    REQUIRE(!source || source_ld >= nu_count, "synthesize_ex: source_ld must cover the columns");
    return synthesize_impl(ctx, Grid{n_depth, n_nu, nus, nu_begin, nu_count}, Lines{n_lines, line_nus, doppler, gammas, gamma_cols, alphas, nullptr}, cont,
                           Rays{n_theta, temps, ray_dist, wts}, SynthPlanes{alpha_line_out, total_alphas, F_nu, ld, n_evaluations_dev, I_nus, source, source_ld}, nullptr);
}

int sdx_synthesize_linelist_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                                const sdx_linelist* ll, const sdx_continuum* cont, int n_theta, const double* temps,
                                const double* ray_dist, const double* wts, double* alpha_line_out, double* total_alphas,
                                double* F_nu, int64_t ld, int64_t* n_evaluations_dev)
{
    REQUIRE(ctx, "null context");
    REQUIRE(n_depth > 0 && n_nu >= 0 && n_nu < (int64_t)2147483647, "synthesize: bad sizes");
    REQUIRE(n_nu == 0 || nus, "synthesize: null frequency grid");
    LineParams lp{};
    Lines lines;
    int rc = to_line_params(ll, n_depth, &lp, &lines);
    if (rc) return rc;
    return synthesize_impl(ctx, Grid{n_depth, n_nu, nus, nu_begin, nu_count}, lines, cont, Rays{n_theta, temps, ray_dist, wts},
                           SynthPlanes{alpha_line_out, total_alphas, F_nu, ld, n_evaluations_dev, nullptr, nullptr, 0}, nullptr);
}

int sdx_synthesize_opt_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count,
                           int64_t n_lines, const double* line_nus, const double* doppler, const double* gammas, int gamma_cols,
                           const double* alphas, const sdx_continuum* cont, int n_theta, const double* temps,
                           const double* ray_dist, const double* wts, double* alpha_line_out, double* total_alphas, double* F_nu,
                           int64_t ld, const sdx_synthesis_options* opt, int64_t* n_evaluations_dev)
{
    REQUIRE(ctx && opt, "synthesize_opt: null context or options");
    REQUIRE(!opt->source || opt->source_ld >= nu_count, "synthesize_opt: source_ld must cover the columns");
    LineParams lp{};
    Lines lines{n_lines, line_nus, doppler, gammas, gamma_cols, alphas, nullptr};
    int rc;
    if (opt->linelist) {  // line parameters generated in the pre-pass (f1): the dense arrays are not read
        REQUIRE(n_depth > 0 && n_nu >= 0 && n_nu < (int64_t)2147483647 && (n_nu == 0 || nus), "synthesize_opt: bad sizes");
        rc = to_line_params(opt->linelist, n_depth, &lp, &lines);
    } else {
        rc = check_line_args(ctx, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas);
    }
    if (rc) return rc;
    return synthesize_impl(ctx, Grid{n_depth, n_nu, nus, nu_begin, nu_count}, lines, cont, Rays{n_theta, temps, ray_dist, wts},
                           SynthPlanes{alpha_line_out, total_alphas, F_nu, ld, n_evaluations_dev, opt->I_nus, opt->source, opt->source_ld}, opt);
}

// Phase 1 of the two-collective mode (include/stardis_hip.h): the classification launch of a culled shard's step on a SHARE of the
// lines.  Everything else that launch does for the step — the grid-spacing partials, the shard's line ranges, the continuum plane —
// stays in the context's scratch for the synthesis that follows with options->line_m_max.
int sdx_synthesize_classify_dev(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t nu_begin, int64_t nu_count, int64_t n_lines,
                                const double* line_nus, const double* doppler, const double* gammas, int gamma_cols, const double* alphas,
                                const sdx_continuum* cont, int64_t line_begin, int64_t line_count, double* m_max)
{
    int rc = check_line_args(ctx, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas);
    if (rc) return rc;
    REQUIRE(cont && m_max && n_lines > 0, "classify: null pointer or empty line list");
    REQUIRE(nu_begin >= 0 && nu_count > 0 && nu_begin + nu_count <= n_nu, "classify: shard outside the grid");
    REQUIRE(line_begin >= 0 && line_count >= 0 && line_begin + line_count <= n_lines, "classify: line share outside the list");
    if ((rc = check_file_planes(cont, n_nu))) return rc;
    if ((rc = ensure(ctx, &ctx->cont_ws, &ctx->cont_ws_bytes, (size_t)n_depth * nu_count * sizeof(double)))) return rc;
    // (the partial planes of the line kernels: reserved here so that the synthesis that follows moves nothing)
    if ((rc = ensure(ctx, &ctx->part_ws, &ctx->part_ws_bytes, (size_t)3 * n_depth * nu_count * sizeof(double)))) return rc;
    const ClassifyPhase first{1, line_begin, line_count, m_max};
    ctx->classified.valid = false;
    const Grid g{n_depth, n_nu, nus, nu_begin, nu_count};
    PrepassRequest req{};
    req.cont = cont, req.cont_plane = (double*)ctx->cont_ws, req.ph = &first;
    if (far_field_on(ctx, n_nu) && (rc = far_request(ctx, g, &req.far))) return rc;
    return line_prepass(ctx, g, Lines{n_lines, line_nus, doppler, gammas, gamma_cols, alphas, nullptr}, req, nullptr);
}

// The fused synthesis for a caller that holds everything in host memory (C, or numpy through ctypes): uploads, runs
// sdx_synthesize_dev, downloads.  `cont` carries HOST pointers here; array lengths follow from the sizes in the struct.
static int synthesize_host_check(sdx_ctx* ctx, const Grid& g, const Lines& l, const sdx_continuum* cont, const Rays& rays)
{
    int rc = check_line_args(ctx, g.n_depth, g.n_nu, g.nus, l.n_lines, l.line_nus, l.doppler, l.gammas, l.gamma_cols, l.alphas);
    if (rc) return rc;
    REQUIRE(cont && rays.temps && rays.ray_dist && rays.wts && rays.n_theta > 0 && g.n_depth >= 2, "synthesize: bad arguments");
    if ((rc = host_grid_check(g.n_nu, g.nus))) return rc;
    if ((rc = host_lines_check(l.n_lines, l.line_nus, l.doppler, g.n_depth))) return rc;
    REQUIRE(cont->bf_n_species == 0 || !cont->bf_cutoff || cont->bf_n_levels > 0, "synthesize: bf_n_levels must be set");
    REQUIRE(cont->n_file_planes == 0, "synthesize: file planes are device planes (sdx_synthesize_dev); the host-buffer entry points take tabulated sources as the 1-D table only");
    return SDX_OK;
}

// the continuum's rows (HOST pointers in *cont, device pointers into *c; a null one is absent), in the order both callers upload them;
// `temperature` is not among them: the synthesis points it at the rays' temperatures, sdx_continuum_f64 uploads it behind these
static void continuum_uploads(const sdx_continuum* cont, sdx_continuum* c, int n_depth, int64_t n_nu, int n_levels, HostPlan* plan)
{
    const size_t f8 = sizeof(double), i4 = sizeof(int32_t), depth = (size_t)n_depth * f8;
    plan->in(cont->lambdas, (size_t)n_nu * f8, &c->lambdas);
    plan->in(cont->table_wavelength, (size_t)c->n_table * f8, &c->table_wavelength);
    plan->in(cont->table_sigma, (size_t)c->n_table * f8, &c->table_sigma);
    plan->in(cont->table_density, depth, &c->table_density);
    plan->in(cont->bf_species_offsets, (size_t)(c->bf_n_species + 1) * i4, &c->bf_species_offsets);
    plan->in(cont->bf_species_ion_number, (size_t)c->bf_n_species * i4, &c->bf_species_ion_number);
    plan->in(cont->bf_cutoff, (size_t)n_levels * f8, &c->bf_cutoff);
    plan->in(cont->bf_level_density, (size_t)n_levels * depth, &c->bf_level_density);
    plan->in(cont->ff_species_ion_number, (size_t)c->ff_n_species * i4, &c->ff_species_ion_number);
    plan->in(cont->ff_number_density, (size_t)c->ff_n_species * depth, &c->ff_number_density);
    plan->in(cont->ray_n_h, depth, &c->ray_n_h);
    plan->in(cont->ray_n_he, depth, &c->ray_n_he);
    plan->in(cont->ray_n_h2, depth, &c->ray_n_h2);
    plan->in(cont->electron_density, depth, &c->electron_density);
}

// Uploads everything to ctx's device, enqueues the synthesis of columns [nu_begin, nu_begin + nu_count) and the downloads of the
// requested planes into the caller's [n_depth][n_nu] host arrays (the shard's columns only).  `io` stays alive until the caller
// has called io.finish(); *d_F_out is the shard's device flux plane [n_depth][nu_count] (valid until the next call on ctx).
static int synthesize_host_shard(sdx_ctx* ctx, HostIo& io, const Grid& g, const Lines& l, const sdx_continuum* cont, const Rays& rays, const SynthPlanes& out,
                                 double** d_F_out)
{
    int rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int n_depth = g.n_depth, n_theta = rays.n_theta;
    const int64_t n_nu = g.n_nu, nu_begin = g.nu_begin, nu_count = g.nu_count, n_lines = l.n_lines;
    double *const alpha_line_out = out.alpha_line_out, *const total_alphas = out.total_alphas, *const F_nu = out.F_nu;
    const size_t f8 = sizeof(double), plane = (size_t)n_depth * nu_count * f8, ld = (size_t)n_lines * n_depth * f8;
    sdx_continuum c = *cont;
    const double *d_nus, *d_ln, *d_dw, *d_g, *d_a, *d_t, *d_rd, *d_w;
    double *d_line, *d_total, *d_F;
    int64_t* d_ev;
    const size_t pitch = (size_t)n_nu * f8, row = (size_t)nu_count * f8;
    HostPlan plan;
    plan.in(g.nus, (size_t)n_nu * f8, &d_nus);
    plan.in(l.line_nus, (size_t)n_lines * f8, &d_ln);
    plan.in(l.doppler, ld, &d_dw);
    plan.in(l.gammas, (size_t)n_lines * l.gamma_cols * f8, &d_g);
    plan.in(l.alphas, ld, &d_a);
    plan.in(rays.temps, (size_t)n_depth * f8, &d_t);
    plan.in(rays.ray_dist, (size_t)(n_depth - 1) * n_theta * f8, &d_rd);
    plan.in(rays.wts, (size_t)n_theta * f8, &d_w);
    continuum_uploads(cont, &c, n_depth, n_nu, c.bf_n_species > 0 ? c.bf_n_levels : 0, &plan);
    plan.out2d(alpha_line_out ? alpha_line_out + nu_begin : nullptr, pitch, row, n_depth, &d_line);
    plan.out2d(total_alphas ? total_alphas + nu_begin : nullptr, pitch, row, n_depth, &d_total);
    if (F_nu)
        plan.out2d(F_nu + nu_begin, pitch, row, n_depth, &d_F);
    else
        plan.scratch(plane, &d_F);  // (the sharded entry gathers its last row on the device)
    plan.out(out.n_evaluations, sizeof(int64_t), &d_ev);
    if ((rc = io.stage(plan))) return rc;
    c.temperature = d_t;
    rc = sdx_synthesize_dev(ctx, n_depth, n_nu, d_nus, nu_begin, nu_count, n_lines, d_ln, d_dw, d_g, l.gamma_cols, d_a, &c, n_theta, d_t, d_rd, d_w,
                            d_line, d_total, d_F, nu_count, d_ev);
    if (rc) return rc;
    if ((rc = io.collect(plan))) return rc;
    if (d_F_out) *d_F_out = d_F;
    return SDX_OK;
}

int sdx_synthesize_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                       const double* doppler, const double* gammas, int gamma_cols, const double* alphas, const sdx_continuum* cont,
                       int n_theta, const double* temps, const double* ray_dist, const double* wts, double* alpha_line_out,
                       double* total_alphas, double* F_nu, int64_t* n_evaluations)
{
    const Grid g{n_depth, n_nu, nus, 0, n_nu};
    const Lines lines{n_lines, line_nus, doppler, gammas, gamma_cols, alphas, nullptr};
    const Rays rays{n_theta, temps, ray_dist, wts};
    int rc = synthesize_host_check(ctx, g, lines, cont, rays);
    if (rc) return rc;
    REQUIRE(n_nu == 0 || F_nu, "synthesize: null output");
    if (n_nu == 0) return SDX_OK;
    HostIo io{ctx};
    int64_t ev = 0;
    rc = synthesize_host_shard(ctx, io, g, lines, cont, rays, SynthPlanes{alpha_line_out, total_alphas, F_nu, n_nu, n_evaluations ? &ev : nullptr, nullptr, nullptr, 0}, nullptr);
    if (rc) return rc;
    if ((rc = io.finish())) return rc;
    if (n_evaluations) *n_evaluations = ev;
    return SDX_OK;
}

// The continuum sources for a caller that holds everything in host memory: what calc_alpha_file / _bf / _ff / _rayleigh /
// _electron (opacities_solvers/base.py:40-317) return, and their sum in calc_alphas' order (:655-700), from ONE upload of the
// per-depth vectors and the table — on the context's persistent staging like the other *_f64 entry points.  Each plane is
// produced by the device function the per-source *_dev entry point runs (the same bits); `total` by k_total_alphas.
int sdx_continuum_f64(sdx_ctx* ctx, int n_depth, int64_t n_nu, double* nus, const sdx_continuum* cont, double* alpha_file,
                      double* alpha_bf, double* alpha_ff, double* alpha_rayleigh, double* alpha_electron, double* total_alphas)
{
    REQUIRE(ctx && cont && n_depth > 0 && n_nu >= 0, "continuum: bad arguments");
    REQUIRE(alpha_file || alpha_bf || alpha_ff || alpha_rayleigh || alpha_electron || total_alphas, "continuum: no output requested");
    if (n_nu == 0) return SDX_OK;
    REQUIRE(nus, "continuum: null frequency grid");
    REQUIRE(cont->n_file_planes == 0, "continuum: file planes are device planes; the host-buffer entry point takes the 1-D table only");
    const bool has_table = cont->table_sigma != nullptr, has_bf = cont->bf_cutoff && cont->bf_n_species > 0;
    const bool has_ff = cont->ff_number_density && cont->ff_n_species > 0;
    REQUIRE(!has_table || (cont->lambdas && cont->table_wavelength && cont->table_density && cont->n_table > 0), "continuum: incomplete table source");
    REQUIRE(!has_bf || (cont->bf_n_levels > 0 && cont->bf_n_levels <= 4096 && cont->bf_species_offsets && cont->bf_species_ion_number && cont->bf_level_density),
            "continuum: incomplete bound-free description (bf_n_levels must be set, 1..4096)");
    REQUIRE(!has_ff || (cont->ff_species_ion_number && cont->temperature), "continuum: incomplete free-free description");
    REQUIRE(!alpha_file || has_table, "continuum: alpha_file requested without a table");
    HIP_TRY(hipSetDevice(ctx->device));
    int rc;
    const size_t f8 = sizeof(double), plane = (size_t)n_depth * n_nu * f8;
    sdx_continuum c = *cont;
    const int n_levels = has_bf ? c.bf_n_levels : 0;
    const bool clip = alpha_rayleigh != nullptr;  // calc_alpha_rayleigh zeroes the caller's frequencies above 2.3e15 Hz in place (:99)
    double* d_nus;
    double* const outs[] = {total_alphas, alpha_file, alpha_bf, alpha_ff, alpha_rayleigh, alpha_electron};
    double* d_out[6];
    HostPlan plan;
    plan.inout(nus, (size_t)n_nu * f8, &d_nus, clip);
    continuum_uploads(cont, &c, n_depth, n_nu, n_levels, &plan);
    plan.in(cont->temperature, (size_t)n_depth * f8, &c.temperature);
    for (int k = 0; k < 6; ++k) plan.out(outs[k], plane, &d_out[k]);
    HostIo io{ctx};
    if ((rc = io.stage(plan))) return rc;
    // the total first: it reads the caller's frequencies as they came (the Rayleigh source clips its own copy of a frequency
    // above 2.3e15 Hz, :99, whether or not the array has been clipped yet)
    if (total_alphas && (rc = launch_total(ctx, Grid{n_depth, n_nu, d_nus, 0, n_nu}, &c, nullptr, 0, d_out[0], n_nu))) return rc;
    if (alpha_file && (rc = sdx_alpha_file_1d_dev(ctx, n_depth, n_nu, c.lambdas, c.n_table, c.table_wavelength, c.table_sigma, c.table_density, d_out[1], n_nu)))
        return rc;
    if (alpha_bf) {
        ContinuumArgs a{};
        if (has_bf) {
            double* coef = nullptr;
            if ((rc = launch_bf_coef(ctx, n_depth, c.bf_n_species, n_levels, c.bf_species_offsets, c.bf_species_ion_number, c.bf_cutoff, c.bf_level_density, &coef)))
                return rc;
            a.bf_n_species = c.bf_n_species;
            a.bf_species_offsets = (const int*)c.bf_species_offsets;
            a.bf_species_ion_number = (const int*)c.bf_species_ion_number;
            a.bf_cutoff = c.bf_cutoff;
            a.bf_coef = coef;
        }
        if ((rc = launch_source(ctx, "k_alpha_bf", kSrcBf, n_depth, n_nu, d_nus, a, d_out[2], n_nu))) return rc;
    }
    if (alpha_ff && (rc = sdx_alpha_ff_dev(ctx, n_depth, n_nu, d_nus, c.temperature ? c.temperature : d_nus, has_ff ? c.ff_n_species : 0, c.ff_species_ion_number,
                                           c.ff_number_density, d_out[3], n_nu)))
        return rc;
    if (alpha_rayleigh && (rc = sdx_alpha_rayleigh_dev(ctx, n_depth, n_nu, d_nus, c.ray_n_h, c.ray_n_he, c.ray_n_h2, d_out[4], n_nu))) return rc;
    if (alpha_electron) {
        if (c.electron_density) {
            if ((rc = sdx_alpha_electron_dev(ctx, n_depth, n_nu, c.electron_density, d_out[5], n_nu))) return rc;
        } else {
            HIP_TRY(hipMemsetAsync(d_out[5], 0, plane, ctx->stream));  // (the reference returns the scalar 0 when disabled, :164-165)
        }
    }
    if ((rc = io.collect(plan))) return rc;
    return io.finish();
}

// ---- fp32-mixed twins of the host-buffer entry points (include/stardis_hip.h): the option on for the call, restored afterwards
namespace {
struct MixedScope {
    sdx_ctx* ctx;
    int64_t saved;
    explicit MixedScope(sdx_ctx* c) : ctx(c), saved(c ? c->mixed_precision : 0)
    {
        if (ctx) ctx->mixed_precision = 1;
    }
    ~MixedScope()
    {
        if (ctx) ctx->mixed_precision = saved;
    }
};
}  // namespace

int sdx_line_opacity_f32mix(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                            const double* doppler, const double* gammas, int gamma_cols, const double* alphas, double* out, int64_t* n_evaluations)
{
    REQUIRE(ctx, "null context");
    MixedScope on(ctx);
    return sdx_line_opacity_f64(ctx, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas, out, n_evaluations);
}

int sdx_raytrace_f32mix(sdx_ctx* ctx, int n_depth, int64_t n_nu, int n_theta, const double* nus, const double* temps, const double* ray_dist,
                        const double* wts, const double* alphas, double* F, double* I_nus)
{
    REQUIRE(ctx, "null context");
    MixedScope on(ctx);
    return sdx_raytrace_f64(ctx, n_depth, n_nu, n_theta, nus, temps, ray_dist, wts, alphas, F, I_nus);
}

int sdx_synthesize_f32mix(sdx_ctx* ctx, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus, const double* doppler,
                          const double* gammas, int gamma_cols, const double* alphas, const sdx_continuum* cont, int n_theta, const double* temps,
                          const double* ray_dist, const double* wts, double* alpha_line_out, double* total_alphas, double* F_nu, int64_t* n_evaluations)
{
    REQUIRE(ctx, "null context");
    MixedScope on(ctx);
    return sdx_synthesize_f64(ctx, n_depth, n_nu, nus, n_lines, line_nus, doppler, gammas, gamma_cols, alphas, cont, n_theta, temps, ray_dist, wts,
                              alpha_line_out, total_alphas, F_nu, n_evaluations);
}

}  // extern "C"

// ================================================================================================ one process, several GPUs
// the frequency axis shards with no data-path exchange (radiation_field_solvers/base.py:200 is a prange over
// nu); one process drives one context + stream per device, the line list is replicated, every device keeps the GLOBAL window
// rule, and ONE ncclAllGather (RCCL over xGMI) of the padded F_nu[-1] shards leaves the whole emergent spectrum on every device.
//
// RCCL is opened at run time (dlopen of librccl.so.1, RTLD_LOCAL), not linked: a process that has imported torch already holds
// torch's own copy under the same SONAME and the loader hands that one back — two RCCL builds never meet in one process — and a
// single-GPU user of this library does not map RCCL's half gigabyte of device code.  Every RCCL failure (library missing,
// communicator set-up, the collective itself) is SDX_ERR_COMM.
namespace {
struct RcclApi {
    void* handle = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    std::string error;
};

RcclApi* rccl_api()
{
    static std::mutex m;
    static RcclApi api;
    std::lock_guard<std::mutex> lock(m);
    if (api.handle) return &api;
    // Which RCCL: the one that sits NEXT TO THE HIP RUNTIME THIS LIBRARY IS BOUND TO.  A process may hold two ROCm stacks — the
    // system's and the one a PyTorch wheel bundles (its own libamdhip64 and librccl under torch/lib) — and whichever HIP runtime
    // was loaded first serves everybody; an RCCL from the other stack on top of it fails in ncclCommInitAll ("unhandled cuda
    // error": seen when this library was loaded before torch and "librccl.so.1" then resolved to torch's copy).  An absolute
    // path also keeps the loader from handing back a same-named library that is already mapped.  SDX_RCCL_LIB overrides.
    const char* env = std::getenv("SDX_RCCL_LIB");
    void* h = nullptr;
    std::string tried;
    if (env && *env) {
        h = dlopen(env, RTLD_NOW | RTLD_LOCAL);
        tried = env;
    } else {
        Dl_info info{};
        std::string dir;
        if (dladdr((const void*)&hipGetDeviceCount, &info) && info.dli_fname) {
            dir = info.dli_fname;
            const size_t slash = dir.rfind('/');
            dir = slash == std::string::npos ? std::string() : dir.substr(0, slash + 1);
        }
        const std::string candidates[] = {dir + "librccl.so.1", dir + "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
        for (const std::string& c : candidates) {
            if (c.empty() || (c[0] != '/' && c != "librccl.so.1")) continue;
            h = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
            tried += (tried.empty() ? "" : ", ") + c;
            if (h) break;
        }
    }
    if (!h) {
        const char* e = dlerror();
        api.error = std::string("RCCL not available (tried ") + tried + "): " + (e ? e : "dlopen failed");
        return &api;
    }
    bool ok = true;
    auto sym = [&](const char* name) {
        void* p = dlsym(h, name);
        if (!p) ok = false, api.error = std::string("RCCL symbol missing: ") + name;
        return p;
    };
    api.CommInitAll = (decltype(api.CommInitAll))sym("ncclCommInitAll");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.AllGather = (decltype(api.AllGather))sym("ncclAllGather");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    api.GetVersion = (decltype(api.GetVersion))sym("ncclGetVersion");
    if (!ok) {
        dlclose(h);
        return &api;
    }
    api.handle = h;
    api.error.clear();
    return &api;
}
}  // namespace

struct sdx_group {
    int n = 0;
    std::vector<int> devices;
    std::vector<sdx_ctx*> ctx;
    std::vector<ncclComm_t> comm;  // empty: loop-back test mode (SDX_GROUP_LOOPBACK=1, duplicate devices allowed, no RCCL)
    std::vector<double*> send, recv;  // per device: [per], [per * n]
    size_t per_cap = 0;
    // what the last sdx_synthesize_sharded_f64 did (sdx_group_last_gather)
    int64_t last_bytes_per_rank = 0;
    int last_ranks = 0;
};

#define NCCL_TRY(api, expr)                                                                                     \
    do {                                                                                                        \
        ncclResult_t r_ = (expr);                                                                               \
        if (r_ != ncclSuccess) return fail(SDX_ERR_COMM, std::string(#expr) + ": " + (api)->GetErrorString(r_)); \
    } while (0)

static int group_buffers(sdx_group* g, size_t per)
{
    if (g->per_cap >= per) return SDX_OK;
    for (int r = 0; r < g->n; ++r) {
        HIP_TRY(hipSetDevice(g->devices[r]));
        HIP_TRY(hipStreamSynchronize(g->ctx[r]->stream));
        if (g->send[r]) HIP_TRY(hipFree(g->send[r]));
        if (g->recv[r]) HIP_TRY(hipFree(g->recv[r]));
        g->send[r] = g->recv[r] = nullptr;
        HIP_TRY(hipMalloc((void**)&g->send[r], per * sizeof(double)));
        HIP_TRY(hipMalloc((void**)&g->recv[r], per * g->n * sizeof(double)));
    }
    g->per_cap = per;
    return SDX_OK;
}

extern "C" {

void sdx_group_destroy(sdx_group* g)
{
    if (!g) return;
    RcclApi* api = g->comm.empty() ? nullptr : rccl_api();
    for (int r = 0; r < (int)g->ctx.size(); ++r) {
        if (!g->ctx[r]) continue;
        hipSetDevice(g->devices[r]);
        hipStreamSynchronize(g->ctx[r]->stream);
        if (r < (int)g->send.size() && g->send[r]) hipFree(g->send[r]);
        if (r < (int)g->recv.size() && g->recv[r]) hipFree(g->recv[r]);
    }
    if (api && api->handle)
        for (ncclComm_t c : g->comm)
            if (c) api->CommDestroy(c);
    for (sdx_ctx* c : g->ctx) sdx_destroy(c);
    delete g;
}

sdx_group* sdx_group_create(int n_gpus, const int* devices)
{
    if (n_gpus <= 0 || n_gpus > 64) {
        fail(SDX_ERR_ARG, "sdx_group_create: n_gpus must be 1..64");
        return nullptr;
    }
    const bool loopback = knob("SDX_GROUP_LOOPBACK") && std::atoi(knob("SDX_GROUP_LOOPBACK")) == 1;  // test hook, see header
    // RCCL first: without it there is no group, whatever the devices
    RcclApi* api = loopback ? nullptr : rccl_api();
    if (api && !api->handle) {
        fail(SDX_ERR_COMM, api->error);
        return nullptr;
    }
    const int visible = sdx_device_count();
    std::unique_ptr<sdx_group> g(new sdx_group());
    g->n = n_gpus;
    for (int r = 0; r < n_gpus; ++r) {
        const int dev = devices ? devices[r] : r;
        if (dev < 0 || dev >= visible) {
            fail(SDX_ERR_ARG, "sdx_group_create: device " + std::to_string(dev) + " is not visible (sdx_device_count() = " + std::to_string(visible) + ")");
            return nullptr;
        }
        if (!loopback)
            for (int q = 0; q < r; ++q)
                if (g->devices[q] == dev) {
                    fail(SDX_ERR_ARG, "sdx_group_create: device " + std::to_string(dev) + " listed twice (one RCCL rank per GPU)");
                    return nullptr;
                }
        g->devices.push_back(dev);
    }
    g->send.assign(n_gpus, nullptr);
    g->recv.assign(n_gpus, nullptr);
    for (int r = 0; r < n_gpus; ++r) {
        sdx_ctx* c = sdx_create(g->devices[r], nullptr);
        if (!c) {
            sdx_group_destroy(g.release());
            return nullptr;
        }
        g->ctx.push_back(c);
    }
    if (!loopback) {
        g->comm.assign(n_gpus, nullptr);
        const ncclResult_t r = api->CommInitAll(g->comm.data(), n_gpus, g->devices.data());
        if (r != ncclSuccess) {
            const std::string msg = std::string("ncclCommInitAll: ") + api->GetErrorString(r);
            for (auto& c : g->comm) c = nullptr;
            sdx_group_destroy(g.release());
            fail(SDX_ERR_COMM, msg);
            return nullptr;
        }
    }
    return g.release();
}

int sdx_group_size(const sdx_group* g) { return g ? g->n : 0; }
sdx_ctx* sdx_group_context(sdx_group* g, int rank) { return g && rank >= 0 && rank < g->n ? g->ctx[rank] : nullptr; }

int sdx_group_last_gather(const sdx_group* g, int* ranks, int64_t* bytes_per_rank, int* rccl_version)
{
    REQUIRE(g, "null group");
    if (ranks) *ranks = g->last_ranks;
    if (bytes_per_rank) *bytes_per_rank = g->last_bytes_per_rank;
    if (rccl_version) {
        *rccl_version = 0;
        if (!g->comm.empty()) {
            RcclApi* api = rccl_api();
            if (api->handle) api->GetVersion(rccl_version);
        }
    }
    return SDX_OK;
}

int sdx_synthesize_sharded_f64(sdx_group* g, int n_depth, int64_t n_nu, const double* nus, int64_t n_lines, const double* line_nus,
                               const double* doppler, const double* gammas, int gamma_cols, const double* alphas, const sdx_continuum* cont,
                               int n_theta, const double* temps, const double* ray_dist, const double* wts, const int64_t* shard_begin,
                               double* alpha_line_out, double* total_alphas, double* F_nu, double* emergent_flux, int64_t* n_evaluations)
{
    REQUIRE(g, "null group");
    const int P = g->n;
    const Lines lines{n_lines, line_nus, doppler, gammas, gamma_cols, alphas, nullptr};
    const Rays rays{n_theta, temps, ray_dist, wts};
    int rc = synthesize_host_check(g->ctx[0], Grid{n_depth, n_nu, nus, 0, n_nu}, lines, cont, rays);
    if (rc) return rc;
    REQUIRE(n_nu == 0 || F_nu || emergent_flux, "synthesize_sharded: no output requested");
    if (n_nu == 0) return SDX_OK;
    // shards: contiguous blocks of the GLOBAL frequency index, equal by default
    std::vector<int64_t> begin(P + 1);
    const int64_t per_equal = (n_nu + P - 1) / P;
    for (int r = 0; r <= P; ++r) begin[r] = shard_begin ? shard_begin[r] : std::min<int64_t>((int64_t)r * per_equal, n_nu);
    REQUIRE(begin[0] == 0 && begin[P] == n_nu, "synthesize_sharded: shard_begin must run from 0 to n_nu");
    int64_t per = 0;
    for (int r = 0; r < P; ++r) {
        REQUIRE(begin[r + 1] >= begin[r], "synthesize_sharded: shard_begin must not descend");
        per = std::max(per, begin[r + 1] - begin[r]);
    }
    if ((rc = group_buffers(g, (size_t)per))) return rc;

    // per device, in parallel host threads (the staging memcpy of a replicated 10^6-line list is the slow part): upload,
    // enqueue the shard's synthesis, pack its F_nu[-1] columns into the (zero-padded) send buffer, enqueue the plane downloads
    std::vector<std::unique_ptr<HostIo>> io(P);
    std::vector<int> rcs(P, SDX_OK), codes(P, 0);
    std::vector<std::string> errs(P);
    int64_t ev = 0;
    // the evaluation count (every window of every line: a global figure) is taken from ONE rank — the first that has columns,
    // not blindly rank 0, whose shard may be empty; asking for it switches that rank's culled pre-pass off (it has to see every
    // window), which makes it the straggler of the group: a diagnostic, not something to request in a timed loop
    int ev_rank = -1;
    for (int r = 0; r < P && ev_rank < 0; ++r)
        if (begin[r + 1] > begin[r]) ev_rank = r;
    auto work = [&](int r) {
        sdx_ctx* ctx = g->ctx[r];
        io[r].reset(new HostIo(ctx));
        const int64_t b = begin[r], cnt = begin[r + 1] - begin[r];
        double* d_F = nullptr;
        int rr = SDX_OK;
        if (hipSetDevice(ctx->device) != hipSuccess) rr = fail(SDX_ERR_HIP, "hipSetDevice failed");
        if (!rr && cnt > 0)
            rr = synthesize_host_shard(ctx, *io[r], Grid{n_depth, n_nu, nus, b, cnt}, lines, cont, rays,
                                       SynthPlanes{alpha_line_out, total_alphas, F_nu, n_nu, (r == ev_rank && n_evaluations) ? &ev : nullptr, nullptr, nullptr, 0}, &d_F);
        if (!rr && hipMemsetAsync(g->send[r], 0, (size_t)per * sizeof(double), ctx->stream) != hipSuccess) rr = fail(SDX_ERR_HIP, "hipMemsetAsync(send) failed");
        if (!rr && cnt > 0 &&
            hipMemcpyAsync(g->send[r], d_F + (size_t)(n_depth - 1) * cnt, (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
            rr = fail(SDX_ERR_HIP, "hipMemcpyAsync(pack flux shard) failed");
        rcs[r] = rr;
        if (rr) errs[r] = g_error, codes[r] = g_error_code;
    };
    if (P == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int r = 0; r < P; ++r) th.emplace_back(work, r);
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < P; ++r)
        if (rcs[r]) return fail(rcs[r], "device " + std::to_string(g->devices[r]) + ": " + errs[r]);

    // the one collective: all-gather of the padded emergent-flux shards, stream-ordered behind each device's kernels
    if (!g->comm.empty()) {
        RcclApi* api = rccl_api();
        NCCL_TRY(api, api->GroupStart());
        for (int r = 0; r < P; ++r) {
            const ncclResult_t res = api->AllGather(g->send[r], g->recv[r], (size_t)per, ncclDouble, g->comm[r], g->ctx[r]->stream);
            if (res != ncclSuccess) {
                api->GroupEnd();
                return fail(SDX_ERR_COMM, std::string("ncclAllGather: ") + api->GetErrorString(res));
            }
        }
        NCCL_TRY(api, api->GroupEnd());
    } else {  // loop-back test mode: the same data movement as plain copies after a full synchronisation
        for (int r = 0; r < P; ++r) {
            HIP_TRY(hipSetDevice(g->devices[r]));
            HIP_TRY(hipStreamSynchronize(g->ctx[r]->stream));
        }
        for (int r = 0; r < P; ++r) {
            HIP_TRY(hipSetDevice(g->devices[r]));
            for (int q = 0; q < P; ++q)
                HIP_TRY(hipMemcpyAsync(g->recv[r] + (size_t)q * per, g->send[q], (size_t)per * sizeof(double), hipMemcpyDeviceToDevice, g->ctx[r]->stream));
        }
    }
    g->last_ranks = P;
    g->last_bytes_per_rank = per * (int64_t)sizeof(double);

    // the gathered spectrum comes back from device 0 (every device holds it), padding trimmed
    HIP_TRY(hipSetDevice(g->devices[0]));
    std::vector<double> gathered;
    if (emergent_flux) {
        gathered.resize((size_t)per * P);
        HIP_TRY(hipMemcpyAsync(gathered.data(), g->recv[0], gathered.size() * sizeof(double), hipMemcpyDeviceToHost, g->ctx[0]->stream));
    }
    for (int r = 0; r < P; ++r) {
        HIP_TRY(hipSetDevice(g->devices[r]));
        if ((rc = io[r]->finish())) return rc;
    }
    if (emergent_flux)
        for (int r = 0; r < P; ++r) std::memcpy(emergent_flux + begin[r], gathered.data() + (size_t)r * per, (size_t)(begin[r + 1] - begin[r]) * sizeof(double));
    if (n_evaluations) *n_evaluations = ev;
    return SDX_OK;
}

}  // extern "C"

#ifdef SDX_PRE_STATS
// analysis build only (scripts/r5/pre_stats.sh): the phase time stamps of the pre-pass blocks of the launches so far, then cleared
extern "C" int sdx_pre_stats_read(unsigned long long* out, long long n_words)
{
    const size_t bytes = std::min<size_t>((size_t)n_words * 8, sizeof(unsigned long long) * (size_t)sdx::kPreStatSlots * 8);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sdx::g_pre_stats), bytes) != hipSuccess) return -1;
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(sdx::g_pre_stats)) != hipSuccess) return -1;
    return hipMemset(p, 0, sizeof(unsigned long long) * (size_t)sdx::kPreStatSlots * 8) == hipSuccess ? 0 : -1;
}
#endif

#ifdef SDX_WALK_STATS
// analysis build only (scripts/r4/walk_stats.sh): the line kernel's wave statistics of the launches so far, then cleared
extern "C" int sdx_walk_stats_read(unsigned long long* out, long long n_words)
{
    const size_t bytes = std::min<size_t>((size_t)n_words * 8, sizeof(unsigned long long) * (size_t)sdx::kWalkStatSlots * 8);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sdx::g_walk_stats), bytes) != hipSuccess) return -1;
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(sdx::g_walk_stats)) != hipSuccess) return -1;
    return hipMemset(p, 0, sizeof(unsigned long long) * (size_t)sdx::kWalkStatSlots * 8) == hipSuccess ? 0 : -1;
}
#endif

