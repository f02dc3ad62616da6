// Shared helpers of libpcseg (gfx950 only, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/pcseg.h"

namespace pcseg {

constexpr int WAVE = 64;

void set_error(const char *fmt, ...);

#define PCSEG_CHECK_HIP(expr)                                                              \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            pcseg::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return PCSEG_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)

#define PCSEG_CHECK_LAUNCH()                                                               \
    do {                                                                                   \
        hipError_t _e = hipGetLastError();                                                 \
        if (_e != hipSuccess) {                                                            \
            pcseg::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return PCSEG_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)

#define PCSEG_REQUIRE(cond, msg)                                                           \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            pcseg::set_error("%s: %s", __func__, msg);                                     \
            return PCSEG_ERR_ARG;                                                          \
        }                                                                                  \
    } while (0)

// optional per-kernel timing (pcseg_timing_enable): hipEvents recorded around every launch ON THE LAUNCH STREAM
struct LaunchTimer {
    hipStream_t stream;
    void *stop;  // hipEvent_t recorded by the destructor (nullptr: timing off)
    LaunchTimer(const char *kernel, const char *where, hipStream_t s);  // where = __PRETTY_FUNCTION__ (template arguments)
    ~LaunchTimer();
};

#define PCSEG_LAUNCH(kernel, grid, block, lds, stream, ...)                 \
    do {                                                                    \
        pcseg::LaunchTimer _timer(#kernel, __PRETTY_FUNCTION__, stream);                         \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);  \
    } while (0)

inline int check_shape(int B, int H, int W)
{
    // linear indices are int32 per frame; rows/cols are stored as uint16 in the EDT scratch
    if (B < 1 || H < 1 || W < 1) return 0;
    if ((int64_t)H * W >= ((int64_t)1 << 30)) return 0;
    if (H > 32768 || W > 32768) return 0;
    return 1;
}

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// carve typed regions out of the caller's workspace.  A workspace's layout is written ONCE, as the function that takes its
// regions: run on a null base it takes nothing (every region comes back null) and only adds up `off` -- which is what the
// pcseg_*_workspace_bytes queries return
struct Carver {
    char *base;
    size_t off = 0;
    size_t cap;
    Carver(void *p, size_t bytes) : base((char *)p), cap(bytes) {}
    template <typename T>
    T *take(size_t n)
    {
        size_t bytes = align_up(n * sizeof(T));
        T *p = base ? (T *)(base + off) : nullptr;
        off += bytes;
        return p;
    }
    bool ok() const { return off <= cap && base != nullptr; }
    // the workspace guard of every entry point, asked once its layout is carved: false, with the error set, where the
    // caller's workspace does not hold the layout (the entry point then returns PCSEG_ERR_WORKSPACE)
    bool fits(const char *who) const
    {
        if (!ok()) set_error("%s: workspace too small (%zu < %zu)", who, cap, off);
        return ok();
    }
};

// what a pcseg_*_workspace_bytes query answers: the bytes that `carve(cv, args...)` takes
template <typename Carve, typename... Args>
inline size_t carved_bytes(Carve carve, Args... args)
{
    Carver cv(nullptr, 0);
    carve(cv, args...);
    return cv.off;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }

// row * W as a FULL-RATE 24-bit multiply, widened afterwards: rows, word rows and widths are below 2^15 (check_shape) and a
// frame has fewer than 2^30 pixels, so the product fits 32 bits.  Written as (int64_t)r * W the compiler emits
// v_mad_u64_u32 -- a quarter-rate instruction -- for every pixel address of the tile kernels (87 of them in the union-find
// tile pass, whose VALU pipe is the bottleneck).
__device__ __forceinline__ int64_t rowoff(int r, int W) { return (int64_t)__mul24(r, W); }

// Inclusive prefix maximum / minimum over the 64 lanes of a wave with DPP moves only (no LDS round trip per step, which
// is what __shfl_up costs: ds_bpermute + a wait): four shifts inside the 16-lane rows, then lane 15 of rows 0 and 2 is
// broadcast into rows 1 and 3, then lane 31 into rows 2 and 3.  Lanes without a source keep `ident` (bound_ctrl off).
template <bool MAX>
__device__ __forceinline__ int wave_prefix_extreme(int x)
{
    constexpr int ident = MAX ? (int)0x80000000 : 0x7FFFFFFF;
#define PCSEG_DPP_STEP(ctrl, row_mask)                                                              \
    {                                                                                               \
        const int t = __builtin_amdgcn_update_dpp(ident, x, ctrl, row_mask, 0xF, false);            \
        x = MAX ? max(x, t) : min(x, t);                                                            \
    }
    PCSEG_DPP_STEP(0x111, 0xF)  // row_shr:1
    PCSEG_DPP_STEP(0x112, 0xF)  // row_shr:2
    PCSEG_DPP_STEP(0x114, 0xF)  // row_shr:4
    PCSEG_DPP_STEP(0x118, 0xF)  // row_shr:8
    PCSEG_DPP_STEP(0x142, 0xA)  // row_bcast:15 into rows 1 and 3
    PCSEG_DPP_STEP(0x143, 0xC)  // row_bcast:31 into rows 2 and 3
#undef PCSEG_DPP_STEP
    return x;
}
__device__ __forceinline__ int wave_prefix_max(int x) { return wave_prefix_extreme<true>(x); }
__device__ __forceinline__ int wave_prefix_min(int x) { return wave_prefix_extreme<false>(x); }
__device__ __forceinline__ int wave_last_lane(int x) { return __builtin_amdgcn_readlane(x, WAVE - 1); }

// ---- prefix sums (the only copies: every count -> offset step of the library goes through these two)
// inclusive prefix sum over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T v)
{
    const int lane = lane_id();
    for (int off = 1; off < WAVE; off <<= 1) {
        const T t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// exclusive prefix of v over the THREADS threads of a block, *total = the block's sum.  wsum: THREADS / 64 values of LDS,
// free for the next scan when the call returns (two barriers: every thread of the block must call)
template <int THREADS, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *total, T *wsum)
{
    static_assert(THREADS % WAVE == 0, "whole waves");
    const int wid = threadIdx.x / WAVE;
    const T inc = wave_inclusive_sum(v);
    if (lane_id() == WAVE - 1) wsum[wid] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < THREADS / WAVE; ++w) {
        if (w < wid) base += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// XCD-aware tile order for kernels whose blocks read a halo of their neighbours' pixels.  Workgroups are dealt
// round-robin over the 8 XCDs (blocks b and b + 8 share one; MI355X_MICROARCH.md, "Workgroup dispatch"), each XCD with
// an L2 of its own: with the plain blockIdx -> tile map the left / right neighbour of a tile runs on ANOTHER XCD, so
// every halo column costs its full cache line from HBM a second time (for a 64-column tile of 4-byte pixels: 6 lines
// fetched per 4 used).  This map hands XCD k the k-th eighth of the tile sequence (x fastest, then y, then frame), in
// order: neighbouring tiles of a frame are issued together on one XCD and share their halo lines in its L2.  Speed
// only -- any block -> tile bijection is correct.
struct TileIndex {
    int x, y, z;
};
__device__ __forceinline__ TileIndex xcd_tile_index()
{
    const unsigned gx = gridDim.x, gy = gridDim.y;
    const unsigned total = gx * gy * gridDim.z;
    const unsigned b = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const unsigned per = total / 8u;
    const unsigned t = b < per * 8u ? (b % 8u) * per + b / 8u : b;  // (a remainder of < 8 blocks keeps its place)
    TileIndex ti;
    ti.x = (int)(t % gx);
    ti.y = (int)((t / gx) % gy);
    ti.z = (int)(t / (gx * gy));
    return ti;
}

// relaxed agent-scope accesses: served by L2, never by a stale L1 line
__device__ __forceinline__ int ld_agent(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned ld_agent(const unsigned *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ccl.hip, for the fused class-map front end (frontend.hip): where the union-find image and the per-block root counts
// live in a pcseg_ccl_workspace_bytes workspace, and the passes after the tile pass for equal-valued 8-connected
// components of a uint8 image (border links, flatten + count, scan, relabel -> raster-order labels)
struct CclPlan {
    int *parent;
    int *blockcount;
    int nblk;
    int *corrupt;  // [B] raised by a fenced walk (union_find.h, walk_ok): the frame's count comes out as -1
};
int ccl_plan(void *workspace, size_t workspace_bytes, int B, int H, int W, CclPlan *plan, const char *who);
int ccl_equal_u8_finish(const uint8_t *in, const CclPlan &plan, bool tile_pass_done, int *labels, int *counts, int B, int H, int W,
                        hipStream_t s);

}  // namespace pcseg
