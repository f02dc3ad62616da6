// Grayscale morphological reconstruction (skimage.morphology.reconstruction of scikit-image 0.18.3, 2-D, 3 x 3 footprint or
// its 4-connected cross) and the elementwise steps of skimage.morphology.h_maxima / h_minima around it.
//
// Reconstruction by dilation of `seed` under `mask` is the largest image R with seed <= R <= mask in which every value above
// the seed is carried along a connected path of pixels whose mask is at least that value: the fixed point of
//     R <- max(R, min(mask, max of R over the neighbourhood)),      R(0) = min(seed, mask),
// with nothing outside the frame (the pad is the type's minimum, which raises nothing).  Erosion is the mirror image: min and
// max change places and the pad is the type's maximum.  Both are computed as written, on order-preserving unsigned keys of
// the values (int32: the sign bit flipped; float64: the usual total-order key, -0.0 read as +0.0) -- nothing is negated, so
// INT32_MIN and the infinities are values like any other.  Inputs must be free of NaN.
//
// The iteration runs on the marked-tile rounds of tile_rounds.h with one tiling: a tile of REC_TW x REC_TH pixels sits in
// LDS with a one-pixel halo, its four waves sweep it downwards, upwards, to the right and to the left (Gauss-Seidel: a sweep
// step reads the line the step before wrote) until a whole iteration of the four changes nothing, the tile is stored and
// every neighbour tile that touches a rim pixel the visit changed is marked.  Round 0 visits every tile, REC_GRID_ROUNDS
// rounds are grids, the tail kernel does the rest; at the round cap the frame's REC_FLAG_ROUNDS is raised: the image is no
// fixed point and must not be used.  No value is read back and nothing is allocated: the launch sequence is fixed.
//
// WHAT THE ROUNDS NEED: MONOTONE VALUES.  (Dilation; erosion with the order reversed.)  Values only rise: R(0) <= every
// later R <= the fixed point F (induction: min(mask, max over neighbours of something <= F) <= F), so whatever a tile reads
// from a neighbour's rim while that neighbour stores it -- the clamped seed in round 0, an older or a newer stored value
// later, never a mixture: stores are naturally aligned 4- or 8-byte words -- is a lower bound of F, and so is everything the
// tile derives from it.  A tile marks after its store (rec_tile).  So when a round marks nothing the image is a fixed point
// of the whole frame, and being between R(0) and F it is F.
#include <algorithm>
#include <climits>

#include "common.h"
#include "tile_rounds.h"

// the elementwise kernels must round as numpy does: one rounding per written operation, no fused multiply-add
#pragma clang fp contract(off)

namespace pcseg {

constexpr int REC_TW = 64, REC_TH = 32;                   // tile width and height
constexpr int REC_SW = REC_TW + 2, REC_SH = REC_TH + 2;   // with halo
constexpr int REC_THREADS = 256;                          // one wave per sweep direction
constexpr int REC_GRID_ROUNDS = 6;                        // rounds enqueued as grids (round 0: every tile; then device lists)
constexpr int REC_LIST_GRID = 512;                        // blocks of a list-walking round
// iterations of one tile visit: an iteration that changes something settles at least one more pixel of the tile for good
constexpr int REC_MAX_SWEEPS = REC_TW * REC_TH + 2;
constexpr int REC_FLAG_SEED = PCSEG_RECONSTRUCT_SEED_BEYOND_MASK, REC_FLAG_ROUNDS = PCSEG_RECONSTRUCT_NOT_CONVERGED;
// the workspace's counters (int32): [r] tiles listed for grid round r (1 <= r < REC_GRID_ROUNDS), then
constexpr int REC_CNT_GRID_TILES = 16, REC_CNT_TAIL_TILES = 17, REC_CNT_TAIL_ROUNDS = 18, REC_COUNTERS = 32;
static_assert(REC_GRID_ROUNDS <= REC_CNT_GRID_TILES, "one counter per grid round");
static_assert(REC_THREADS == 4 * WAVE && REC_TW == WAVE && REC_TH <= WAVE, "a wave spans a tile row; a column fits a wave");

// order-preserving unsigned keys
template <typename T>
struct RecKey;
template <>
struct RecKey<int32_t> {
    using K = unsigned;
    __device__ static __forceinline__ K key(int32_t v) { return (unsigned)v ^ 0x80000000u; }
    __device__ static __forceinline__ int32_t value(K k) { return (int32_t)(k ^ 0x80000000u); }
};
template <>
struct RecKey<double> {
    using K = unsigned long long;
    __device__ static __forceinline__ K key(double v)
    {
        if (v == 0.0) v = 0.0;  // -0.0 == +0.0
        const unsigned long long u = (unsigned long long)__double_as_longlong(v);
        return (u >> 63) ? ~u : (u | (1ull << 63));
    }
    __device__ static __forceinline__ double value(K k) { return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k)); }
};

// dilation: values grow towards the mask from below; erosion: they shrink towards it from above
template <typename K, bool ERODE>
struct RecOrder {
    static constexpr K PAD = ERODE ? ~(K)0 : (K)0;
    __device__ static __forceinline__ K lower(K a, K b) { return a < b ? a : b; }
    __device__ static __forceinline__ K upper(K a, K b) { return a < b ? b : a; }
    __device__ static __forceinline__ K grow(K a, K b) { return ERODE ? lower(a, b) : upper(a, b); }
    __device__ static __forceinline__ K clamp(K a, K m) { return ERODE ? upper(a, m) : lower(a, m); }
    __device__ static __forceinline__ bool beyond(K s, K m) { return ERODE ? s < m : s > m; }
    __device__ static __forceinline__ void atomic_grow(K *p, K v)
    {
        if (ERODE) atomicMin(p, v);
        else atomicMax(p, v);
    }
};

template <typename T>
struct RecArgs {
    const T *seed, *mask;
    T *out;
    int *flags;     // [B]
    int *counters;  // REC_COUNTERS
    int H, W, conn, tilesX, tilesY;
};

// the lanes of one wave have written LDS and are about to read each other's values (what a cooperative group of the
// wave's size does to synchronise)
__device__ __forceinline__ void rec_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// mark tile (tx, ty) of frame b, if the frame has it, for the next round
__device__ __forceinline__ void rec_mark(uint8_t *dout, int *list_out, int *count_out, int b, int tx, int ty, int tilesX, int tilesY)
{
    if (tx < 0 || tx >= tilesX || ty < 0 || ty >= tilesY) return;
    mark_tile(dout, list_out, count_out, ((int64_t)b * tilesY + ty) * tilesX + tx);
}

// One visit of tile (tx, ty) of frame b (block-uniform control flow: every return is taken by all threads of the block).
// FIRST: round 0 -- no mark is needed, the tile starts from min(seed, mask) (halo included: a neighbour may not have stored
// anything yet) and is stored in any case.
template <typename T, bool ERODE>
__device__ __forceinline__ void rec_tile(typename RecKey<T>::K *sR, typename RecKey<T>::K *sM, const RecArgs<T> &a, const bool FIRST,
                                         uint8_t *din, uint8_t *dout, int *list_out, int *count_out, int counter, int b, int tx, int ty)
{
    using KT = RecKey<T>;
    using K = typename KT::K;
    using O = RecOrder<K, ERODE>;
    constexpr int TW = REC_TW, TH = REC_TH, SW = REC_SW, SH = REC_SH, NT = REC_THREADS;
    const int tid = threadIdx.x;
    if (!FIRST && !take_mark(din + ((int64_t)b * a.tilesY + ty) * a.tilesX + tx)) return;
    if (!FIRST && tid == 0) atomicAdd(a.counters + counter, 1);
    const int H = a.H, W = a.W;
    const int r0 = ty * TH, c0 = tx * TW;
    const int64_t fbase = (int64_t)b * H * W;
    bool beyond = false;
    for (int i = tid; i < SH * SW; i += NT) {
        const int lr = i / SW, lc = i % SW;
        const int r = r0 + lr - 1, c = c0 + lc - 1;
        K kr = O::PAD, km = O::PAD;
        if (r >= 0 && r < H && c >= 0 && c < W) {
            const int64_t g = fbase + rowoff(r, W) + c;
            km = KT::key(a.mask[g]);
            if (FIRST) {
                const K ks = KT::key(a.seed[g]);
                if (lr >= 1 && lr <= TH && lc >= 1 && lc <= TW && O::beyond(ks, km)) beyond = true;
                kr = O::clamp(ks, km);
            } else {
                kr = KT::key(a.out[g]);
            }
        }
        sR[i] = kr;
        sM[i] = km;
    }
    const bool any_beyond = __syncthreads_or(beyond);  // (also the barrier after the load)
    if (FIRST && any_beyond && tid == 0) atomicOr(a.flags + b, REC_FLAG_SEED);
    // thread = rim pixel: 0 .. 63 the top row, 64 .. 127 the bottom row, 128 .. 159 the left column, 160 .. 191 the right one.
    // Each remembers the value its pixel had on arrival: what the visit changed on the rim is known without global memory
    const int wave = tid >> 6, lane = tid & 63;
    int rim = -1;
    if (wave == 0) rim = 1 * SW + 1 + lane;
    else if (wave == 1) rim = TH * SW + 1 + lane;
    else if (wave == 2 && lane < TH) rim = (1 + lane) * SW + 1;
    else if (wave == 2 && lane < 2 * TH) rim = (1 + lane - TH) * SW + TW;
    const K rim_before = rim >= 0 ? sR[rim] : (K)0;
    // wave 0 sweeps down (lane = column, one row per step), wave 1 up, wave 2 to the right (lane = row, one column per step),
    // wave 3 to the left.  A step reads the line behind it -- the pixel straight behind and, with 8 neighbours, its two
    // diagonal ones -- which the same wave's step before wrote: the lanes of one wave exchange through LDS, which serves a
    // wave's accesses in order, so between two steps the wave only synchronises with itself (rec_wave_sync) and the four
    // sweeps run at their own pace.  Waves write each other's pixels: every write is an LDS atomic max / min, so a pixel never
    // moves backwards, and whatever a wave misses of another's progress is a lower bound.  The end does not depend on any of
    // this: it is the block-wide vote after an iteration in which NO wave wrote, and in such an iteration every read saw the
    // final state.  The vertical sweeps have TH steps and run twice while the horizontal ones run once.
    const bool conn8 = a.conn == 8;
    bool changed_any = false, capped = true;
    for (int iter = 0; iter < REC_MAX_SWEEPS; ++iter) {
        bool changed = false;
        for (int step = 0; step < TW; ++step) {
            int i, behind, side;
            bool active = true;
            if (wave < 2) {
                const int s = step % TH;
                i = (wave == 0 ? 1 + s : TH - s) * SW + 1 + lane;
                behind = wave == 0 ? -SW : SW;
                side = 1;
            } else {
                active = lane < TH;
                i = (1 + (active ? lane : 0)) * SW + (wave == 2 ? 1 + step : TW - step);
                behind = wave == 2 ? -1 : 1;
                side = SW;
            }
            if (active) {
                K best = sR[i + behind];
                if (conn8) best = O::grow(best, O::grow(sR[i + behind - side], sR[i + behind + side]));
                const K cur = sR[i];
                const K nw = O::grow(cur, O::clamp(best, sM[i]));
                if (nw != cur) {
                    O::atomic_grow(&sR[i], nw);
                    changed = true;
                }
            }
            rec_wave_sync();
        }
        if (!__syncthreads_or(changed)) {
            capped = false;
            break;
        }
        changed_any = true;
    }
    if (capped && tid == 0) atomicOr(a.flags + b, REC_FLAG_ROUNDS);  // (cannot happen, see REC_MAX_SWEEPS: never spin)
    if (!FIRST && !changed_any) return;
    for (int i = tid; i < TH * TW; i += NT) {
        const int lr = i / TW, lc = i % TW;
        const int r = r0 + lr, c = c0 + lc;
        if (r < H && c < W) a.out[fbase + rowoff(r, W) + c] = KT::value(sR[(lr + 1) * SW + lc + 1]);
    }
    if (!changed_any) return;
    // the neighbours whose halo holds a rim pixel that changed, after the store
    __threadfence();
    __syncthreads();
    const unsigned long long ch = __ballot(rim >= 0 && sR[rim] != rim_before);
    if (lane == 0 && ch != 0) {
        const unsigned long long first = 1ull, last = 1ull << 63;
        if (wave < 2) {
            const int ny = wave == 0 ? ty - 1 : ty + 1;
            rec_mark(dout, list_out, count_out, b, tx, ny, a.tilesX, a.tilesY);
            if (conn8 && (ch & first)) rec_mark(dout, list_out, count_out, b, tx - 1, ny, a.tilesX, a.tilesY);
            if (conn8 && (ch & last)) rec_mark(dout, list_out, count_out, b, tx + 1, ny, a.tilesX, a.tilesY);
        } else if (wave == 2) {
            if (ch & ((1ull << TH) - 1ull)) rec_mark(dout, list_out, count_out, b, tx - 1, ty, a.tilesX, a.tilesY);
            if (ch >> TH) rec_mark(dout, list_out, count_out, b, tx + 1, ty, a.tilesX, a.tilesY);
        }
    }
}

#define PCSEG_REC_LDS(T)                                                     \
    __shared__ typename RecKey<T>::K sR[REC_SH * REC_SW];                    \
    __shared__ typename RecKey<T>::K sM[REC_SH * REC_SW];

// round 0: grid = (tilesX, tilesY, B)
template <typename T, bool ERODE>
__global__ void __launch_bounds__(REC_THREADS) rec_first_kernel(RecArgs<T> a, uint8_t *dout, int *list_out, int *count_out)
{
    PCSEG_REC_LDS(T)
    rec_tile<T, ERODE>(sR, sM, a, true, nullptr, dout, list_out, count_out, 0, blockIdx.z, blockIdx.x, blockIdx.y);
}

// rounds 1 .. REC_GRID_ROUNDS - 1: a fixed grid walks the list of tiles the round before marked.  (walk_list and the list's
// decode rather than for_tiles around them: through the second closure the kernel takes 102 scalar registers instead of
// 100, and the int32 kernels then hold 7 waves per SIMD where their LDS allows 8 -- profiles/tile_rounds/resource_usage.md.)
template <typename T, bool ERODE>
__global__ void __launch_bounds__(REC_THREADS) rec_list_kernel(RecArgs<T> a, uint8_t *din, uint8_t *dout, const int *list, const int *count,
                                                               int *list_out, int *count_out)
{
    PCSEG_REC_LDS(T)
    const TileList tiles{list, count, a.tilesX * a.tilesY, a.tilesX};
    walk_list(list, count, blockIdx.x, gridDim.x, [&](const int e) {
        const TileAt t = tiles.at(e);
        rec_tile<T, ERODE>(sR, sM, a, false, din, dout, list_out, count_out, REC_CNT_GRID_TILES, t.b, t.tx, t.ty);
        __syncthreads();  // the next listed tile reuses the LDS tile
    });
}

// the rest of the fixed point, one block per frame; at the round cap (max_rounds) the frame is flagged
template <typename T, bool ERODE>
__global__ void __launch_bounds__(REC_THREADS) rec_tail_kernel(RecArgs<T> a, uint8_t *din, uint8_t *dout, int max_rounds)
{
    PCSEG_REC_LDS(T)
    const int b = blockIdx.x;
    const Tiling tiling{0, a.tilesX, a.tilesY};
    const int rounds = tail_rounds<REC_THREADS>(
        b, din, dout, 0, max_rounds, tiling, tiling, [](const int) { return true; },
        [&](const Tiling &, const Tiling &, const int tx, const int ty, uint8_t *in, uint8_t *out) {
            rec_tile<T, ERODE>(sR, sM, a, false, in, out, nullptr, nullptr, REC_CNT_TAIL_TILES, b, tx, ty);
        });
    if (threadIdx.x != 0) return;
    if (rounds < 0) atomicOr(a.flags + b, REC_FLAG_ROUNDS);
    else if (rounds > 0) atomicMax(a.counters + REC_CNT_TAIL_ROUNDS, rounds);
}

struct RecWorkspace {
    int *counters;
    uint8_t *markA, *markB;
    int *list[2];
};

// ORDER MATTERS from counters to markB: one fill clears the three of them.
static RecWorkspace rec_carve(Carver &cv, int B, int H, int W)
{
    const size_t ntiles = (size_t)B * ((W + REC_TW - 1) / REC_TW) * ((H + REC_TH - 1) / REC_TH);
    RecWorkspace ws;
    ws.counters = cv.take<int>(REC_COUNTERS);
    ws.markA = cv.take<uint8_t>(ntiles);
    ws.markB = cv.take<uint8_t>(ntiles);
    ws.list[0] = cv.take<int>(ntiles);
    ws.list[1] = cv.take<int>(ntiles);
    return ws;
}

template <typename T, bool ERODE>
static int rec_rounds(const RecArgs<T> &a, const RecWorkspace &ws, int B, int max_rounds, hipStream_t s)
{
    uint8_t *din = ws.markA, *dout = ws.markB;
    for (int round = 0; round < REC_GRID_ROUNDS; ++round) {
        // (a round's marks go into the next round's list while that round is a grid; the tail kernel scans the marks)
        const bool lists_next = round + 1 < REC_GRID_ROUNDS;
        int *lout = lists_next ? ws.list[(round + 1) & 1] : nullptr, *cout = lists_next ? ws.counters + round + 1 : nullptr;
        if (round == 0)
            PCSEG_LAUNCH((rec_first_kernel<T, ERODE>), dim3(a.tilesX, a.tilesY, B), dim3(REC_THREADS), 0, s, a, dout, lout, cout);
        else
            PCSEG_LAUNCH((rec_list_kernel<T, ERODE>), dim3(REC_LIST_GRID), dim3(REC_THREADS), 0, s, a, din, dout, (const int *)ws.list[round & 1],
                         (const int *)(ws.counters + round), lout, cout);
        PCSEG_CHECK_LAUNCH();
        uint8_t *t = din;
        din = dout;
        dout = t;
    }
    PCSEG_LAUNCH((rec_tail_kernel<T, ERODE>), dim3(B), dim3(REC_THREADS), 0, s, a, din, dout, max_rounds);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

template <typename T>
static int reconstruct(const char *who, const T *seed, const T *mask, T *out, int32_t *flags, int B, int H, int W, int conn, int method,
                       int max_rounds, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    if (!(seed && mask && out && flags && workspace && check_shape(B, H, W) && B <= 65535 && (conn == 4 || conn == 8) &&
          (method == PCSEG_RECONSTRUCT_DILATION || method == PCSEG_RECONSTRUCT_EROSION) && out != seed && out != mask)) {
        set_error("%s: bad arguments", who);
        return PCSEG_ERR_ARG;
    }
    const int tilesX = (W + REC_TW - 1) / REC_TW, tilesY = (H + REC_TH - 1) / REC_TH;
    if ((int64_t)B * tilesX * tilesY >= ((int64_t)1 << 31) || tilesY > 65535) {
        set_error("%s: bad arguments", who);
        return PCSEG_ERR_ARG;
    }
    Carver cv(workspace, workspace_bytes);
    const RecWorkspace ws = rec_carve(cv, B, H, W);
    if (!cv.fits(who)) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (max_rounds <= 0) max_rounds = (tilesX * tilesY + 64) * 64;  // (the watershed's cap)
    PCSEG_CHECK_HIP(hipMemsetAsync(ws.counters, 0, (size_t)((char *)ws.list[0] - (char *)ws.counters), s));
    PCSEG_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)B, s));
    const RecArgs<T> a{seed, mask, out, flags, ws.counters, H, W, conn, tilesX, tilesY};
    return method == PCSEG_RECONSTRUCT_EROSION ? rec_rounds<T, true>(a, ws, B, max_rounds, s) : rec_rounds<T, false>(a, ws, B, max_rounds, s);
}

// ---- h-maxima / h-minima: range, shift, mark
// range[2 b] / range[2 b + 1]: the keys (widened to 64 bits) of the smallest / largest value of frame b
__global__ void __launch_bounds__(256) hmax_range_init_kernel(unsigned long long *range, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        range[2 * b] = ~0ull;
        range[2 * b + 1] = 0ull;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) hmax_range_kernel(const T *__restrict__ img, unsigned long long *__restrict__ range, int64_t n)
{
    const int b = blockIdx.y;
    const T *f = img + (int64_t)b * n;
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = RecKey<T>::key(f[i]);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const unsigned long long l = (unsigned long long)__shfl_xor((long long)lo, off), u = (unsigned long long)__shfl_xor((long long)hi, off);
        lo = l < lo ? l : lo;
        hi = u > hi ? u : hi;
    }
    if (lane_id() == 0) {
        atomicMin(range + 2 * b, lo);
        atomicMax(range + 2 * b + 1, hi);
    }
}

// is h above the frame's range (scikit-image's leading test `h > np.ptp(image)`)?  EDT: the image is sqrt(d2) of the int32 range
template <typename T, typename HT>
__device__ __forceinline__ bool hmax_above_range(const unsigned long long *range, int b, HT h, bool edt);
template <>
__device__ __forceinline__ bool hmax_above_range<int32_t, int64_t>(const unsigned long long *range, int b, int64_t h, bool)
{
    const int64_t lo = RecKey<int32_t>::value((unsigned)range[2 * b]), hi = RecKey<int32_t>::value((unsigned)range[2 * b + 1]);
    return h > hi - lo;
}
template <>
__device__ __forceinline__ bool hmax_above_range<double, double>(const unsigned long long *range, int b, double h, bool edt)
{
    double lo, hi;
    if (edt) {
        lo = sqrt((double)RecKey<int32_t>::value((unsigned)range[2 * b]));
        hi = sqrt((double)RecKey<int32_t>::value((unsigned)range[2 * b + 1]));
    } else {
        lo = RecKey<double>::value(range[2 * b]);
        hi = RecKey<double>::value(range[2 * b + 1]);
    }
    const double ptp = hi - lo;
    return h > ptp;
}

// sign < 0: h_maxima's seed image - h, clipped at the type's minimum; sign > 0: h_minima's image + h, clipped at its maximum
__global__ void __launch_bounds__(256) hmax_shift_i32_kernel(const int32_t *__restrict__ img, int64_t h, int sign, int32_t *__restrict__ seed,
                                                              int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t v = (int64_t)img[i] + (sign < 0 ? -h : h);
    seed[i] = (int32_t)(v < INT_MIN ? (int64_t)INT_MIN : v > INT_MAX ? (int64_t)INT_MAX : v);
}

// the float64 shift: resolution = (2 * 1e-15) * |x|, then (x - h) - resolution or (x + h) + resolution: three roundings
__device__ __forceinline__ double hmax_shifted(double x, double h, int sign)
{
    const double resolution = (2.0 * 1e-15) * fabs(x);
    if (sign < 0) {
        const double d = x - h;
        return d - resolution;
    }
    const double d = x + h;
    return d + resolution;
}

__global__ void __launch_bounds__(256) hmax_shift_f64_kernel(const double *__restrict__ img, double h, int sign, double *__restrict__ seed,
                                                              int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) seed[i] = hmax_shifted(img[i], h, sign);
}

__global__ void __launch_bounds__(256) hmax_shift_edt_kernel(const int32_t *__restrict__ d2, double h, double *__restrict__ dist,
                                                              double *__restrict__ seed, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const double d = sqrt((double)d2[i]);
    dist[i] = d;
    seed[i] = hmax_shifted(d, h, -1);
}

// out = residue >= h with residue = image - rec (sign < 0) or rec - image (sign > 0); all zero in a frame whose range is below h
template <typename T, typename HT>
__global__ void __launch_bounds__(256) hmax_mark_kernel(const T *__restrict__ img, const T *__restrict__ rec, HT h, int sign,
                                                         const unsigned long long *__restrict__ range, bool edt, uint8_t *__restrict__ out,
                                                         int64_t n)
{
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t g = (int64_t)b * n + i;
    if (hmax_above_range<T, HT>(range, b, h, edt)) {
        out[g] = 0;
        return;
    }
    const HT x = (HT)img[g], r = (HT)rec[g];
    const HT residue = sign < 0 ? x - r : r - x;
    out[g] = residue >= h ? 1 : 0;
}

static inline unsigned hmax_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

template <typename T>
static int hmax_range(const T *img, uint64_t *range, int B, int H, int W, pcseg_stream_t stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    PCSEG_LAUNCH(hmax_range_init_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (unsigned long long *)range, B);
    PCSEG_CHECK_LAUNCH();
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 256 * 16 - 1) / (256 * 16), 1024);
    PCSEG_LAUNCH(hmax_range_kernel<T>, dim3(blocks, B), dim3(256), 0, s, img, (unsigned long long *)range, n);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

template <typename T, typename HT>
static int hmax_mark(const T *img, const T *rec, HT h, int sign, const uint64_t *range, bool edt, uint8_t *out, int B, int H, int W,
                     pcseg_stream_t stream)
{
    const int64_t n = (int64_t)H * W;
    PCSEG_LAUNCH((hmax_mark_kernel<T, HT>), dim3(hmax_blocks(n), B), dim3(256), 0, (hipStream_t)stream, img, rec, h, sign,
                 (const unsigned long long *)range, edt, out, n);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_reconstruct_workspace_bytes(int B, int H, int W)
{
    if (!check_shape(B, H, W)) return 0;
    return carved_bytes(rec_carve, B, H, W);
}

int pcseg_reconstruct_i32(const int32_t *seed, const int32_t *mask, int32_t *out, int32_t *flags, int B, int H, int W, int conn, int method,
                          int max_rounds, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    return reconstruct<int32_t>(__func__, seed, mask, out, flags, B, H, W, conn, method, max_rounds, workspace, workspace_bytes, stream);
}

int pcseg_reconstruct_f64(const double *seed, const double *mask, double *out, int32_t *flags, int B, int H, int W, int conn, int method,
                          int max_rounds, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    return reconstruct<double>(__func__, seed, mask, out, flags, B, H, W, conn, method, max_rounds, workspace, workspace_bytes, stream);
}

int pcseg_hmax_range_i32(const int32_t *img, uint64_t *range, int B, int H, int W, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(img && range && check_shape(B, H, W) && B <= 65535, "bad arguments");
    return hmax_range<int32_t>(img, range, B, H, W, stream);
}

int pcseg_hmax_range_f64(const double *img, uint64_t *range, int B, int H, int W, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(img && range && check_shape(B, H, W) && B <= 65535, "bad arguments");
    return hmax_range<double>(img, range, B, H, W, stream);
}

int pcseg_hmax_shift_i32(const int32_t *img, int64_t h, int sign, int32_t *seed, int B, int H, int W, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(img && seed && check_shape(B, H, W) && (sign == 1 || sign == -1) && h > 0 && h <= (int64_t)0xFFFFFFFFll, "bad arguments");
    const int64_t total = (int64_t)B * H * W;
    PCSEG_LAUNCH(hmax_shift_i32_kernel, dim3(hmax_blocks(total)), dim3(256), 0, (hipStream_t)stream, img, h, sign, seed, total);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_hmax_shift_f64(const double *img, double h, int sign, double *seed, int B, int H, int W, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(img && seed && check_shape(B, H, W) && (sign == 1 || sign == -1) && h > 0, "bad arguments");
    const int64_t total = (int64_t)B * H * W;
    PCSEG_LAUNCH(hmax_shift_f64_kernel, dim3(hmax_blocks(total)), dim3(256), 0, (hipStream_t)stream, img, h, sign, seed, total);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_hmax_shift_edt(const int32_t *d2, double h, double *dist, double *seed, int B, int H, int W, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(d2 && dist && seed && check_shape(B, H, W) && h > 0, "bad arguments");
    const int64_t total = (int64_t)B * H * W;
    PCSEG_LAUNCH(hmax_shift_edt_kernel, dim3(hmax_blocks(total)), dim3(256), 0, (hipStream_t)stream, d2, h, dist, seed, total);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_hmax_mark_i32(const int32_t *img, const int32_t *rec, int64_t h, int sign, const uint64_t *range, uint8_t *out, int B, int H, int W,
                        pcseg_stream_t stream)
{
    PCSEG_REQUIRE(img && rec && range && out && check_shape(B, H, W) && B <= 65535 && (sign == 1 || sign == -1) && h > 0, "bad arguments");
    return hmax_mark<int32_t, int64_t>(img, rec, h, sign, range, false, out, B, H, W, stream);
}

int pcseg_hmax_mark_f64(const double *img, const double *rec, double h, int sign, const uint64_t *range, int range_of_d2, uint8_t *out, int B,
                        int H, int W, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(img && rec && range && out && check_shape(B, H, W) && B <= 65535 && (sign == 1 || sign == -1) && h > 0 &&
                      (range_of_d2 == 0 || range_of_d2 == 1),
                  "bad arguments");
    return hmax_mark<double, double>(img, rec, h, sign, range, range_of_d2 != 0, out, B, H, W, stream);
}

}  // extern "C"
