// Per-ROI shape table: second moments, axes, orientation and perimeter of every label of an int32 label image
// (what skimage's RegionProperties offers beyond the fields the reference itself reads: tiff_analysis.py:742-883, 1018
// hand RegionProperties objects back; HCN_nanosims_rois_activity_distance_5iso_YG.m:104, 173 ask for regionprops 'all').
//
// Everything a label contributes is an INTEGER: three second-order sums and four counts of border pixels, so the table
// does not depend on the order of the atomics and is exact in int64 for any frame check_shape admits (H W < 2^30).
//
// Launches (asynchronous, no host read):
//   shape_init_kernel       rows below min(counts[b], cap) zeroed, the frame's label bound and overflow flag set
//   shape_moments_kernel    the column-run walk of label_reduce.h (a lane owns 4 columns x 32 rows, same-label neighbouring
//                           lanes are summed by a segmented shuffle): a vertical run [r0, r1) in column c adds S2(r1 - 1) -
//                           S2(r0 - 1), c * sum r and n c^2 in closed form (no per-pixel work), into a slot table of 64-bit
//                           partials (the sum of r^2 of one block in absolute rows does not fit 32 bits) with an
//                           eight-lanes-per-row flush
//   shape_perimeter_kernel  skimage.measure.perimeter(region.image, 4) on integers: a 64 x 32 label tile with a 2-pixel halo
//                           in LDS, border bits of the tile plus a 1-pixel ring in LDS, the class of a border pixel from three
//                           constant 64-bit masks indexed by its neighbourhood value; a lane walks 8 rows of one column, the
//                           wave sums same-label neighbouring lanes, then one LDS table and integer global atomics
//   shape_properties_kernel one thread per row: the derived float64 columns
#include "label_reduce.h"

// every product, quotient and sum of the derived columns rounded on its own (no FMA), as neighbours.hip and surface.hip
#pragma clang fp contract(off)

namespace pcseg {

struct ShWorkspace {
    int *nrows;  // [B] min(counts[b], cap): the label bound of both passes (labels above it own no initialised row)
};

// the ONE layout of the workspace
static ShWorkspace shape_carve(Carver &cv, int B)
{
    ShWorkspace w;
    w.nrows = cv.take<int>((size_t)B);
    return w;
}

__global__ void __launch_bounds__(256) shape_init_kernel(long long *__restrict__ out, const int *__restrict__ counts,
                                                          int *__restrict__ nrows, int *__restrict__ overflow, int cap)
{
    const int b = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int nl = min(max(counts[b], 0), cap);
    if (idx == 0) {
        nrows[b] = nl;
        if (overflow) overflow[b] = 0;
    }
    if ((idx >> 3) < nl) out[(int64_t)b * cap * 8 + idx] = 0;
}

// ---- moments
struct RunMom {
    int key;  // the label; 0 = none
    unsigned long long rr, rc, cc;
};

// sum of i^2 for i = 0..x (x >= -1)
__device__ __forceinline__ long long sum_squares(long long x) { return x * (x + 1) * (2 * x + 1) / 6; }

// VEC: W % 4 == 0 and a 16-byte aligned image: one 16-byte load per row; otherwise four guarded 4-byte loads
template <bool VEC>
struct MomentsWalk : LabelRows<VEC> {
    using Run = RunMom;
    int *tags;
    unsigned long long (*lm)[4];
    long long *gout;
    int *overflow;
    int b, nl, cap;
    __device__ __forceinline__ Run run(int label, int start, int end, int col) const
    {
        const long long n = end - start;
        const long long sr = n * (start + end - 1) / 2;
        return Run{label, (unsigned long long)(sum_squares(end - 1) - sum_squares(start - 1)), (unsigned long long)(sr * col),
                   (unsigned long long)(n * col * col)};
    }
    static __device__ __forceinline__ Run shfl(const Run &a, int off)
    {
        return Run{a.key, __shfl_down(a.rr, off), __shfl_down(a.rc, off), __shfl_down(a.cc, off)};
    }
    static __device__ __forceinline__ void merge(Run &a, const Run &o) { a.rr += o.rr; a.rc += o.rc; a.cc += o.cc; }
    __device__ __forceinline__ void commit(const Run &a) const
    {
        if (a.key > nl) {
            if (a.key > cap && overflow) overflow[b] = 1;
            return;
        }
        const int slot = slot_claim(tags, a.key);
        if (slot >= 0) {
            atomicAdd(&lm[slot][0], a.rr);
            atomicAdd(&lm[slot][1], a.rc);
            atomicAdd(&lm[slot][2], a.cc);
        } else {
            unsigned long long *t = (unsigned long long *)(gout + (int64_t)(a.key - 1) * 8);
            atomicAdd(&t[0], a.rr);
            atomicAdd(&t[1], a.rc);
            atomicAdd(&t[2], a.cc);
        }
    }
};

template <bool VEC>
__global__ void __launch_bounds__(256, 4) shape_moments_kernel(const int *__restrict__ labels, const int *__restrict__ nrows, int H,
                                                                int W, int cap, long long *__restrict__ out,
                                                                int *__restrict__ overflow)
{
    __shared__ int tags[LABEL_SLOTS];
    __shared__ unsigned long long lm[LABEL_SLOTS][4];
    const TileIndex ti = xcd_tile_index();  // (a frame's blocks on one XCD: their atomics on the frame's table meet in one L2)
    const int b = ti.z;
    const int nl = nrows[b];
    long long *gout = out + (int64_t)b * cap * 8;
    for (int i = threadIdx.x; i < LABEL_SLOTS; i += 256) {
        tags[i] = 0;
        lm[i][0] = 0; lm[i][1] = 0; lm[i][2] = 0;
    }
    __syncthreads();
    const int c = (ti.x * 256 + threadIdx.x) * 4;
    const int r0 = ti.y * RUN_ROWS;
    column_run_walk(MomentsWalk<VEC>{{labels + (int64_t)b * H * W, c, W}, tags, lm, gout, overflow, b, nl, cap}, c, r0,
                    min(H, r0 + RUN_ROWS));
    __syncthreads();
    // flush: one atomic instruction carries the three neighbouring words of a row's 64-byte line
    slots_flush8(tags, [&](int i, int l, int f) {
        if (f < 3 && lm[i][f]) atomicAdd((unsigned long long *)(gout + (int64_t)(l - 1) * 8 + f), lm[i][f]);
    });
}

// ---- perimeter
constexpr int PT_W = 64, PT_H = 32;                // pixels of a tile
constexpr int PL_W = PT_W + 4, PL_H = PT_H + 4;    // labels: the tile and a 2-pixel halo
constexpr int PB_W = PT_W + 2, PB_H = PT_H + 2;    // border bits: the tile and a 1-pixel ring
// value v = 1 + 2 #(4-neighbours on the border) + 10 #(diagonal neighbours on the border) of a border pixel -> its weight
// class (skimage.measure.perimeter: 1 for {5,7,15,17,25,27}, sqrt 2 for {21,33}, (1 + sqrt 2) / 2 for {13,23})
constexpr unsigned long long PM_ONE = (1ull << 5) | (1ull << 7) | (1ull << 15) | (1ull << 17) | (1ull << 25) | (1ull << 27);
constexpr unsigned long long PM_SQRT2 = (1ull << 21) | (1ull << 33);
constexpr unsigned long long PM_MID = (1ull << 13) | (1ull << 23);

struct PerSlots {
    int *tags;
    int (*cnt)[4];
};

// lo = n_1 | n_sqrt2 << 16, hi = n_mid | n_border << 16 (a wave adds at most 512 to a field)
__device__ __forceinline__ void per_commit(const PerSlots &ls, long long *gout, int *overflow, int b, int nl, int cap, int l,
                                           unsigned lo, unsigned hi)
{
    if (l > nl) {
        if (l > cap && overflow) overflow[b] = 1;
        return;
    }
    const unsigned v[4] = {lo & 0xFFFFu, lo >> 16, hi & 0xFFFFu, hi >> 16};
    const int slot = slot_claim(ls.tags, l);
    if (slot >= 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (v[k]) atomicAdd((unsigned *)&ls.cnt[slot][k], v[k]);
    } else {
        unsigned long long *t = (unsigned long long *)(gout + (int64_t)(l - 1) * 8 + 3);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (v[k]) atomicAdd(&t[k], (unsigned long long)v[k]);
    }
}

__global__ void __launch_bounds__(256) shape_perimeter_kernel(const int *__restrict__ labels, const int *__restrict__ nrows, int H,
                                                               int W, int cap, long long *__restrict__ out,
                                                               int *__restrict__ overflow)
{
    __shared__ int lab[PL_H][PL_W];
    __shared__ uint8_t bb[PB_H][PB_W + 2];
    __shared__ int tags[LABEL_SLOTS];
    __shared__ int cnt[LABEL_SLOTS][4];
    const TileIndex ti = xcd_tile_index();  // (neighbouring tiles share their halo lines in one L2)
    const int b = ti.z;
    const int nl = nrows[b];
    const int *g = labels + (int64_t)b * H * W;
    long long *gout = out + (int64_t)b * cap * 8;
    const int R0 = ti.y * PT_H, C0 = ti.x * PT_W;
    for (int i = threadIdx.x; i < LABEL_SLOTS; i += 256) {
        tags[i] = 0;
        cnt[i][0] = 0; cnt[i][1] = 0; cnt[i][2] = 0; cnt[i][3] = 0;
    }
    // labels of the tile and its halo; -1 outside the image: never a label, so "outside" counts as another label
    for (int idx = threadIdx.x; idx < PL_H * PL_W; idx += 256) {
        const int rr = idx / PL_W, cc = idx - rr * PL_W;
        const int r = R0 - 2 + rr, c = C0 - 2 + cc;
        lab[rr][cc] = (r >= 0 && r < H && c >= 0 && c < W) ? g[rowoff(r, W) + c] : -1;
    }
    __syncthreads();
    // border bit: a pixel of a label with a 4-neighbour of another label
    for (int idx = threadIdx.x; idx < PB_H * PB_W; idx += 256) {
        const int rr = idx / PB_W, cc = idx - rr * PB_W;
        const int l = lab[rr + 1][cc + 1];
        bb[rr][cc] = l > 0 && (lab[rr][cc + 1] != l || lab[rr + 2][cc + 1] != l || lab[rr + 1][cc] != l || lab[rr + 1][cc + 2] != l);
    }
    __syncthreads();
    const PerSlots ls{tags, cnt};
    // wave w walks rows 8 w .. 8 w + 7 of the tile, a lane one column: the border pixels of a vertical run of one label add
    // up in two registers
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    int cur = 0;
    unsigned lo = 0, hi = 0;
    for (int i = 0; i < 8; ++i) {
        const int rr = wv * 8 + i;
        if (R0 + rr >= H || C0 + lane >= W || !bb[rr + 1][lane + 1]) continue;
        const int l = lab[rr + 2][lane + 2];
        // neighbours of ANOTHER label never count (regionprops crops to the region's own pixels)
        auto on = [&](int dr, int dc) { return (int)(bb[rr + 1 + dr][lane + 1 + dc] && lab[rr + 2 + dr][lane + 2 + dc] == l); };
        const int v = 1 + 2 * (on(-1, 0) + on(1, 0) + on(0, -1) + on(0, 1)) + 10 * (on(-1, -1) + on(-1, 1) + on(1, -1) + on(1, 1));
        if (l != cur) {
            if (lo | hi) per_commit(ls, gout, overflow, b, nl, cap, cur, lo, hi);
            cur = l;
            lo = 0;
            hi = 0;
        }
        lo += (unsigned)((PM_ONE >> v) & 1ull) | ((unsigned)((PM_SQRT2 >> v) & 1ull) << 16);
        hi += (unsigned)((PM_MID >> v) & 1ull) | (1u << 16);
    }
    if (!(lo | hi)) cur = 0;
    // lanes next to each other with the same label are summed into the first of them
    const WaveSeg seg = wave_segment(cur);
    uint2 cnt2 = make_uint2(lo, hi);
    segment_reduce(
        cnt2, seg.remain, [](const uint2 &a, int off) { return make_uint2(__shfl_down(a.x, off), __shfl_down(a.y, off)); },
        [](uint2 &a, const uint2 &o) { a.x += o.x; a.y += o.y; });
    if (seg.head && cur > 0) per_commit(ls, gout, overflow, b, nl, cap, cur, cnt2.x, cnt2.y);
    __syncthreads();
    // flush, four lanes per slot (columns 3..6 of the row)
    for (int base = 0; base < LABEL_SLOTS; base += 64) {
        const int i = base + (int)(threadIdx.x >> 2), f = threadIdx.x & 3;
        const int l = tags[i];
        if (l == 0) continue;
        const unsigned v = (unsigned)cnt[i][f];
        if (v) atomicAdd((unsigned long long *)(gout + (int64_t)(l - 1) * 8 + 3 + f), (unsigned long long)v);
    }
}

// ---- derived values
// a * b - c * d, exact (|a b|, |c d| < 2^126), as a float64: at most two roundings, none while the value fits 53 bits
__device__ __forceinline__ double exact_det(long long a, long long b, long long c, long long d)
{
    const __int128 x = (__int128)a * b - (__int128)c * d;
    const bool neg = x < 0;
    const unsigned __int128 u = neg ? (unsigned __int128)(-x) : (unsigned __int128)x;
    const double v = (double)(unsigned long long)(u >> 64) * 18446744073709551616.0 + (double)(unsigned long long)u;
    return neg ? -v : v;
}

__global__ void __launch_bounds__(256) shape_properties_kernel(const long long *__restrict__ stats, const long long *__restrict__ shape,
                                                                const int *__restrict__ counts, double *__restrict__ out, int cap)
{
    const int b = blockIdx.y;
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= min(counts[b], cap)) return;
    const long long *st = stats + ((int64_t)b * cap + l) * 8, *sh = shape + ((int64_t)b * cap + l) * 8;
    double *o = out + ((int64_t)b * cap + l) * 12;
    const long long A = st[0], sr = st[1], sc = st[2];
    if (A <= 0) {  // a label without a pixel has no shape
        for (int k = 0; k < 12; ++k) o[k] = __builtin_nan("");
        return;
    }
    const double a2 = (double)A * (double)A;
    const double P = exact_det(A, sh[0], sr, sr) / a2, R = exact_det(A, sh[1], sr, sc) / a2, Q = exact_det(A, sh[2], sc, sc) / a2;
    const double ta = Q, tb = -R, tc = P;  // inertia tensor [[a, b], [b, c]]
    const double root = sqrt((P - Q) * (P - Q) + 4.0 * R * R);
    const double l1 = ((P + Q) + root) / 2.0;
    double l2 = ((P + Q) - root) / 2.0;
    if (l2 < 0.0) l2 = 0.0;
    const double pi = 3.141592653589793;
    o[0] = ta; o[1] = tb; o[2] = tc;
    o[3] = l1; o[4] = l2;
    o[5] = 4.0 * sqrt(l1);
    o[6] = 4.0 * sqrt(l2);
    o[7] = l1 == 0.0 ? 0.0 : sqrt(1.0 - l2 / l1);
    o[8] = (ta - tc == 0.0) ? (tb < 0.0 ? -pi / 4.0 : pi / 4.0) : 0.5 * atan2(-2.0 * tb, tc - ta);
    o[9] = sqrt(4.0 * (double)A / pi);
    o[10] = (double)A / (double)((st[5] - st[3]) * (st[6] - st[4]));
    const double s2 = 1.4142135623730951;
    o[11] = (double)sh[3] + (double)sh[4] * s2 + (double)sh[5] * ((1.0 + s2) / 2.0);
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_region_shape_workspace_bytes(int B, int H, int W)
{
    if (!check_shape(B, H, W)) return 0;
    return carved_bytes(shape_carve, B);
}

int pcseg_region_shape(const int32_t *labels, const int32_t *counts, int64_t *shape_out, int32_t *overflow, int B, int H, int W,
                       int cap, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels && counts && shape_out && workspace && check_shape(B, H, W) && cap >= 1 && B <= 65535, "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const ShWorkspace w = shape_carve(cv, B);
    if (!cv.fits("region_shape")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    long long *out = (long long *)shape_out;
    PCSEG_LAUNCH(shape_init_kernel, dim3((unsigned)(((int64_t)cap * 8 + 255) / 256), B), dim3(256), 0, s, out, counts, w.nrows,
                 overflow, cap);
    PCSEG_CHECK_LAUNCH();
    const dim3 mgrid((W + 1023) / 1024, (H + RUN_ROWS - 1) / RUN_ROWS, B);
    if (W % 4 == 0 && ((uintptr_t)labels & 15) == 0)
        PCSEG_LAUNCH(shape_moments_kernel<true>, mgrid, dim3(256), 0, s, labels, (const int *)w.nrows, H, W, cap, out, overflow);
    else
        PCSEG_LAUNCH(shape_moments_kernel<false>, mgrid, dim3(256), 0, s, labels, (const int *)w.nrows, H, W, cap, out, overflow);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(shape_perimeter_kernel, dim3((W + PT_W - 1) / PT_W, (H + PT_H - 1) / PT_H, B), dim3(256), 0, s, labels,
                 (const int *)w.nrows, H, W, cap, out, overflow);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_shape_properties(const int64_t *stats, const int64_t *shape, const int32_t *counts, double *out, int B, int cap,
                           pcseg_stream_t stream)
{
    PCSEG_REQUIRE(stats && shape && counts && out && B >= 1 && B <= 65535 && cap >= 1, "bad arguments");
    PCSEG_LAUNCH(shape_properties_kernel, dim3((cap + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, (const long long *)stats,
                 (const long long *)shape, counts, out, cap);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
