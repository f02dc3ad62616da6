// Per-ROI convexity table: convex area, Feret diameter and Euler number of every label of an int32 label image (what tells
// one cell from a clump: tiff_analysis.py:776-781 counts the cells of a cluster as area // mean cell area,
// refine_boundaries.py:5-7 expects clusters the watershed does not split; HCN_nanosims_rois_activity_distance_5iso_YG.m:104,
// 173 ask for regionprops 'all').  scikit-image 0.18.3 conventions; every value an exact INTEGER (include/pcseg.h).
//
// One ROI is one work item that reads ITS OWN BOUNDING BOX (from the region table) out of the label image: nothing is shared
// between ROIs, so there is no atomic on global memory, no order dependence and no span array sized by the frame.
//   hull_init_kernel    overflow[b] = counts[b] > cap, the frame's list of tall ROIs emptied
//   hull_small_kernel   one WAVE per label: ROIs of at most 64 rows, spans and hull chains in LDS; taller ones are appended to
//                       the frame's list
//   hull_tall_kernel    blocks of 16 waves walk the list (the particle ROI: ~0.6 H rows), the same steps with the spans and
//                       chains in a slice of the workspace
// The steps of a ROI of h rows (doubled coordinates: pixel (r, c) owns the points (2r +- 1, 2c), (2r, 2c +- 1)):
//   1 scan    a wave takes a stripe of rows; per row and 63-column chunk ONE ballot of (pixel == label) gives the row's
//             leftmost / rightmost column and, with the ballot of the row above, the 2 x 2 window counts Q1, Q3, QD of the Euler
//             number as population counts of wave-uniform masks
//   2 hull    the hull's left side is the lower convex envelope of k -> smallest point column in doubled row k (2h + 1 rows,
//             from the spans), its right side the upper envelope of the largest: two monotone chains, one lane each
//   3 rows    a lane per pixel row: the hull cuts the interval [ceil(left / 2), floor(right / 2)] of pixel centres, from exact
//             64-bit integer divisions; their lengths add up to convex_area, the intervals ARE the convex image
//   4 hull    of the convex image's own points, by step 2 on its intervals (it reaches further than the label's hull)
//   5 feret   the largest squared distance over all pairs of that hull's vertices
#include "common.h"

// every operation of the derived columns rounded on its own (no FMA), as shape.hip
#pragma clang fp contract(off)

namespace pcseg {

constexpr int HU_SMALL_H = 64;        // rows of a ROI the one-wave kernel takes
constexpr int HU_TALL_THREADS = 1024;
constexpr int HU_ROWS = 8;            // rows a wave has in flight per step of the scan
constexpr int HU_NONE = 0x3FFFFFFF;   // a row without pixel of the label: left = HU_NONE, right = -HU_NONE

static int hull_tall_blocks(int B) { return B >= 256 ? 4 : (B <= 16 ? 64 : 1024 / B); }
// bytes of the spans and chains of one tall ROI: two chains of at most 2 H + 1 (k, value) vertices, two span arrays
static size_t hull_slice_bytes(int H) { return align_up(2 * (size_t)(2 * H + 1) * sizeof(int2) + 2 * (size_t)H * sizeof(int)); }

struct HuWorkspace {
    int *ntall;   // [B] tall ROIs of the frame
    int *tall;    // [B, cap] their labels
    char *slices; // [B, hull_tall_blocks(B)] of hull_slice_bytes(H)
};

// the ONE layout of the workspace
static HuWorkspace hull_carve(Carver &cv, int B, int H, int cap)
{
    HuWorkspace w;
    w.ntall = cv.take<int>((size_t)B);
    w.tall = cv.take<int>((size_t)B * cap);
    w.slices = cv.take<char>((size_t)B * hull_tall_blocks(B) * hull_slice_bytes(H));
    return w;
}

struct HuScratch {
    int *a, *b;          // [h] leftmost / rightmost column per row: of the label, after step 3 of the convex image
    int2 *left, *right;  // hull chains: (k, value) vertices; the right chain holds NEGATED columns (one envelope routine)
};

struct HuShared {
    unsigned long long area, feret;
    int q[3];
    int n[2];
};

__global__ void __launch_bounds__(256) hull_init_kernel(const int *__restrict__ counts, int *__restrict__ ntall,
                                                         int *__restrict__ overflow, int B, int cap)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    ntall[b] = 0;
    if (overflow) overflow[b] = counts[b] > cap;
}

// smallest (side 0) / negated largest (side 1) point column in doubled row k of the box (k = 0 .. 2h; HU_NONE: no point):
// odd k = 2j + 1 is the centre row of pixel row j (points 2a - 1, 2b + 1), even k lies between the pixel rows k/2 - 1 and k/2
__device__ __forceinline__ int hull_chain_value(const int *a, const int *b, int h, int k, int side)
{
    const int j = k >> 1;
    if (side == 0) {
        if (k & 1) return a[j] >= HU_NONE ? HU_NONE : 2 * a[j] - 1;
        int x = HU_NONE;
        if (j > 0) x = min(x, a[j - 1]);
        if (j < h) x = min(x, a[j]);
        return x >= HU_NONE ? HU_NONE : 2 * x;
    }
    if (k & 1) return b[j] <= -HU_NONE ? HU_NONE : -(2 * b[j] + 1);
    int x = -HU_NONE;
    if (j > 0) x = max(x, b[j - 1]);
    if (j < h) x = max(x, b[j]);
    return x <= -HU_NONE ? HU_NONE : -2 * x;
}

// lower convex envelope of k -> hull_chain_value (Andrew's monotone chain, one lane): strict vertices into S, their number back
__device__ int hull_build_chain(const int *a, const int *b, int h, int side, int2 *S)
{
    int n = 0;
    for (int k = 0; k <= 2 * h; ++k) {
        const int v = hull_chain_value(a, b, h, k, side);
        if (v == HU_NONE) continue;
        while (n >= 2) {
            const int2 p0 = S[n - 2], p1 = S[n - 1];
            // p1 on or above the line p0 -> (k, v): not a vertex
            if ((long long)(p1.y - p0.y) * (k - p0.x) >= (long long)(v - p0.y) * (p1.x - p0.x)) --n;
            else break;
        }
        S[n++] = make_int2(k, v);
    }
    return n;
}

// ceil(envelope(k) / 2) of a chain, exact; false when k lies outside the chain
__device__ __forceinline__ bool hull_ceil_half(const int2 *S, int n, int k, long long &q)
{
    if (n == 0 || k < S[0].x || k > S[n - 1].x) return false;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (S[mid].x <= k) lo = mid;
        else hi = mid - 1;
    }
    const int2 p0 = S[lo];
    long long num = p0.y, den = 2;
    if (p0.x != k) {
        const int2 p1 = S[lo + 1];
        const long long dk = p1.x - p0.x;
        num = (long long)p0.y * dk + (long long)(k - p0.x) * (p1.y - p0.y);
        den = 2 * dk;
    }
    q = num / den;
    if (num % den > 0) ++q;
    return true;
}

// all NT threads of the block: the ROI `l` of the box [r0, r1) x [c0, c1) (inside the frame, not empty) -> o[0..3]
template <int NT>
__device__ void hull_roi(const int *__restrict__ lab, int H, int W, int l, int r0, int c0, int r1, int c1, const HuScratch &s,
                         HuShared &sh, long long *__restrict__ o)
{
    constexpr int NW = NT / WAVE;
    const int tid = threadIdx.x, lane = lane_id(), wv = tid >> 6;
    const int h = r1 - r0;
    if (tid == 0) {
        sh.area = 0; sh.feret = 0;
        sh.q[0] = 0; sh.q[1] = 0; sh.q[2] = 0;
    }
    for (int i = tid; i < h; i += NT) {
        s.a[i] = HU_NONE;
        s.b[i] = -HU_NONE;
    }
    __syncthreads();
    // ---- 1 scan: wave wv owns the window rows [ws, we) (a window row wr covers the pixel rows wr and wr + 1; wr = r0 - 1 ..
    // r1 - 1), lane j of a chunk the window columns base + j, base + j + 1 (j < 63; lane 63 only lends its pixel)
    {
        const int per = (h + 1 + NW - 1) / NW;
        const int ws = r0 - 1 + wv * per, we = min(ws + per, r1);
        int q1 = 0, q3 = 0, qd = 0;
        for (int base = c0 - 1; base < c1 && ws < we; base += 63) {
            const int c = base + lane;
            const bool cin = c >= 0 && c < W && c <= c1;
            int top = 0;
            if (cin && ws >= 0) top = lab[rowoff(ws, W) + c];
            unsigned long long T = __ballot(top == l);
            for (int pr = ws + 1; pr <= we; pr += HU_ROWS) {
                int v[HU_ROWS];
#pragma unroll
                for (int u = 0; u < HU_ROWS; ++u) {
                    const int r = pr + u;
                    v[u] = 0;
                    if (cin && r <= we && r < H) v[u] = lab[rowoff(r, W) + c];
                }
#pragma unroll
                for (int u = 0; u < HU_ROWS; ++u) {
                    const int r = pr + u;
                    if (r > we) break;
                    const unsigned long long Bm = __ballot(v[u] == l);
                    const unsigned long long t1 = T >> 1, b1 = Bm >> 1, valid = ~(1ull << 63);
                    const unsigned long long odd = T ^ t1 ^ Bm ^ b1;  // one or three of the four set
                    const unsigned long long two = (T & t1) | (T & Bm) | (T & b1) | (t1 & Bm) | (t1 & b1) | (Bm & b1);  // >= 2
                    q1 += __popcll(odd & ~two & valid);
                    q3 += __popcll(odd & two & valid);
                    qd += __popcll(((T & b1 & ~t1 & ~Bm) | (t1 & Bm & ~T & ~b1)) & valid);
                    if (Bm && r < r1 && lane == 0) {  // (this wave alone touches row r's span)
                        const int i = r - r0;
                        s.a[i] = min(s.a[i], base + (__ffsll((long long)Bm) - 1));
                        s.b[i] = max(s.b[i], base + 63 - __clzll((long long)Bm));
                    }
                    T = Bm;
                }
            }
        }
        if (lane == 0 && (q1 | q3 | qd)) {
            atomicAdd(&sh.q[0], q1);
            atomicAdd(&sh.q[1], q3);
            atomicAdd(&sh.q[2], qd);
        }
    }
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        // ---- 2 / 4 hull: one lane per chain (in two waves where the block has them)
        constexpr int RIGHT = NT > WAVE ? WAVE : 1;
        if (tid == 0) sh.n[0] = hull_build_chain(s.a, s.b, h, 0, s.left);
        if (tid == RIGHT) sh.n[1] = hull_build_chain(s.a, s.b, h, 1, s.right);
        __syncthreads();
        if (pass == 1) break;
        // ---- 3 rows
        const int nl = sh.n[0], nr = sh.n[1];
        long long area = 0;
        for (int j = tid; j < h; j += NT) {
            long long lo = 0, hi = 0;
            const bool in = hull_ceil_half(s.left, nl, 2 * j + 1, lo) && hull_ceil_half(s.right, nr, 2 * j + 1, hi);
            hi = -hi;  // floor(right / 2) = -ceil(-right / 2)
            const bool some = in && hi >= lo;
            s.a[j] = some ? (int)lo : HU_NONE;
            s.b[j] = some ? (int)hi : -HU_NONE;
            if (some) area += hi - lo + 1;
        }
        for (int off = 32; off > 0; off >>= 1) area += __shfl_down(area, off);
        if (lane == 0 && area) atomicAdd(&sh.area, (unsigned long long)area);
        __syncthreads();
    }
    // ---- 5 feret: all pairs of the second hull's vertices (every lane reads the same partner: an LDS broadcast)
    {
        const int nl = sh.n[0], nv = sh.n[0] + sh.n[1];
        unsigned long long best = 0;
        for (int i = tid; i < nv; i += NT) {
            const int2 p = i < nl ? s.left[i] : s.right[i - nl];
            const long long pk = p.x, pv = i < nl ? p.y : -p.y;
            for (int j = 0; j < nv; ++j) {
                const int2 q = j < nl ? s.left[j] : s.right[j - nl];
                const long long dk = pk - q.x, dv = pv - (j < nl ? q.y : -q.y);
                best = max(best, (unsigned long long)(dk * dk + dv * dv));
            }
        }
        for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned long long)__shfl_down(best, off));
        if (lane == 0 && best) atomicMax(&sh.feret, best);
    }
    __syncthreads();
    if (tid == 0) {
        o[0] = (long long)sh.area;
        o[1] = (long long)sh.feret;
        o[2] = ((long long)sh.q[0] - sh.q[1] - 2ll * sh.q[2]) / 4;
        o[3] = 0;
    }
    __syncthreads();  // (the next ROI of this block resets sh)
}

struct HuBox {
    int r0, c0, r1, c1;
};

// the label's bounding box from its region row, held inside the frame whatever the row contains; false: nothing to look at
__device__ __forceinline__ bool hull_box(const long long *st, int H, int W, HuBox &bx)
{
    if (st[0] <= 0) return false;
    bx.r0 = (int)min(max(st[3], 0ll), (long long)H);
    bx.c0 = (int)min(max(st[4], 0ll), (long long)W);
    bx.r1 = (int)min(max(st[5], 0ll), (long long)H);
    bx.c1 = (int)min(max(st[6], 0ll), (long long)W);
    return bx.r1 > bx.r0 && bx.c1 > bx.c0;
}

__global__ void __launch_bounds__(WAVE) hull_small_kernel(const int *__restrict__ labels, const int *__restrict__ counts,
                                                           const long long *__restrict__ stats, long long *__restrict__ out,
                                                           int *__restrict__ ntall, int *__restrict__ tall, int H, int W, int cap)
{
    __shared__ int a[HU_SMALL_H], b[HU_SMALL_H];
    __shared__ int2 left[2 * HU_SMALL_H + 1], right[2 * HU_SMALL_H + 1];
    __shared__ HuShared sh;
    const int l = blockIdx.x + 1, f = blockIdx.y;
    if (l > min(counts[f], cap)) return;
    const int64_t row = (int64_t)f * cap + (l - 1);
    long long *o = out + row * 4;
    HuBox bx;
    if (!hull_box(stats + row * 8, H, W, bx)) {  // a label without pixel
        if (threadIdx.x < 4) o[threadIdx.x] = 0;
        return;
    }
    if (bx.r1 - bx.r0 > HU_SMALL_H) {
        if (threadIdx.x == 0) tall[(int64_t)f * cap + atomicAdd(&ntall[f], 1)] = l;  // (at most one entry per label: < cap)
        return;
    }
    const HuScratch s{a, b, left, right};
    hull_roi<WAVE>(labels + (int64_t)f * H * W, H, W, l, bx.r0, bx.c0, bx.r1, bx.c1, s, sh, o);
}

__global__ void __launch_bounds__(HU_TALL_THREADS) hull_tall_kernel(const int *__restrict__ labels,
                                                                     const long long *__restrict__ stats,
                                                                     long long *__restrict__ out, const int *__restrict__ ntall,
                                                                     const int *__restrict__ tall, char *__restrict__ slices,
                                                                     size_t slice_bytes, int H, int W, int cap)
{
    __shared__ HuShared sh;
    const int f = blockIdx.y;
    char *mine = slices + ((size_t)f * gridDim.x + blockIdx.x) * slice_bytes;
    HuScratch s;
    s.left = (int2 *)mine;
    s.right = s.left + (2 * H + 1);
    s.a = (int *)(s.right + (2 * H + 1));
    s.b = s.a + H;
    const int n = min(ntall[f], cap);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int l = tall[(int64_t)f * cap + i];
        const int64_t row = (int64_t)f * cap + (l - 1);
        HuBox bx;
        if (l < 1 || l > cap || !hull_box(stats + row * 8, H, W, bx)) continue;
        hull_roi<HU_TALL_THREADS>(labels + (int64_t)f * H * W, H, W, l, bx.r0, bx.c0, bx.r1, bx.c1, s, sh, out + row * 4);
    }
}

__global__ void __launch_bounds__(256) hull_properties_kernel(const long long *__restrict__ stats, const long long *__restrict__ hull,
                                                               const int *__restrict__ counts, double *__restrict__ out, int cap)
{
    const int b = blockIdx.y;
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= min(counts[b], cap)) return;
    const int64_t row = (int64_t)b * cap + l;
    const long long A = stats[row * 8];
    const long long *hu = hull + row * 4;
    double *o = out + row * 4;
    if (A <= 0) {  // a label without a pixel has no hull
        for (int k = 0; k < 4; ++k) o[k] = __builtin_nan("");
        return;
    }
    o[0] = (double)hu[0];
    o[1] = (double)A / (double)hu[0];
    o[2] = sqrt((double)hu[1] / 4.0);
    o[3] = (double)hu[2];
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_region_hull_workspace_bytes(int B, int H, int W, int cap)
{
    if (!check_shape(B, H, W) || cap < 1) return 0;
    return carved_bytes(hull_carve, B, H, cap);
}

int pcseg_region_hull(const int32_t *labels, const int32_t *counts, const int64_t *stats, int64_t *hull_out, int32_t *overflow, int B,
                      int H, int W, int cap, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels && counts && stats && hull_out && workspace && check_shape(B, H, W) && cap >= 1 && B <= 65535,
                  "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const HuWorkspace w = hull_carve(cv, B, H, cap);
    if (!cv.fits("region_hull")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    PCSEG_LAUNCH(hull_init_kernel, dim3((B + 255) / 256), dim3(256), 0, s, counts, w.ntall, overflow, B, cap);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(hull_small_kernel, dim3(cap, B), dim3(WAVE), 0, s, labels, counts, (const long long *)stats, (long long *)hull_out,
                 w.ntall, w.tall, H, W, cap);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(hull_tall_kernel, dim3(hull_tall_blocks(B), B), dim3(HU_TALL_THREADS), 0, s, labels, (const long long *)stats,
                 (long long *)hull_out, (const int *)w.ntall, (const int *)w.tall, w.slices, hull_slice_bytes(H), H, W, cap);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_hull_properties(const int64_t *stats, const int64_t *hull, const int32_t *counts, double *out, int B, int cap,
                          pcseg_stream_t stream)
{
    PCSEG_REQUIRE(stats && hull && counts && out && B >= 1 && B <= 65535 && cap >= 1, "bad arguments");
    PCSEG_LAUNCH(hull_properties_kernel, dim3((cap + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, (const long long *)stats,
                 (const long long *)hull, counts, out, cap);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
