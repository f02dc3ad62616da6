// Local neighbourhoods (include/pcseg_local.h): for every query pixel the set pixels in each distance ring around it, per set,
// and for every point the other points of each slot in each distance bin.  The per-cell marks of the frame-wide statistics of
// window_pairs.hip and neighbours.hip: summed over the window's pixels the ring counts are pcseg_window_pairs' bins, summed over
// a slot's points the point counts are pcseg_point_neighbours' pair histogram.
//
// pcseg_disk_counts works on BIT WORDS with a running count: per (frame, set, row) WW + 1 cells {pre, bits}, WW = ceil(W / 32),
// bits = the set's pixels at columns 32 w .. 32 w + 31 (bit j = column 32 w + j, 0 at columns >= W), pre = the set's pixels of
// the row at columns < 32 w; cell WW = {the row's total, 0}.  The set pixels of a row at columns < x, 0 <= x <= W, are
//     P(x) = pre[x >> 5] + popcount(bits[x >> 5] & ((1 << (x & 31)) - 1)):
// one 8-byte load, one mask, one v_bcnt.  The pixels of the DISK d2 < thr[k + 1] on the row dy of a query at (pr, pc) are
// P(pc + h + 1) - P(pc - h) with the half-width h = h_k(|dy|) = floor(sqrt(thr[k + 1] - 1 - dy^2)) (none when dy^2 >= thr[k + 1]),
// both columns clipped to [0, W]; ring k = disk k - disk k - 1.
//
// Launches (all asynchronous, no host read):
//   lc_pack_kernel       one wave per image row: byte -> C bit words per 64 columns with ballots, the running count of
//                        set c in lane c; the sets' areas by integer atomics, one per row and set
//   lc_halfwidth_kernel  the table h[|dy|][k], (R + 1, m) int16, -1 = the disk misses the row: a float square root corrected
//                        against the defining inequality h^2 <= t < (h + 1)^2 in integers.  The same for every query
//   lc_walk_kernel       one wave per query.  A lane owns one bin of a chunk of KL = min(64, 2^ceil(log2 m)) bins and one of
//                        RL = 64 / KL row phases; it walks its rows dy (clipped to the image) and adds the disk's pixels of all
//                        C sets to C registers.  The row phases are summed with butterflies, the ring is the difference to the
//                        lane below (the chunk before: a carried scalar), and the lanes of phase 0 write counts[i, c, k]: one
//                        coalesced store per (query, set, bin).  No LDS, no atomics: nothing depends on scheduling
//   lc_points_kernel     one wave per point: its lanes stride over the frame's points (coalesced, shared by the frame's waves in
//                        L2), d2 and the bin as nb_scan_tile computes them, counts into an LDS row of the wave (K m integers),
//                        then one store per (point, slot, bin)
#include "table_common.h"

#include "../../include/pcseg_local.h"

namespace pcseg {

constexpr int LC_THREADS = 256;                 // four waves: four queries (or points) per block
constexpr int LC_WAVES = LC_THREADS / WAVE;
constexpr int LC_MAX_SETS = 8;
constexpr int LC_POINTS_LDS = 64 * 1024;        // above it a block of lc_points_kernel has two waves

struct LcGeom {
    int B, C, H, W;
    int WW1;     // cells per (set, row): ceil(W / 32) + 1
    int R, m;
    int KL, RL;  // bin lanes and row phases of a wave: KL RL = 64
};

static LcGeom lc_geom(int B, int C, int H, int W, int n_edges, int64_t reach)
{
    LcGeom g;
    g.B = B; g.C = C; g.H = H; g.W = W;
    g.WW1 = (W + 31) / 32 + 1;
    g.R = (int)reach;
    g.m = n_edges - 1;
    g.KL = 1;
    while (g.KL < WAVE && g.KL < g.m) g.KL *= 2;
    g.RL = WAVE / g.KL;
    return g;
}

// cells[((b C + c) H + y) WW1 + w] = {pre, bits}
__global__ void __launch_bounds__(LC_THREADS) lc_pack_kernel(const uint8_t *__restrict__ in, uint2 *__restrict__ cells,
                                                              unsigned long long *__restrict__ area, int64_t rows, LcGeom g)
{
    const int lane = lane_id();
    const int chunks = (g.W + 63) >> 6, WW = g.WW1 - 1;
    for (int64_t row = (int64_t)blockIdx.x * LC_WAVES + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * LC_WAVES) {
        const int64_t b = row / g.H;
        const int y = (int)(row - b * g.H);
        const uint8_t *src = in + row * g.W;
        uint2 *dst = cells + ((b * g.C) * g.H + y) * g.WW1;  // set 0; set c: + c H WW1
        const int64_t set_stride = (int64_t)g.H * g.WW1;
        unsigned run = 0;  // lane c: the pixels of set c to the left of the chunk
        for (int ch = 0; ch < chunks; ++ch) {
            const int col = ch * 64 + lane;
            const unsigned v = col < g.W ? src[col] : 0u;
#pragma unroll
            for (int c = 0; c < LC_MAX_SETS; ++c) {
                if (c >= g.C) break;
                const unsigned long long mk = __ballot((v >> c) & 1u);
                const unsigned lo = (unsigned)mk, hi = (unsigned)(mk >> 32), before = __shfl(run, c);
                if (lane == 0) dst[c * set_stride + 2 * ch] = make_uint2(before, lo);
                if (lane == 1 && 2 * ch + 1 < WW) dst[c * set_stride + 2 * ch + 1] = make_uint2(before + __popc(lo), hi);
                if (lane == c) run += (unsigned)__popcll(mk);
            }
        }
        if (lane < g.C) {
            dst[lane * set_stride + WW] = make_uint2(run, 0u);
            if (run) atomicAdd(&area[b * g.C + lane], (unsigned long long)run);
        }
    }
}

// hw[ady * m + k] = floor(sqrt(thr[k + 1] - 1 - ady^2)), -1 where that is negative
__global__ void __launch_bounds__(256) lc_halfwidth_kernel(const long long *__restrict__ thr, int16_t *__restrict__ hw, int R, int m)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= (R + 1) * m) return;
    const int ady = idx / m, k = idx - ady * m;
    const long long t = thr[k + 1] - 1 - (long long)ady * ady;  // thr[k + 1] <= thr[m] <= (R + 1)^2
    int h = -1;
    if (t >= 0) {
        h = (int)sqrtf((float)t);
        while (h > 0 && (long long)h * h > t) --h;
        while ((long long)(h + 1) * (h + 1) <= t) ++h;  // h^2 <= t < (h + 1)^2; h <= R by the definition of R
    }
    hw[idx] = (int16_t)h;
}

// the set's pixels of a row at columns < x (0 <= x <= W); row: the (set, row)'s cells
__device__ __forceinline__ int lc_below(const uint2 *__restrict__ row, int x)
{
    const uint2 e = row[x >> 5];
    return (int)(e.x + __popc(e.y & ((1u << (x & 31)) - 1u)));
}

__global__ void __launch_bounds__(LC_THREADS) lc_walk_kernel(const uint2 *__restrict__ cells, const int16_t *__restrict__ hw,
                                                              const int32_t *__restrict__ queries, const int64_t *__restrict__ foff,
                                                              int64_t n, int32_t *__restrict__ counts, LcGeom g)
{
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * LC_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;  // wave-uniform
    const int b = last_le(foff, g.B, i);
    constexpr int far = 1 << 24;  // (a coordinate beyond the contract is pulled in: the arithmetic below cannot wrap)
    const int pr = min(max(queries[2 * i], -far), far), pc = min(max(queries[2 * i + 1], -far), far);
    const int dy0 = max(-g.R, -pr), dy1 = min(g.R, g.H - 1 - pr);  // the rows pr + dy inside the image (none: dy0 > dy1)
    const int kl = lane & (g.KL - 1), rl = lane / g.KL;
    const int64_t set_stride = (int64_t)g.H * g.WW1;
    const uint2 *frame = cells + (int64_t)b * g.C * set_stride;
    int32_t *out = counts + i * g.C * g.m;
    int carry[LC_MAX_SETS] = {0, 0, 0, 0, 0, 0, 0, 0};  // disk k - 1 of the chunk's first bin (wave-uniform)
    for (int kb = 0; kb < g.m; kb += g.KL) {
        const int k = kb + kl;
        int acc[LC_MAX_SETS] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (k < g.m) {
            for (int dy = dy0 + rl; dy <= dy1; dy += g.RL) {
                const int h = hw[(dy < 0 ? -dy : dy) * g.m + k];
                if (h < 0) continue;
                const int x0 = min(max(pc - h, 0), g.W), x1 = min(max(pc + h + 1, 0), g.W);
                if (x1 <= x0) continue;
                const uint2 *row = frame + (int64_t)(pr + dy) * g.WW1;
#pragma unroll
                for (int c = 0; c < LC_MAX_SETS; ++c) {
                    if (c >= g.C) break;
                    acc[c] += lc_below(row + c * set_stride, x1) - lc_below(row + c * set_stride, x0);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < LC_MAX_SETS; ++c) {
            if (c >= g.C) break;
            int s = acc[c];
            for (int o = WAVE / 2; o >= g.KL; o >>= 1) s += __shfl_xor(s, o);  // over the row phases
            int below = __shfl_up(s, 1);
            if (kl == 0) below = carry[c];
            if (rl == 0 && k < g.m) out[c * g.m + k] = s - below;
            carry[c] = __shfl(s, g.KL - 1);
        }
    }
}

__global__ void __launch_bounds__(LC_THREADS) lc_points_kernel(const double *__restrict__ xy, const int32_t *__restrict__ slot,
                                                                const int64_t *__restrict__ foff, const double *__restrict__ thr,
                                                                int64_t n, int B, int K, int m, int32_t *__restrict__ counts)
{
#pragma clang fp contract(off)  // each product and the sum rounded on their own (no FMA): nb_scan_tile's d2
    extern __shared__ __align__(16) unsigned char lc_lds[];
    double *s_thr = (double *)lc_lds;                                   // [m + 1]
    const int lane = lane_id(), wave = threadIdx.x / WAVE, waves = blockDim.x / WAVE;
    unsigned *h = (unsigned *)(s_thr + m + 1) + (size_t)wave * K * m;  // [K][m] of this wave
    for (int k = threadIdx.x; k <= m; k += blockDim.x) s_thr[k] = thr[k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * waves + wave;
    if (i >= n) return;  // wave-uniform; no barrier below
    int32_t *row = counts + i * K * m;
    const int qs = slot[i];
    if (qs < 0 || qs >= K) {
        for (int e = lane; e < K * m; e += WAVE) row[e] = -1;
        return;
    }
    // h is private to this wave64, and the LDS operations of one wave are carried out in the order they are issued: the
    // fences below only keep the compiler from moving them.  Rows shared between waves would need barriers instead
    for (int e = lane; e < K * m; e += WAVE) h[e] = 0;
    __threadfence_block();
    const int b = last_le(foff, B, i);
    const int64_t f0 = foff[b], f1 = foff[b + 1];
    const double qx = xy[2 * i], qy = xy[2 * i + 1], tlast = s_thr[m];
    for (int64_t j = f0 + lane; j < f1; j += WAVE) {
        const int t = slot[j];
        if (j == i || t < 0 || t >= K) continue;
        const double dx = qx - xy[2 * j], dy = qy - xy[2 * j + 1];
        const double d2 = dx * dx + dy * dy;
        // thr[bin] <= d2 < thr[bin + 1]
        if (d2 < tlast) atomicAdd(&h[t * m + last_le(s_thr, m, d2)], 1u);
    }
    __threadfence_block();
    for (int e = lane; e < K * m; e += WAVE) row[e] = (int32_t)h[e];
}

struct LcWorkspace {
    uint2 *cells;
    long long *thr;
    int16_t *hw;
};

static LcWorkspace lc_carve(Carver &cv, const LcGeom &g)
{
    LcWorkspace w;
    w.cells = cv.take<uint2>((size_t)g.B * g.C * g.H * g.WW1);
    w.thr = cv.take<long long>((size_t)g.m + 1);
    w.hw = cv.take<int16_t>((size_t)(g.R + 1) * g.m);
    return w;
}

static bool lc_shape_ok(int B, int C, int H, int W, int n_edges)
{
    return check_shape(B, H, W) && B <= 65535 && C >= 1 && C <= LC_MAX_SETS && n_edges >= 2 && n_edges <= MAX_HIST_BINS + 1;
}

struct LcPointWorkspace {
    double *thr;
};

static LcPointWorkspace lc_point_carve(Carver &cv, int n_edges)
{
    LcPointWorkspace w;
    w.thr = cv.take<double>((size_t)n_edges);
    return w;
}

static bool lc_points_ok(int64_t n, int B, int K, int n_edges)
{
    return n >= 0 && n < ((int64_t)1 << 24) && B >= 1 && K >= 1 && K <= MAX_TYPE_SLOTS && n_edges >= 2 && n_edges <= MAX_HIST_BINS + 1;
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

int pcseg_local_rows(void) { return WAVE; }
int pcseg_local_bins(void) { return WAVE; }
int pcseg_local_point_tile(void) { return WAVE; }

size_t pcseg_disk_counts_workspace_bytes(int B, int C, int H, int W, int n_edges, int64_t reach)
{
    if (!lc_shape_ok(B, C, H, W, n_edges) || reach < 0 || reach > PCSEG_WINDOW_MAX_REACH) return 0;
    return carved_bytes(lc_carve, lc_geom(B, C, H, W, n_edges, reach));
}

int pcseg_disk_counts(const uint8_t *planes, int B, int C, int H, int W, const int32_t *queries, const int64_t *frame_offsets,
                      int64_t n_queries, double scale, const double *edges, int n_edges, int32_t *counts, int64_t *area,
                      void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(planes && frame_offsets && area && workspace && lc_shape_ok(B, C, H, W, n_edges) && n_queries >= 0 &&
                      n_queries < ((int64_t)1 << 31) && (n_queries == 0 || (queries && counts)),
                  "bad arguments");
    int64_t thr[MAX_HIST_BINS + 1], reach = 0;
    int rc = pcseg_surface_thresholds(edges, n_edges, scale, thr);  // (checks edges and scale)
    if (rc != PCSEG_OK) return rc;
    rc = pcseg_window_reach(edges, n_edges, scale, &reach);
    if (rc != PCSEG_OK) return rc;
    PCSEG_REQUIRE(reach <= PCSEG_WINDOW_MAX_REACH, "the reach of the last edge is above PCSEG_WINDOW_MAX_REACH");
    const LcGeom g = lc_geom(B, C, H, W, n_edges, reach);
    Carver cv(workspace, workspace_bytes);
    const LcWorkspace w = lc_carve(cv, g);
    if (!cv.fits("disk_counts")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    PCSEG_CHECK_HIP(hipMemsetAsync(area, 0, sizeof(int64_t) * (size_t)B * C, s));
    const int64_t rows = (int64_t)B * H;
    const int64_t pack_blocks = (rows + LC_WAVES - 1) / LC_WAVES;
    PCSEG_LAUNCH(lc_pack_kernel, dim3((unsigned)(pack_blocks > 65536 ? 65536 : pack_blocks)), dim3(LC_THREADS), 0, s, planes, w.cells,
                 (unsigned long long *)area, rows, g);
    PCSEG_CHECK_LAUNCH();
    if (n_queries == 0) return PCSEG_OK;
    const int64_t *thr_p = thr;
    const int up = upload_values(s, w.thr, n_edges, [=](int k) { return (long long)thr_p[k]; });
    if (up != PCSEG_OK) return up;
    const int cells_hw = (g.R + 1) * g.m;
    PCSEG_LAUNCH(lc_halfwidth_kernel, dim3((unsigned)((cells_hw + 255) / 256)), dim3(256), 0, s, (const long long *)w.thr, w.hw, g.R, g.m);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(lc_walk_kernel, dim3((unsigned)((n_queries + LC_WAVES - 1) / LC_WAVES)), dim3(LC_THREADS), 0, s, (const uint2 *)w.cells,
                 (const int16_t *)w.hw, queries, frame_offsets, n_queries, counts, g);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

size_t pcseg_point_counts_workspace_bytes(int64_t n_points, int B, int K, int n_edges)
{
    if (!lc_points_ok(n_points, B, K, n_edges)) return 0;
    return carved_bytes(lc_point_carve, n_edges);
}

int pcseg_point_counts(const double *xy, const int32_t *slot, const int64_t *frame_offsets, int64_t n_points, int B, int K,
                       double scale, const double *edges, int n_edges, int32_t *counts, void *workspace, size_t workspace_bytes,
                       pcseg_stream_t stream)
{
    PCSEG_REQUIRE(xy && slot && frame_offsets && counts && workspace && lc_points_ok(n_points, B, K, n_edges) && scale > 0.0 &&
                      std::isfinite(scale) && hist_edges_ok(edges, n_edges),
                  "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const LcPointWorkspace w = lc_point_carve(cv, n_edges);
    if (!cv.fits("point_counts")) return PCSEG_ERR_WORKSPACE;
    if (n_points == 0) return PCSEG_OK;
    hipStream_t s = (hipStream_t)stream;
    const int m = n_edges - 1;
    const int rc = upload_values(s, w.thr, n_edges, [=](int k) { return d2_threshold(edges[k], scale); });
    if (rc != PCSEG_OK) return rc;
    const size_t per_wave = sizeof(unsigned) * (size_t)K * m, fixed = sizeof(double) * (size_t)(m + 1);
    const int waves = fixed + LC_WAVES * per_wave <= (size_t)LC_POINTS_LDS ? LC_WAVES : 2;  // (K m <= 4096: two waves fit 41 KB)
    PCSEG_LAUNCH(lc_points_kernel, dim3((unsigned)((n_points + waves - 1) / waves)), dim3(waves * WAVE), fixed + waves * per_wave, s, xy,
                 slot, frame_offsets, (const double *)w.thr, n_points, B, K, m, counts);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
