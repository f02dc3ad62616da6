// Clustering against chance: exact window pair counts (include/pcseg_spatial.h).  For the window M of a frame -- the
// pixels in which a point can sit -- gamma(dy, dx) = #{(y, x) : M[y, x] and M[y + dy, x + dx]} is counted for every lag
// within the reach R of the last distance bin, and the lags are summed per bin: n points placed independently and
// uniformly on the A pixels of M have npairs * bin_k / A^2 pairs in bin k in expectation, exactly.
//
// Everything works on BIT WORDS (the layout of surface.hip): uint32 (B, H, WW), WW = ceil(W / 32), bit j of word w of a
// row = pixel column 32 w + j, bits at columns >= W are 0.  One AND and one popcount handle 32 pixel pairs.
//
// Launches (all asynchronous, no host read):
//   wp_pack_kernel    one wave per 64 pixels of a row: byte -> bit with a ballot; the frame's area by integer atomics
//   wp_lag_kernel     one block per (frame, dy, chunk of WP_ROWS rows y with y + dy < H).  The rows y of the chunk and
//                     the rows y + dy sit in LDS, the latter with `pad` zero words on both sides so that a negative dx
//                     needs no branch.  A lane owns one dx = 32 q + s, a wave 64 consecutive dx -- its lanes read at
//                     most three distinct q, and equal addresses broadcast --, and the block's four waves deal the
//                     (group of 64 dx, row) pairs among themselves.  Per word w of row y the lane forms
//                     alignbit(B[w + q + 1], B[w + q], s), ANDs it with A[w] (one address per wave) and adds the popcount
//                     to a register; B[w + q + 1] is the next word's B[w + q].  Only the words between the first and the
//                     last non-zero word of row y are walked.  Counts go to an LDS row of the block, then once per block
//                     and dx to gamma in the workspace (32-bit integer atomics: gamma <= H W < 2^30).
//   wp_bin_kernel     every lag once: its bin by a search over the m + 1 integer thresholds, dy > 0 counted twice (the
//                     other half plane), LDS histogram per block, one 64-bit global atomic per non-zero bin
//   wp_finish_kernel  one block per frame: n_px and over = A^2 - the bins
//   wp_lags_kernel    (lags wanted) gamma as int64 (B, R + 1, 2 R + 1), zero where the lag reaches beyond the image
#include "table_common.h"

#include "../../include/pcseg_spatial.h"

namespace pcseg {

constexpr int WP_ROWS = 16;      // rows y of a lag block: LDS = 4 (WP_ROWS (2 WW + 2 pad) + 2 Rx + 1 + 2 WP_ROWS) bytes
constexpr int WP_THREADS = 256;  // four waves share the rows
constexpr int64_t WP_MAX_REACH = PCSEG_WINDOW_MAX_REACH;

// the lags that can count anything in an H x W frame: |dy| <= Ry, |dx| <= Rx
struct WpGeom {
    int H, W, WW;
    int R;            // the reach of the bins
    int Ry, Rx, ndx;  // min(R, H - 1), min(R, W - 1), 2 Rx + 1
    int pad, bw;      // zero words on either side of a row y + dy, and its padded width: q in [-(pad - 1), pad - 1]
    int groups;       // groups of 64 dx
    size_t lds() const { return sizeof(uint32_t) * ((size_t)WP_ROWS * (WW + bw) + ndx + 2 * WP_ROWS); }
};

static WpGeom wp_geom(int H, int W, int64_t reach)
{
    WpGeom g;
    g.H = H; g.W = W; g.WW = (W + 31) / 32;
    g.R = (int)reach;
    g.Ry = g.R < H - 1 ? g.R : H - 1;
    g.Rx = g.R < W - 1 ? g.R : W - 1;
    g.ndx = 2 * g.Rx + 1;
    g.pad = (g.Rx + 31) / 32 + 1;
    g.bw = g.WW + 2 * g.pad;
    g.groups = (g.ndx + WAVE - 1) / WAVE;
    return g;
}

__global__ void __launch_bounds__(256) wp_pack_kernel(const uint8_t *__restrict__ in, uint32_t *__restrict__ bits,
                                                       unsigned long long *__restrict__ area, int64_t rows, int H, int W, int WW)
{
    const int lane = lane_id();
    const int chunks = (W + 63) >> 6;
    const int64_t total = rows * chunks;
    for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < total; it += (int64_t)gridDim.x * 4) {
        const int64_t row = it / chunks;
        const int c = (int)(it - row * chunks);
        const int col = c * 64 + lane;
        const bool bit = col < W && in[row * W + col] != 0;
        const unsigned long long m = __ballot(bit);
        if (lane == 0) {
            bits[row * WW + 2 * c] = (uint32_t)m;
            if (m) atomicAdd(&area[row / H], (unsigned long long)__popcll(m));
        }
        if (lane == 1 && 2 * c + 1 < WW) bits[row * WW + 2 * c + 1] = (uint32_t)(m >> 32);
    }
}

__global__ void __launch_bounds__(WP_THREADS) wp_lag_kernel(const uint32_t *__restrict__ bits, unsigned *__restrict__ gamma, WpGeom g)
{
    extern __shared__ __align__(16) unsigned char wp_lds[];
    uint32_t *sA = (uint32_t *)wp_lds;       // [WP_ROWS][WW]  rows y
    uint32_t *sB = sA + WP_ROWS * g.WW;      // [WP_ROWS][bw]  rows y + dy, padded
    unsigned *s_cnt = sB + WP_ROWS * g.bw;   // [ndx]
    int *s_lo = (int *)(s_cnt + g.ndx), *s_hi = s_lo + WP_ROWS;  // first and last non-zero word of a row y
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    const int b = blockIdx.z, dy = blockIdx.y, y0 = blockIdx.x * WP_ROWS;
    const int WW = g.WW, bw = g.bw, pad = g.pad;
    const int nrows = min(WP_ROWS, g.H - dy - y0);  // the chunk's rows y with y + dy inside the image
    if (nrows <= 0) return;                         // block-uniform
    const uint32_t *fb = bits + (int64_t)b * g.H * WW;
    for (int e = tid; e < nrows * WW; e += WP_THREADS) sA[e] = fb[(int64_t)y0 * WW + e];
    for (int e = tid; e < nrows * bw; e += WP_THREADS) {
        const int r = e / bw, w = e - r * bw - pad;
        sB[e] = (w >= 0 && w < WW) ? fb[(int64_t)(y0 + r + dy) * WW + w] : 0u;
    }
    for (int e = tid; e < g.ndx; e += WP_THREADS) s_cnt[e] = 0;
    __syncthreads();
    for (int r = wave; r < nrows; r += WP_THREADS / WAVE) {
        int lo = WW, hi = -1;
        for (int w = lane; w < WW; w += WAVE)
            if (sA[r * WW + w]) {
                lo = min(lo, w);
                hi = max(hi, w);
            }
        for (int o = 32; o >= 1; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o));
            hi = max(hi, __shfl_xor(hi, o));
        }
        if (lane == 0) {
            s_lo[r] = lo;
            s_hi[r] = hi;
        }
    }
    __syncthreads();
    for (int item = wave; item < g.groups * nrows; item += WP_THREADS / WAVE) {  // wave-uniform
        const int grp = item / nrows, r = item - grp * nrows;
        const int wlo = __builtin_amdgcn_readfirstlane(s_lo[r]), whi = __builtin_amdgcn_readfirstlane(s_hi[r]);
        if (whi < 0) continue;  // an empty row y
        const int dxi = grp * WAVE + lane;
        const int dx = min(dxi, g.ndx - 1) - g.Rx;  // (the lanes beyond the last dx walk it once more and add nothing)
        const int q = dx >> 5;                      // floor(dx / 32), -(pad - 1) <= q <= pad - 1
        const unsigned s = (unsigned)dx & 31u;
        const uint32_t *a = sA + r * WW;
        const uint32_t *bp = sB + r * bw + pad + q;  // bp[w], bp[w + 1] for w in [0, WW): indices 1 .. bw - 1 of the row
        unsigned c = 0;
        uint32_t lo = bp[wlo];
        for (int w = wlo; w <= whi; ++w) {
            const uint32_t hi = bp[w + 1];
            // bit j = column 32 w + j + dx of row y + dy
            c += __popc(a[w] & __builtin_amdgcn_alignbit(hi, lo, s));
            lo = hi;
        }
        if (dxi < g.ndx && c) atomicAdd(&s_cnt[dxi], c);
    }
    __syncthreads();
    unsigned *grow = gamma + ((int64_t)b * (g.Ry + 1) + dy) * g.ndx;
    for (int e = tid; e < g.ndx; e += WP_THREADS) {
        const unsigned c = s_cnt[e];
        if (c) atomicAdd(&grow[e], c);
    }
}

// lags [blockIdx.x * per_block, + per_block) of frame blockIdx.y into hist[b][1 + k]
__global__ void __launch_bounds__(256) wp_bin_kernel(const unsigned *__restrict__ gamma, const long long *__restrict__ thr, int m,
                                                      unsigned long long *__restrict__ hist, int Ry, int Rx, int64_t per_block)
{
    extern __shared__ __align__(16) unsigned char wp_lds[];
    unsigned long long *s_h = (unsigned long long *)wp_lds;  // [m]
    const int b = blockIdx.y, ndx = 2 * Rx + 1;
    const int64_t total = (int64_t)(Ry + 1) * ndx;
    const int64_t first = per_block * blockIdx.x, last = min(total, first + per_block);
    for (int k = threadIdx.x; k < m; k += 256) s_h[k] = 0;
    __syncthreads();
    for (int64_t l = first + threadIdx.x; l < last; l += 256) {
        const unsigned c = gamma[b * total + l];
        if (!c) continue;
        const int dy = (int)(l / ndx), dx = (int)(l - (int64_t)dy * ndx) - Rx;
        const long long d2 = (long long)dy * dy + (long long)dx * dx;
        const int k = last_le(thr, m + 1, d2);  // thr[k] <= d2 < thr[k + 1] (thr[0] = 0; k = m: beyond the last edge)
        if (k < m) atomicAdd(&s_h[k], (unsigned long long)c * (dy > 0 ? 2u : 1u));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < m; k += 256)
        if (s_h[k]) atomicAdd(&hist[(int64_t)b * (m + 2) + 1 + k], s_h[k]);
}

__global__ void __launch_bounds__(256) wp_finish_kernel(const unsigned long long *__restrict__ area, unsigned long long *__restrict__ hist, int m)
{
    __shared__ unsigned long long s_sum;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    unsigned long long mine = 0;
    unsigned long long *row = hist + (int64_t)b * (m + 2);
    for (int k = threadIdx.x; k < m; k += 256) mine += row[1 + k];
    if (mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long A = area[b];
        row[0] = A;
        row[m + 1] = A * A - s_sum;
    }
}

__global__ void __launch_bounds__(256) wp_lags_kernel(const unsigned *__restrict__ gamma, long long *__restrict__ lags, int64_t total,
                                                       int R, int Ry, int Rx)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int nx = 2 * R + 1;
    const int64_t row = idx / nx;
    const int dx = (int)(idx - row * nx) - R, dy = (int)(row % (R + 1));
    const int64_t b = row / (R + 1);
    long long v = 0;
    if (dy <= Ry && dx >= -Rx && dx <= Rx) v = gamma[(b * (Ry + 1) + dy) * (2 * Rx + 1) + dx + Rx];
    lags[idx] = v;
}

struct WpWorkspace {
    uint32_t *bits;
    unsigned long long *area;
    unsigned *gamma;
    long long *thr;
    size_t gamma_words;
};

static WpWorkspace wp_carve(Carver &cv, int B, const WpGeom &g, int n_edges)
{
    WpWorkspace w;
    w.bits = cv.take<uint32_t>((size_t)B * g.H * g.WW);
    w.area = cv.take<unsigned long long>((size_t)B);
    w.gamma_words = (size_t)B * (g.Ry + 1) * g.ndx;
    w.gamma = cv.take<unsigned>(w.gamma_words);
    w.thr = cv.take<long long>((size_t)n_edges);
    return w;
}

static bool wp_shape_ok(int B, int H, int W, int n_edges)
{
    return check_shape(B, H, W) && B <= 65535 && n_edges >= 2 && n_edges <= MAX_HIST_BINS + 1;
}

// R = floor(sqrt(t - 1)) for the last threshold t >= 1
static int64_t wp_reach_of(int64_t t)
{
    const uint64_t v = (uint64_t)t - 1;  // below 2^63: r < 2^32 and (r + 1)^2 < 2^64, nothing wraps
    uint64_t r = (uint64_t)std::sqrt((double)v);
    while (r > 0 && r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return (int64_t)r;
}

static int wp_thresholds(const double *edges, int n_edges, double scale, int64_t *thr, int64_t *reach)
{
    const int rc = pcseg_surface_thresholds(edges, n_edges, scale, thr);  // (checks edges and scale)
    if (rc != PCSEG_OK) return rc;
    *reach = wp_reach_of(thr[n_edges - 1]);
    return PCSEG_OK;
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

int pcseg_window_rows(void) { return WP_ROWS; }

int pcseg_window_reach(const double *edges, int n_edges, double scale, int64_t *reach)
{
    PCSEG_REQUIRE(reach && n_edges >= 2 && n_edges <= MAX_HIST_BINS + 1, "bad arguments");
    int64_t thr[MAX_HIST_BINS + 1];
    return wp_thresholds(edges, n_edges, scale, thr, reach);
}

size_t pcseg_window_pairs_workspace_bytes(int B, int H, int W, int n_edges, int64_t reach)
{
    if (!wp_shape_ok(B, H, W, n_edges) || reach < 0 || reach > WP_MAX_REACH) return 0;
    return carved_bytes(wp_carve, B, wp_geom(H, W, reach), n_edges);
}

int pcseg_window_pairs(const uint8_t *mask, int B, int H, int W, double scale, const double *edges, int n_edges, int64_t *hist,
                       int64_t *lags, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(mask && hist && workspace && wp_shape_ok(B, H, W, n_edges), "bad arguments");
    int64_t thr[MAX_HIST_BINS + 1], reach = 0;
    const int rc = wp_thresholds(edges, n_edges, scale, thr, &reach);
    if (rc != PCSEG_OK) return rc;
    PCSEG_REQUIRE(reach <= WP_MAX_REACH, "the reach of the last edge is above PCSEG_WINDOW_MAX_REACH");
    const WpGeom g = wp_geom(H, W, reach);
    const int64_t total = (int64_t)B * (g.R + 1) * (2 * g.R + 1);  // of the lag table
    PCSEG_REQUIRE(!lags || (total + 255) / 256 < ((int64_t)1 << 31), "the lag table is too large");
    Carver cv(workspace, workspace_bytes);
    const WpWorkspace w = wp_carve(cv, B, g, n_edges);
    if (!cv.fits("window_pairs")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int m = n_edges - 1;
    const int64_t rows = (int64_t)B * H;
    const int64_t *thr_p = thr;
    const int up = upload_values(s, w.thr, n_edges, [=](int k) { return (long long)thr_p[k]; });
    if (up != PCSEG_OK) return up;
    PCSEG_CHECK_HIP(hipMemsetAsync(w.area, 0, sizeof(unsigned long long) * (size_t)B, s));
    PCSEG_CHECK_HIP(hipMemsetAsync(w.gamma, 0, sizeof(unsigned) * w.gamma_words, s));
    PCSEG_CHECK_HIP(hipMemsetAsync(hist, 0, sizeof(int64_t) * (size_t)B * (m + 2), s));
    const int64_t pack_blocks = (rows * ((W + 63) / 64) + 15) / 16;
    PCSEG_LAUNCH(wp_pack_kernel, dim3((unsigned)(pack_blocks > 16384 ? 16384 : pack_blocks)), dim3(256), 0, s, mask, w.bits, w.area, rows,
                 H, W, g.WW);
    PCSEG_CHECK_LAUNCH();
    const size_t lds = g.lds();
    if (lds > 64 * 1024)
        PCSEG_CHECK_HIP(hipFuncSetAttribute((const void *)wp_lag_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    PCSEG_LAUNCH(wp_lag_kernel, dim3((H + WP_ROWS - 1) / WP_ROWS, g.Ry + 1, B), dim3(WP_THREADS), lds, s, (const uint32_t *)w.bits, w.gamma, g);
    PCSEG_CHECK_LAUNCH();
    const int64_t n_lags = (int64_t)(g.Ry + 1) * g.ndx;
    const int64_t per_block = 256 * 16;
    PCSEG_LAUNCH(wp_bin_kernel, dim3((unsigned)((n_lags + per_block - 1) / per_block), B), dim3(256), sizeof(unsigned long long) * m, s,
                 (const unsigned *)w.gamma, (const long long *)w.thr, m, (unsigned long long *)hist, g.Ry, g.Rx, per_block);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(wp_finish_kernel, dim3(B), dim3(256), 0, s, (const unsigned long long *)w.area, (unsigned long long *)hist, m);
    PCSEG_CHECK_LAUNCH();
    if (lags) {
        PCSEG_LAUNCH(wp_lags_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const unsigned *)w.gamma, (long long *)lags, total,
                     g.R, g.Ry, g.Rx);
        PCSEG_CHECK_LAUNCH();
    }
    return PCSEG_OK;
}

}  // extern "C"
