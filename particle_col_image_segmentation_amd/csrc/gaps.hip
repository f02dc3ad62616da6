// Edge-to-edge gaps: the nearest-label transform that EXCLUDES the pixel's own label, and the table of the smallest gap of
// every ROI to the ROIs of each type slot (include/pcseg_gaps.h).  Integers only, so nothing depends on the order of the atomics.
//
// Why two candidates per column suffice: for a query of label l, a column can only offer its nearest site whose label is
// not l.  Keep per pixel the column's nearest site (g1, l1) and its nearest site with a label other than l1, (g2, l2), at
// equal distance the smaller label each time.  If l1 != l, (g1, l1) is the lexicographic minimum of (distance, label) over ALL
// sites of the column and carries another label than l, so it is the minimum over the sites that do; if l1 == l the sites
// with a label other than l are those with a label other than l1, whose minimum is (g2, l2).  d2 = k * k + g * g grows with g
// for a fixed column offset k, so the minimum of (d2, label) over the frame is the minimum over the columns' offers.
// Launches (asynchronous, no host read):
//   gap_col_kernel    one lane per column, down the rows and up again (eight rows' loads in flight).  Each scan carries the last
//                     site (row, label A) and the last site with a label other than A (row, B): on a site of label X != A,
//                     (row2, B) = (row1, A), (row1, A) = (row, X), else row1 = row.  The way down leaves its two candidates in
//                     the planes, the way up merges its own two into them: gg = g1 | g2 << 16, l1, l2.  Also the smallest and
//                     the largest site label of the frame (span), one wave reduction and two atomics per wave
//   gap_row_kernel    a row block's (gg, l1) staged in LDS, 8 bytes a cell; per pixel voronoi.hip's expanding search over the
//                     column offsets, left only when k * k > best (STRICT: an equally near site of a smaller label is still seen).
//                     g1 <= g2, so k * k + g1 * g1 > best rejects a column before l1 is looked at; l2 is read from global
//                     memory only for a candidate with d <= best.  A frame whose sites carry ONE label answers its pixels of that
//                     label at once (span): they would search the whole row for nothing
// and for the table, per slot t the column pass with sel_t as the selection, then
//   gap_sel_kernel        (once) sel_t = live & (slot_of == t) for the K slots
//   gap_table_row_kernel  the same stage and search, but only for the RIM pixels of live labels (a 4-neighbour that is not the
//                         label: the minimum over a label's pixels is always attained there), and no image is written: the
//                         min of d2 << 32 | near over a run of lanes of one label is folded by label_reduce.h's segmented
//                         wave reduction, the rest goes through its LDS slot table (64-bit atomicMin) into (B, cap, K)
//   gap_table_kernel      every (label, slot) of the table from the accumulators: -1 / 0 for none and for labels not live
#include <type_traits>

#include "label_reduce.h"

#include "../../include/pcseg_gaps.h"

// (no floating point in here; the pragma keeps any that is added later rounded operation by operation, as surface.hip)
#pragma clang fp contract(off)

namespace pcseg {

// a staged distance without site: its square is >= 2^31 > any d2 of a frame, adding k * k still fits 32 bits (VOR_G_NONE),
// and it fits the 16 bits of a packed distance
constexpr unsigned GAP_G_NONE = 46341u;
constexpr unsigned GAP_CELL_NONE = GAP_G_NONE | (GAP_G_NONE << 16);
constexpr unsigned GAP_BEST0 = 0x7FFFFFFFu;
constexpr int GAP_COL_ROWS = 8;      // rows whose loads a column lane issues together
constexpr int GAP_MAX_WIDTH = 16382;  // PCSEG_GAPS_MAX_WIDTH
constexpr unsigned long long GAP_NO_KEY = ~0ull;
static_assert((GAP_MAX_WIDTH + 2) * 8 <= 128 * 1024, "one row of the stage fits 128 KB of LDS");

struct GapSite {  // voronoi.hip's SiteTest
    const uint8_t *sel;  // the frame's row of the selection, or null
    int cap;
    __device__ __forceinline__ bool operator()(int l) const { return l >= 1 && l <= cap && (!sel || sel[l - 1] != 0); }
};

struct GapWs {
    unsigned *gg;  // (B, H, W) g1 | g2 << 16
    int *l1, *l2;  // (B, H, W)
    int *span;     // (B, 2): the largest site label, the largest INT_MAX - site label; 0, 0 = a frame without site
};

inline GapWs gap_carve(Carver &cv, int B, int H, int W)
{
    GapWs ws;
    const size_t n = (size_t)B * H * W;
    ws.gg = cv.take<unsigned>(n);
    ws.l1 = cv.take<int>(n);
    ws.l2 = cv.take<int>(n);
    ws.span = cv.take<int>(2 * (size_t)B);
    return ws;
}

// a column's scan state: the last site and the last site of another label than that one (rows; -1 = none)
struct GapScan {
    int r1 = -1, a = 0, r2 = -1, b = 0;
    __device__ __forceinline__ void site(int row, int x)
    {
        if (r1 >= 0 && x != a) {
            r2 = r1;
            b = a;
        }
        r1 = row;
        a = x;
    }
};

// the smaller of two candidates (distance, label), at equal distance the smaller label (two "none" have label 0 both)
__device__ __forceinline__ void gap_min2(unsigned da, int la, unsigned db, int lb, unsigned &d, int &l)
{
    const bool first = da < db || (da == db && la <= lb);
    d = first ? da : db;
    l = first ? la : lb;
}

__global__ void __launch_bounds__(64) gap_col_kernel(const int *__restrict__ labels, const uint8_t *__restrict__ sel, int cap,
                                                      unsigned *__restrict__ gg, int *__restrict__ l1, int *__restrict__ l2,
                                                      int *__restrict__ span, int H, int W)
{
    const int c0 = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    const bool in = c0 < W;  // (every lane walks for the wave reduction: a lane past the width re-reads the last column, writes nothing)
    const int c = min(c0, W - 1);
    const int64_t fbase = (int64_t)b * H * W + c;
    const int *lab = labels + fbase;
    const GapSite site{sel ? sel + (int64_t)b * cap : nullptr, cap};
    int hi = 0, lo = 0x7FFFFFFF;
    // ---- down: the two candidates at or above every row
    GapScan dn;
    for (int rb = 0; rb < H; rb += GAP_COL_ROWS) {
        int v[GAP_COL_ROWS];
#pragma unroll
        for (int j = 0; j < GAP_COL_ROWS; ++j) v[j] = lab[rowoff(min(rb + j, H - 1), W)];
#pragma unroll
        for (int j = 0; j < GAP_COL_ROWS; ++j) {
            const int r = rb + j;
            if (r >= H) break;
            if (site(v[j])) {
                dn.site(r, v[j]);
                hi = max(hi, v[j]);
                lo = min(lo, v[j]);
            }
            if (in) {
                const int64_t at = fbase + rowoff(r, W);
                gg[at] = (dn.r1 < 0 ? GAP_G_NONE : (unsigned)(r - dn.r1)) | ((dn.r2 < 0 ? GAP_G_NONE : (unsigned)(r - dn.r2)) << 16);
                l1[at] = dn.a;
                l2[at] = dn.b;
            }
        }
    }
    // ---- up: the two candidates at or below every row, merged with those of the way down
    GapScan up;
    for (int rb = (H - 1) / GAP_COL_ROWS * GAP_COL_ROWS; rb >= 0; rb -= GAP_COL_ROWS) {
        int v[GAP_COL_ROWS], pa[GAP_COL_ROWS], pb[GAP_COL_ROWS];
        unsigned pg[GAP_COL_ROWS];
#pragma unroll
        for (int j = 0; j < GAP_COL_ROWS; ++j) {
            const int64_t off = rowoff(min(rb + j, H - 1), W);
            v[j] = lab[off];
            pg[j] = in ? gg[fbase + off] : GAP_CELL_NONE;
            pa[j] = in ? l1[fbase + off] : 0;
            pb[j] = in ? l2[fbase + off] : 0;
        }
#pragma unroll
        for (int j = GAP_COL_ROWS - 1; j >= 0; --j) {
            const int r = rb + j;
            if (r >= H) continue;
            if (site(v[j])) up.site(r, v[j]);
            if (!in) continue;
            const unsigned d1 = pg[j] & 0xFFFFu, d2 = pg[j] >> 16;
            const unsigned u1 = up.r1 < 0 ? GAP_G_NONE : (unsigned)(up.r1 - r), u2 = up.r2 < 0 ? GAP_G_NONE : (unsigned)(up.r2 - r);
            unsigned g1, g2, gd, gu;
            int m1, m2, ld, lu;
            gap_min2(d1, pa[j], u1, up.a, g1, m1);
            // each side's nearest site of another label than m1: its first candidate unless that one carries m1
            gd = pa[j] != m1 ? d1 : d2;
            ld = pa[j] != m1 ? pa[j] : pb[j];
            gu = up.a != m1 ? u1 : u2;
            lu = up.a != m1 ? up.a : up.b;
            gap_min2(gd, ld, gu, lu, g2, m2);
            const int64_t at = fbase + rowoff(r, W);
            gg[at] = g1 | (g2 << 16);
            l1[at] = m1;
            l2[at] = g2 == GAP_G_NONE ? 0 : m2;
        }
    }
    // ---- the frame's smallest and largest site label
    for (int off = 1; off < WAVE; off <<= 1) {
        hi = max(hi, __shfl_xor(hi, off));
        lo = min(lo, __shfl_xor(lo, off));
    }
    if (threadIdx.x == 0 && hi > 0) {
        atomicMax(&span[2 * b], hi);
        atomicMax(&span[2 * b + 1], 0x7FFFFFFF - lo);
    }
}

// ---- the row search, shared by the transform and the table
constexpr int gap_waves_per_row(int RB) { return RB >= 4 ? 1 : 4 / RB; }

// a block of 256 threads stages (gg, l1) of the rows r0 .. r0 + nrows - 1 of a frame, cells[RB][W + 2] with one guard cell
// either side of a row, and waits for it
template <int RB>
__device__ __forceinline__ void gap_stage_rows(uint2 *cells, const unsigned *__restrict__ gg, const int *__restrict__ l1,
                                               int64_t fbase, int r0, int nrows, int W)
{
    const int P = W + 2;
    for (int j = 0; j < nrows; ++j)
        for (int c = threadIdx.x; c < W; c += 256) {
            const int64_t gi = fbase + rowoff(r0 + j, W) + c;
            cells[j * P + c + 1] = make_uint2(gg[gi], (unsigned)l1[gi]);
        }
    if (threadIdx.x < 2 * RB) cells[(threadIdx.x >> 1) * P + ((threadIdx.x & 1) ? W + 1 : 0)] = make_uint2(GAP_CELL_NONE, 0u);
    __syncthreads();
}

// the pixel of label l at column c of a staged row (gr[-1] and gr[W] are the guard cells; second: the row of l2): the
// lexicographic minimum of (d2, label) over the columns' offers within `best` (in: the reach; out: d2).  False: none
__device__ __forceinline__ bool gap_search(const uint2 *gr, const int *__restrict__ second, int c, int W, int l, unsigned &best,
                                           int &lbl)
{
    bool found = false;
    lbl = 0;
    // column cc at squared offset kk: its nearest site of another label than l, if that lies within best
    auto offer = [&](int cc, const uint2 cell, unsigned kk) {
        const unsigned g1 = cell.x & 0xFFFFu;
        unsigned d = __umul24(g1, g1) + kk;
        if (d > best) return;
        int cand = (int)cell.y;
        if (cand == l) {
            const unsigned g2 = cell.x >> 16;
            d = __umul24(g2, g2) + kk;
            if (d > best) return;
            cand = second[cc];
        }
        if (d < best || !found || cand < lbl) {  // (d <= best here)
            best = d;
            lbl = cand;
            found = true;
        }
    };
    offer(c, gr[c], 0u);
    // offsets k .. k + 3 on both sides per trip (eight LDS reads issued together); indices are clamped onto the guard
    // cells, which never qualify.  The exit test is STRICT, as in vor_row_kernel
    const int klim = max(c, W - 1 - c);
    for (int k = 1; k <= klim && (unsigned)(k * k) <= best; k += 4) {
        uint2 gl[4], gq[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            gl[t] = gr[max(c - k - t, -1)];
            gq[t] = gr[min(c + k + t, W)];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned kk = (unsigned)((k + t) * (k + t));
            offer(c - k - t, gl[t], kk);
            offer(c + k + t, gq[t], kk);
        }
    }
    return found;
}

template <int RB>
__global__ void __launch_bounds__(256) gap_row_kernel(const int *__restrict__ labels, const unsigned *__restrict__ gg,
                                                       const int *__restrict__ l1, const int *__restrict__ l2,
                                                       const int *__restrict__ span, unsigned best0, int *__restrict__ d2_out,
                                                       int *__restrict__ near_out, int H, int W)
{
    extern __shared__ __attribute__((aligned(16))) uint2 gap_cells[];
    const int P = W + 2;
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * RB;
    const int nrows = min(RB, H - r0);
    const int64_t fbase = (int64_t)b * H * W;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int WPR = gap_waves_per_row(RB), RSTEP = 4 / WPR;  // waves per row; rows the block's four waves cover at a time
    const int hi = span[2 * b], lo = 0x7FFFFFFF - span[2 * b + 1];
    if (hi == 0) {  // a frame without site
        for (int j = wave / WPR; j < nrows; j += RSTEP)
            for (int c = lane + 64 * (wave % WPR); c < W; c += 64 * WPR) {
                const int64_t gi = fbase + rowoff(r0 + j, W) + c;
                d2_out[gi] = -1;
                near_out[gi] = 0;
            }
        return;
    }
    const int only = lo == hi ? hi : 0;  // the one label all sites of the frame carry
    gap_stage_rows<RB>(gap_cells, gg, l1, fbase, r0, nrows, W);
    for (int j = wave / WPR; j < nrows; j += RSTEP)
        for (int c = lane + 64 * (wave % WPR); c < W; c += 64 * WPR) {
            const int r = r0 + j;
            const int64_t gi = fbase + rowoff(r, W) + c;
            const int l = labels[gi];
            unsigned best = best0;
            int lbl = 0;
            const bool found = !(only && l == only) && gap_search(gap_cells + j * P + 1, l2 + fbase + rowoff(r, W), c, W, l, best, lbl);
            d2_out[gi] = found ? (int)best : -1;
            near_out[gi] = found ? lbl : 0;
        }
}

// The table's row pass for one slot: the search only where it can decide the table, reduced on the spot.  A query is a pixel
// of a live label l with a 4-neighbour inside the frame that is not l: from any other pixel of l one axis step towards
// the partner's pixel stays in l and is strictly closer, so the minimum is never attained there.  The wave folds the lanes
// of a run of l (interior pixels carry no value but keep the run together), the block's LDS slot table the rest
template <int RB>
__global__ void __launch_bounds__(256) gap_table_row_kernel(const int *__restrict__ labels, const uint8_t *__restrict__ live, int cap,
                                                             const unsigned *__restrict__ gg, const int *__restrict__ l1,
                                                             const int *__restrict__ l2, const int *__restrict__ span,
                                                             unsigned best0, unsigned long long *__restrict__ acc, int K, int t,
                                                             int H, int W)
{
    extern __shared__ __attribute__((aligned(16))) uint2 gap_cells[];
    __shared__ int tags[LABEL_SLOTS];                 // (3072 bytes in front of the stage: a multiple of 16)
    __shared__ unsigned long long mins[LABEL_SLOTS];
    const int P = W + 2;
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * RB;
    const int nrows = min(RB, H - r0);
    const int64_t fbase = (int64_t)b * H * W;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int WPR = gap_waves_per_row(RB), RSTEP = 4 / WPR;
    const int hi = span[2 * b], lo = 0x7FFFFFFF - span[2 * b + 1];
    if (hi == 0) return;  // no site of this slot in the frame: the accumulators keep "none"
    const int only = lo == hi ? hi : 0;
    for (int i = threadIdx.x; i < LABEL_SLOTS; i += 256) {
        tags[i] = 0;
        mins[i] = GAP_NO_KEY;
    }
    gap_stage_rows<RB>(gap_cells, gg, l1, fbase, r0, nrows, W);
    unsigned long long *gacc = acc + (int64_t)b * cap * K + t;  // [(l - 1) * K]
    const uint8_t *alive = live + (int64_t)b * cap;
    const int *lab = labels + fbase;
    for (int j = wave / WPR; j < nrows; j += RSTEP)
        for (int cb = 64 * (wave % WPR); cb < W; cb += 64 * WPR) {  // (every lane stays for the wave's reduction)
            const int r = r0 + j, c = cb + lane;
            int lq = 0;
            unsigned long long m = GAP_NO_KEY;
            if (c < W) {
                const int64_t at = rowoff(r, W) + c;
                const int l = lab[at];
                if (l >= 1 && l <= cap && l != only && alive[l - 1] != 0) {
                    lq = l;
                    const bool rim = (c > 0 && lab[at - 1] != l) || (c + 1 < W && lab[at + 1] != l) || (r > 0 && lab[at - W] != l) ||
                                     (r + 1 < H && lab[at + W] != l);
                    unsigned best = best0;
                    int lbl = 0;
                    if (rim && gap_search(gap_cells + j * P + 1, l2 + fbase + rowoff(r, W), c, W, l, best, lbl))
                        m = ((unsigned long long)best << 32) | (unsigned)lbl;
                }
            }
            const WaveSeg seg = wave_segment(lq);
            segment_reduce(
                m, seg.remain, [](const unsigned long long &x, int off) { return __shfl_down(x, off); },
                [](unsigned long long &x, const unsigned long long &o) { x = min(x, o); });
            if (seg.head && lq > 0 && m != GAP_NO_KEY) {
                const int slot = slot_claim(tags, lq);
                if (slot >= 0) atomicMin(&mins[slot], m);
                else atomicMin(&gacc[(int64_t)(lq - 1) * K], m);
            }
        }
    __syncthreads();
    for (int i = threadIdx.x; i < LABEL_SLOTS; i += 256) {
        const int l = tags[i];
        if (l && mins[i] != GAP_NO_KEY) atomicMin(&gacc[(int64_t)(l - 1) * K], mins[i]);
    }
}

// sel (K, B, cap): the live labels of every slot
__global__ void __launch_bounds__(256) gap_sel_kernel(const uint8_t *__restrict__ live, const uint8_t *__restrict__ slot_of,
                                                       uint8_t *__restrict__ sel, int64_t n, int K)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool on = live[i] != 0;
    const int s = slot_of[i];
    for (int t = 0; t < K; ++t) sel[t * n + i] = (uint8_t)(on && s == t);
}

__global__ void __launch_bounds__(256) gap_table_kernel(const unsigned long long *__restrict__ acc, const uint8_t *__restrict__ live,
                                                         int *__restrict__ gap2, int *__restrict__ partner, int64_t n, int K)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long v = acc[i];
    const bool some = live[i / K] != 0 && v != GAP_NO_KEY;
    gap2[i] = some ? (int)(v >> 32) : -1;
    partner[i] = some ? (int)(unsigned)v : 0;
}

struct GapTableWs {
    GapWs col;
    uint8_t *sel;             // (K, B, cap)
    unsigned long long *acc;  // (B, cap, K)
};

inline GapTableWs gap_table_carve(Carver &cv, int B, int H, int W, int cap, int K)
{
    GapTableWs ws;
    ws.col = gap_carve(cv, B, H, W);
    ws.sel = cv.take<uint8_t>((size_t)K * B * cap);
    ws.acc = cv.take<unsigned long long>((size_t)B * cap * K);
    return ws;
}

static inline bool gap_shape(int B, int H, int W) { return check_shape(B, H, W) && W <= GAP_MAX_WIDTH && B <= 65535; }
static inline unsigned gap_reach(int64_t r2) { return (r2 < 0 || r2 > (int64_t)GAP_BEST0) ? GAP_BEST0 : (unsigned)r2; }

// the column pass of one selection into a carved workspace
static int gap_columns(const int *labels, const uint8_t *sel, int cap, int B, int H, int W, const GapWs &ws, hipStream_t s)
{
    PCSEG_CHECK_HIP(hipMemsetAsync(ws.span, 0, sizeof(int) * 2 * B, s));
    PCSEG_LAUNCH(gap_col_kernel, dim3((W + 63) / 64, B), dim3(64), 0, s, labels, sel, cap, ws.gg, ws.l1, ws.l2, ws.span, H, W);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

// rows per block of a row pass: four while a block's stage stays within 64 KB (W <= 2046), else one (W <= 8190 within 64 KB,
// 128 KB at the widest frame: one block per CU, the occupancy argument of vor_row_kernel).  launch(RB tag, stage bytes)
template <typename Launch>
static int gap_rows_by_width(int W, Launch launch)
{
    const size_t per_row = (size_t)(W + 2) * sizeof(uint2);
    const int rc = 4 * per_row <= 64 * 1024 ? launch(std::integral_constant<int, 4>(), 4 * per_row)
                                            : launch(std::integral_constant<int, 1>(), per_row);
    if (rc) return rc;
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_nearest_other_label_workspace_bytes(int B, int H, int W)
{
    if (!gap_shape(B, H, W)) return 0;
    return carved_bytes(gap_carve, B, H, W);
}

int pcseg_nearest_other_label_i32(const int32_t *labels, const uint8_t *sel, int cap, int64_t r2, int32_t *d2, int32_t *near, int B,
                                  int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels && d2 && near && workspace && check_shape(B, H, W) && cap >= 1 && B <= 65535, "bad arguments");
    PCSEG_REQUIRE(W <= GAP_MAX_WIDTH, "a frame wider than PCSEG_GAPS_MAX_WIDTH");
    Carver cv(workspace, workspace_bytes);
    const GapWs ws = gap_carve(cv, B, H, W);
    if (!cv.fits("nearest_other_label_i32")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = gap_columns(labels, sel, cap, B, H, W, ws, s)) return rc;
    return gap_rows_by_width(W, [&](auto rb_tag, size_t bytes) -> int {
        constexpr int RB = decltype(rb_tag)::value;
        if (bytes > 64 * 1024)
            PCSEG_CHECK_HIP(hipFuncSetAttribute((const void *)gap_row_kernel<RB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        PCSEG_LAUNCH((gap_row_kernel<RB>), dim3((H + RB - 1) / RB, B), dim3(256), bytes, s, labels, (const unsigned *)ws.gg,
                     (const int *)ws.l1, (const int *)ws.l2, (const int *)ws.span, gap_reach(r2), d2, near, H, W);
        return PCSEG_OK;
    });
}

size_t pcseg_label_gaps_workspace_bytes(int B, int H, int W, int cap, int K)
{
    if (!gap_shape(B, H, W) || cap < 1 || cap >= (1 << 30) || K < 1 || K > 4) return 0;
    return carved_bytes(gap_table_carve, B, H, W, cap, K);
}

int pcseg_label_gaps(const int32_t *labels, const uint8_t *live, const uint8_t *slot_of, int cap, int K, int64_t r2, int32_t *gap2,
                     int32_t *partner, int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels && live && slot_of && gap2 && partner && workspace && check_shape(B, H, W) && cap >= 1 && cap < (1 << 30) &&
                      B <= 65535,
                  "bad arguments");
    PCSEG_REQUIRE(K >= 1 && K <= 4, "1..4 type slots");
    PCSEG_REQUIRE(W <= GAP_MAX_WIDTH, "a frame wider than PCSEG_GAPS_MAX_WIDTH");
    Carver cv(workspace, workspace_bytes);
    const GapTableWs ws = gap_table_carve(cv, B, H, W, cap, K);
    if (!cv.fits("label_gaps")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)B * cap, n = rows * K;
    PCSEG_CHECK_HIP(hipMemsetAsync(ws.acc, 0xFF, sizeof(unsigned long long) * (size_t)n, s));
    PCSEG_LAUNCH(gap_sel_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, live, slot_of, ws.sel, rows, K);
    PCSEG_CHECK_LAUNCH();
    for (int t = 0; t < K; ++t) {
        if (const int rc = gap_columns(labels, ws.sel + (size_t)t * rows, cap, B, H, W, ws.col, s)) return rc;
        const int rc = gap_rows_by_width(W, [&](auto rb_tag, size_t bytes) -> int {
            constexpr int RB = decltype(rb_tag)::value;
            if (bytes > 64 * 1024)
                PCSEG_CHECK_HIP(hipFuncSetAttribute((const void *)gap_table_row_kernel<RB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    (int)bytes));
            PCSEG_LAUNCH((gap_table_row_kernel<RB>), dim3((H + RB - 1) / RB, B), dim3(256), bytes, s, labels, live, cap,
                         (const unsigned *)ws.col.gg, (const int *)ws.col.l1, (const int *)ws.col.l2, (const int *)ws.col.span,
                         gap_reach(r2), ws.acc, K, t, H, W);
            return PCSEG_OK;
        });
        if (rc) return rc;
    }
    PCSEG_LAUNCH(gap_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const unsigned long long *)ws.acc, live, gap2,
                 partner, n, K);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
