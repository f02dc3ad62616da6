// Goal 2 of refine_boundaries.py:1-12: the refined ROIs (watershed labels) related to the class-map components they
// split, and the tables that resolve clusters into refined cells.
//
// pcseg_label_parent: for every refined ROI r of a frame, the class-map component a that shares the most pixels with it
// (ties: the smallest a), that overlap, and the number of distinct components it touches.  Three passes, all on the
// device, all exact (integer counts: any atomic order gives the same result):
//   1. lp_count_kernel   the column-run walk of label_reduce.h over BOTH label images: a lane owns 4 columns of a 32-row
//                        block, a run is a vertical stretch of constant (r, a), runs of adjacent lanes with the same
//                        pair are summed by a segmented shuffle, and a finished run goes into r's
//                        candidate table: LP_SLOTS (label, count) slots, a slot claimed by atomicCAS on its label word.
//                        An r that finds every slot taken by other labels is marked spilled and listed (once).
//   2. lp_spill_kernel   one block per spilled r: scans r's bounding box, counting a in a direct-indexed LDS array over
//                        windows of LP_WIN labels; each pass also finds the smallest a above its window, so only
//                        windows that hold a label are visited.  No hash, no capacity limit.
//   3. lp_final_kernel   argmax over the candidate slots of the other rows, class of the parent, the cap flag.
//
// pcseg_refined_layout / pcseg_refined_table_write: the `refined`, `cell_resolution` and `frames_refined` rows (one
// block per frame, row positions by block scans as in tables.hip) and the refined points for pcseg_point_neighbours.
#include "label_reduce.h"
#include "table_common.h"

namespace pcseg {

constexpr int LP_SLOTS = 16;  // candidate (label, count) slots per refined ROI: one 128-byte line
constexpr int LP_WIN = 4096;  // label window of the spill pass (16 KiB of LDS)

__global__ void __launch_bounds__(256) lp_clear_kernel(const int *__restrict__ counts_r, int B, int cap, int *__restrict__ cand,
                                                       int *__restrict__ spilled, int *__restrict__ n_spill, int *__restrict__ overflow)
{
    const int64_t total = (int64_t)B * cap;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / cap), r = (int)(i - (int64_t)b * cap);
        if (r == 0) overflow[b] = 0;
        if (r >= min(counts_r[b], cap)) continue;
        int4 *c = reinterpret_cast<int4 *>(cand + i * 2 * LP_SLOTS);
#pragma unroll
        for (int k = 0; k < LP_SLOTS / 2; ++k) c[k] = make_int4(0, 0, 0, 0);
        spilled[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_spill = 0;
}

// one finished run of `n` pixels of the pair (r, a) into r's candidate slots.  (Reading a snapshot of the 16 label
// words first and trying only its free slots made the count pass slower on the benchmark batch: 0.98 ms against 0.76.)
__device__ __forceinline__ void lp_commit(int *cand, int *spilled, int *spill_list, int *n_spill, int64_t row, int a, int n)
{
    int *c = cand + row * 2 * LP_SLOTS;
#pragma unroll
    for (int s = 0; s < LP_SLOTS; ++s) {
        const int old = atomicCAS(&c[2 * s], 0, a);
        if (old == 0 || old == a) {
            atomicAdd(&c[2 * s + 1], n);
            return;
        }
    }
    if (atomicExch(&spilled[row], 1) == 0) spill_list[atomicAdd(n_spill, 1)] = (int)row;
}

struct LpRun {
    long long key;  // r << 32 | a; 0 = nothing
    int n;
};

struct LpRaw {
    int4 r, a;
};
__device__ __forceinline__ void landed(const LpRaw &q) { landed(q.r); landed(q.a); }

// the walk's key is the pair (refined label, class-map label) of a pixel.
// VEC: W % 4 == 0 and both images 16-byte aligned (int4 loads); otherwise four guarded loads per row and image
template <bool VEC>
struct LpWalk {
    using Key = long long;
    using Raw = LpRaw;
    using Run = LpRun;
    const int *pa, *pr;  // the frame's two images
    int c, W, nr;
    int *cand, *spilled, *spill_list, *n_spill;
    int64_t rowbase;
    __device__ __forceinline__ Raw load(int y) const
    {
        return Raw{row_labels4<VEC>(pr + rowoff(y, W), c, W), row_labels4<VEC>(pa + rowoff(y, W), c, W)};
    }
    __device__ __forceinline__ void keys(const Raw &q, Key k[4]) const
    {
        const int rv[4] = {q.r.x, q.r.y, q.r.z, q.r.w}, av[4] = {q.a.x, q.a.y, q.a.z, q.a.w};
        // pixels on A = 0, on R = 0 or on an R label without a row (above min(counts_r, cap)) belong to no pair
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = (rv[j] >= 1 && rv[j] <= nr && av[j] >= 1) ? ((long long)rv[j] << 32) | (unsigned)av[j] : 0;
    }
    __device__ __forceinline__ Run run(Key key, int start, int end, int) const { return Run{key, end - start}; }
    static __device__ __forceinline__ Run shfl(const Run &q, int off) { return Run{q.key, __shfl_down(q.n, off)}; }
    static __device__ __forceinline__ void merge(Run &q, const Run &o) { q.n += o.n; }
    __device__ __forceinline__ void commit(const Run &q) const
    {
        lp_commit(cand, spilled, spill_list, n_spill, rowbase + (int)(q.key >> 32) - 1, (int)q.key, q.n);
    }
};

template <bool VEC>
__global__ void __launch_bounds__(256) lp_count_kernel(const int *__restrict__ la, const int *__restrict__ lr,
                                                       const int *__restrict__ counts_r, int H, int W, int cap, int *__restrict__ cand,
                                                       int *__restrict__ spilled, int *__restrict__ spill_list, int *__restrict__ n_spill)
{
    const TileIndex ti = xcd_tile_index();
    const int b = ti.z;
    const int64_t npx = (int64_t)H * W;
    const int c = (ti.x * 256 + threadIdx.x) * 4;
    const int r0 = ti.y * RUN_ROWS;
    column_run_walk(LpWalk<VEC>{la + b * npx, lr + b * npx, c, W, min(counts_r[b], cap), cand, spilled, spill_list, n_spill,
                                (int64_t)b * cap},
                    c, r0, min(H, r0 + RUN_ROWS));
}

// block-wide (sum, max, min) over 256 threads
__device__ __forceinline__ void lp_block_reduce(int &sum, unsigned long long &mx, int &mn, int *s_sum, unsigned long long *s_mx, int *s_mn)
{
    for (int off = 32; off >= 1; off >>= 1) {
        sum += __shfl_xor(sum, off);
        const unsigned long long m = __shfl_xor(mx, off);
        mx = m > mx ? m : mx;
        mn = min(mn, __shfl_xor(mn, off));
    }
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) { s_sum[w] = sum; s_mx[w] = mx; s_mn[w] = mn; }
    __syncthreads();
    sum = s_sum[0]; mx = s_mx[0]; mn = s_mn[0];
    for (int k = 1; k < 4; ++k) {
        sum += s_sum[k];
        mx = s_mx[k] > mx ? s_mx[k] : mx;
        mn = min(mn, s_mn[k]);
    }
    __syncthreads();
}

// spilled rows, exactly: one block per listed r (a persistent grid walks the list the count pass built)
__global__ void __launch_bounds__(256) lp_spill_kernel(const int *__restrict__ la, const int *__restrict__ lr,
                                                       const long long *__restrict__ stats_r, const int *__restrict__ spill_list,
                                                       const int *__restrict__ n_spill, int H, int W, int cap, int *__restrict__ parent,
                                                       int *__restrict__ parent_px, int *__restrict__ n_overlap)
{
    __shared__ int hist[LP_WIN];
    __shared__ int s_sum[4], s_mn[4];
    __shared__ unsigned long long s_mx[4];
    const int items = *n_spill;
    const int64_t npx = (int64_t)H * W;
    const int wv = threadIdx.x >> 6, lane = lane_id();
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int row = spill_list[it];
        const int b = row / cap, rl = row - b * cap + 1;
        const int *pa = la + b * npx, *pr = lr + b * npx;
        int y0 = 0, x0 = 0, y1 = H, x1 = W;
        if (stats_r) {  // bounding box [min_row, max_row1) x [min_col, max_col1), clamped to the frame
            const long long *st = stats_r + (int64_t)row * 8;
            y0 = (int)max(0ll, min((long long)H, st[3])); x0 = (int)max(0ll, min((long long)W, st[4]));
            y1 = (int)max((long long)y0, min((long long)H, st[5])); x1 = (int)max((long long)x0, min((long long)W, st[6]));
        }
        // the smallest a under r
        int lo = 0x7FFFFFFF;
        for (int y = y0 + wv; y < y1; y += 4)
            for (int x = x0 + lane; x < x1; x += 64) {
                const int64_t o = rowoff(y, W) + x;
                const int a = pa[o];
                if (pr[o] == rl && a >= 1) lo = min(lo, a);
            }
        int dummy_sum = 0;
        unsigned long long dummy_mx = 0;
        lp_block_reduce(dummy_sum, dummy_mx, lo, s_sum, s_mx, s_mn);
        unsigned long long best = 0;  // count << 32 | (0x7FFFFFFF - a): the maximum is the largest count, then the smallest a
        int nov = 0;
        while (lo != 0x7FFFFFFF) {
            const int hi = lo > 0x7FFFFFFF - LP_WIN ? 0x7FFFFFFF : lo + LP_WIN;  // window [lo, hi)
            for (int k = threadIdx.x; k < LP_WIN; k += 256) hist[k] = 0;
            __syncthreads();
            int next = 0x7FFFFFFF;
            for (int y = y0 + wv; y < y1; y += 4)
                for (int x = x0 + lane; x < x1; x += 64) {
                    const int64_t o = rowoff(y, W) + x;
                    const int a = pa[o];
                    if (pr[o] != rl || a < lo) continue;
                    if (a < hi) atomicAdd(&hist[a - lo], 1);
                    else next = min(next, a);
                }
            if (hi == 0x7FFFFFFF) {  // (the last window holds 0x7FFFFFFF - lo < LP_WIN labels; a == 0x7FFFFFFF itself:)
                for (int y = y0 + wv; y < y1; y += 4)
                    for (int x = x0 + lane; x < x1; x += 64) {
                        const int64_t o = rowoff(y, W) + x;
                        if (pr[o] == rl && pa[o] == 0x7FFFFFFF) atomicAdd(&hist[0x7FFFFFFF - lo], 1);
                    }
            }
            __syncthreads();
            int cnt = 0;
            unsigned long long mx = 0;
            for (int k = threadIdx.x; k < LP_WIN; k += 256) {
                const int h = hist[k];
                if (h == 0) continue;
                ++cnt;
                const unsigned long long key = ((unsigned long long)(unsigned)h << 32) | (unsigned)(0x7FFFFFFF - (lo + k));
                mx = key > mx ? key : mx;
            }
            lp_block_reduce(cnt, mx, next, s_sum, s_mx, s_mn);
            nov += cnt;
            best = mx > best ? mx : best;
            lo = next;
        }
        if (threadIdx.x == 0) {
            parent[row] = best ? 0x7FFFFFFF - (int)(best & 0xFFFFFFFFu) : 0;
            parent_px[row] = (int)(best >> 32);
            n_overlap[row] = nov;
        }
    }
}

__global__ void __launch_bounds__(256) lp_final_kernel(const int *__restrict__ counts_r, const uint8_t *__restrict__ cls_a, int B, int cap,
                                                       const int *__restrict__ cand, const int *__restrict__ spilled,
                                                       const int *__restrict__ n_spill, int *__restrict__ parent,
                                                       int *__restrict__ parent_px, int *__restrict__ n_overlap,
                                                       uint8_t *__restrict__ cls_r, int *__restrict__ overflow, int *__restrict__ n_spilled)
{
    const int64_t total = (int64_t)B * cap;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / cap), r = (int)(i - (int64_t)b * cap);
        int p = 0, px = 0, nov = 0;
        if (r < min(counts_r[b], cap)) {
            if (spilled[i]) {
                p = parent[i]; px = parent_px[i]; nov = n_overlap[i];
            } else {
                const int4 *c = reinterpret_cast<const int4 *>(cand + i * 2 * LP_SLOTS);
#pragma unroll
                for (int k = 0; k < LP_SLOTS / 2; ++k) {
                    const int4 q = c[k];
                    const int la[2] = {q.x, q.z}, ln[2] = {q.y, q.w};
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        if (la[s] == 0) continue;
                        ++nov;
                        if (ln[s] > px || (ln[s] == px && la[s] < p)) { p = la[s]; px = ln[s]; }
                    }
                }
            }
        }
        parent[i] = p; parent_px[i] = px; n_overlap[i] = nov;
        if (p > cap) overflow[b] = 1;  // the parent has no row: its class is unknown
        if (cls_r) cls_r[i] = (cls_a && p >= 1 && p <= cap) ? cls_a[(int64_t)b * cap + p - 1] : (uint8_t)0;
    }
    if (n_spilled && blockIdx.x == 0 && threadIdx.x == 0) *n_spilled = *n_spill;
}

// ---- tables

constexpr int RF_T = MAX_TYPE_SLOTS;

// a refined row exists for r < min(n_markers, cap) with a pixel (the `rois` rows); a refined point is such a row of kind >= 1
__device__ __forceinline__ bool rf_row(const pcseg_refined_inputs &in, int b, int r)
{
    return in.ws_stats[((int64_t)b * in.cap + r) * 8] > 0;
}

__global__ void __launch_bounds__(256) rf_count_kernel(pcseg_refined_inputs in, long long *__restrict__ n_points)
{
    __shared__ int wsum[4];
    const int b = blockIdx.x;
    const int m = min(in.n_markers[b], in.cap);
    int n = 0;
    for (int r = threadIdx.x; r < m; r += 256) n += rf_row(in, b, r) && in.kind_r[(int64_t)b * in.cap + r] >= 1;
    int tot;
    block_exclusive_scan<256>(n, &tot, wsum);
    if (threadIdx.x == 0) n_points[b] = tot;
}

// offsets[0..B] of the points; totals = {points, frames whose parent label exceeded cap}
__global__ void __launch_bounds__(64) rf_scan_kernel(const long long *__restrict__ n_points, const int *__restrict__ parent_overflow,
                                                     int B, long long *__restrict__ offsets, long long *__restrict__ totals)
{
    if (threadIdx.x == 0) {
        long long acc = 0;
        for (int b = 0; b < B; ++b) {
            offsets[b] = acc;
            acc += n_points[b];
        }
        offsets[B] = acc;
        totals[0] = acc;
    } else if (threadIdx.x == 1) {
        long long acc = 0;
        for (int b = 0; parent_overflow && b < B; ++b) acc += parent_overflow[b] != 0;
        totals[1] = acc;
    }
}

__global__ void __launch_bounds__(256) rf_write_kernel(pcseg_refined_inputs in, TableOffsets tb,
                                                       const long long *__restrict__ pt_offsets, int *__restrict__ acc,
                                                       double *__restrict__ refined, double *__restrict__ resolution,
                                                       double *__restrict__ frames, double *__restrict__ xy, int *__restrict__ pslot,
                                                       int *__restrict__ pid, long long *__restrict__ frame_offsets)
{
    __shared__ int wsum[4];
    __shared__ int s_resolved[RF_T], s_residual[RF_T], s_neg[RF_T];
    __shared__ long long s_count[RF_T];
    const int b = blockIdx.x, cap = in.cap;
    const int64_t fb = (int64_t)b * cap;
    const double fid = (double)in.frame_ids[b];
    const int m = min(in.n_markers[b], cap), n = min(in.counts[b], cap);
    // per class-map row: children, sum of their cells, a child with cells == -1
    int *child = acc + fb * 3;
    for (int a = threadIdx.x; a < n; a += 256) { child[a * 3] = 0; child[a * 3 + 1] = 0; child[a * 3 + 2] = 0; }
    if (threadIdx.x < RF_T) { s_resolved[threadIdx.x] = 0; s_residual[threadIdx.x] = 0; s_neg[threadIdx.x] = 0; s_count[threadIdx.x] = 0; }
    __threadfence();
    __syncthreads();
    // ---- refined rows (and points)
    {
        double *out = refined + tb.first(b, ROWS_ROIS) * 11;
        const long long pbase = pt_offsets[b];
        int carry = 0, pcarry = 0;
        for (int base = 0; base < m; base += 256) {
            const int r = base + threadIdx.x;
            const int valid = r < m && rf_row(in, b, r);
            const int k = valid ? in.kind_r[fb + r] : 0;
            const int point = valid && k >= 1;
            int total, ptotal;
            const int pos = carry + block_exclusive_scan<256>(valid, &total, wsum);
            const int ppos = pcarry + block_exclusive_scan<256>(point, &ptotal, wsum);
            if (valid) {
                const int64_t *st = in.ws_stats + (fb + r) * 8;
                const double area = (double)st[0];
                const double crow = __ddiv_rn((double)st[1], area), ccol = __ddiv_rn((double)st[2], area);
                const int p = in.parent[fb + r], cells = in.cells_r[fb + r];
                double *row = out + (int64_t)pos * 11;
                row[0] = fid; row[1] = (double)(r + 1); row[2] = (double)p; row[3] = (double)in.parent_px[fb + r];
                row[4] = (double)in.n_overlap[fb + r]; row[5] = (double)in.cls_r[fb + r]; row[6] = (double)k;
                row[7] = (double)cells; row[8] = area; row[9] = crow; row[10] = ccol;
                if (k >= 1 && p >= 1 && p <= n) {
                    atomicAdd(&child[(p - 1) * 3], 1);
                    if (cells < 0) atomicOr(&child[(p - 1) * 3 + 2], 1);
                    else atomicAdd(&child[(p - 1) * 3 + 1], cells);
                }
                if (point && xy) {
                    const long long q = pbase + ppos;
                    xy[q * 2] = ccol + 1.0; xy[q * 2 + 1] = crow + 1.0;
                    pslot[q] = in.slot_r[fb + r] < RF_T ? (int)in.slot_r[fb + r] : -1;
                    pid[q] = r + 1;
                }
            }
            carry += total;
            pcarry += ptotal;
        }
        if (frame_offsets && threadIdx.x == 0) {
            frame_offsets[b] = pbase;
            if (b == gridDim.x - 1) frame_offsets[b + 1] = pt_offsets[b + 1];
        }
    }
    __threadfence();
    __syncthreads();
    // ---- cell_resolution rows: one per `cells` row (class-map kind >= 1), in its order
    {
        double *out = resolution + tb.first(b, ROWS_CELLS) * 5;
        int carry = 0;
        for (int base = 0; base < n; base += 256) {
            const int a = base + threadIdx.x;
            const int kind = a < n ? in.kind[fb + a] : 0;
            const int valid = kind > 0;
            int total;
            const int pos = carry + block_exclusive_scan<256>(valid, &total, wsum);
            if (valid) {
                const int ch = ld_agent(&child[a * 3]), sum = ld_agent(&child[a * 3 + 1]), neg = ld_agent(&child[a * 3 + 2]);
                const int resolved = kind == 2 && ch >= 2;
                const int integ = kind == 1 ? 1 : (resolved ? (neg ? -1 : sum) : in.cells[fb + a]);
                double *row = out + (int64_t)pos * 5;
                row[0] = fid; row[1] = (double)(a + 1); row[2] = (double)ch; row[3] = (double)resolved; row[4] = (double)integ;
                const int s = in.slot_of[fb + a];
                if (s < RF_T) {
                    if (kind == 2) atomicAdd(resolved ? &s_resolved[s] : &s_residual[s], 1);
                    if (integ < 0) atomicOr(&s_neg[s], 1);
                    else atomicAdd((unsigned long long *)&s_count[s], (unsigned long long)(long long)integ);
                }
            }
            carry += total;
        }
    }
    __syncthreads();
    // ---- frames_refined: [frame, refined nan flag, per slot: refined cells, refined clusters, resolved, residual, count]
    if (threadIdx.x == 0) {
        double *f = frames + (int64_t)b * (2 + 5 * in.n_slots);
        f[0] = fid;
        f[1] = (double)in.nan_flag_r[b];
        for (int s = 0; s < in.n_slots; ++s) {
            const int64_t *ts = in.type_stats_r + ((int64_t)b * RF_T + s) * 4;  // n_cells, n_clusters, sum of cell areas, first
            double *g = f + 2 + 5 * s;
            g[0] = (double)ts[0]; g[1] = (double)ts[1]; g[2] = (double)s_resolved[s]; g[3] = (double)s_residual[s];
            g[4] = s_neg[s] ? -1.0 : (double)s_count[s];
        }
    }
}

struct LabelParentWs {
    int *cand;                   // [B * cap][LP_SLOTS] (parent, pixels) pairs
    int *spilled, *spill_list;   // [B * cap]
    int *n_spill;                // [1]
};
static LabelParentWs label_parent_carve(Carver &cv, size_t rows)
{
    LabelParentWs ws;
    ws.cand = cv.take<int>(2 * LP_SLOTS * rows);
    ws.spilled = cv.take<int>(rows);
    ws.spill_list = cv.take<int>(rows);
    ws.n_spill = cv.take<int>(1);
    return ws;
}

// pcseg_refined_layout writes the head, pcseg_refined_table_write reads it and uses the accumulators
struct RefinedWs {
    long long *n_points;  // [B]
    long long *offsets;   // [B + 1]
    int *acc;             // [B][cap][3]
};
static RefinedWs refined_carve(Carver &cv, int B, int cap)
{
    RefinedWs ws;
    ws.n_points = cv.take<long long>(B);
    ws.offsets = cv.take<long long>((size_t)B + 1);
    ws.acc = cv.take<int>(3 * (size_t)B * cap);
    return ws;
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_label_parent_workspace_bytes(int B, int H, int W, int cap)
{
    if (!check_shape(B, H, W) || cap < 1) return 0;
    return carved_bytes(label_parent_carve, (size_t)B * cap);
}

int pcseg_label_parent(const int32_t *labels_a, const int32_t *labels_r, const int32_t *counts_r, const int64_t *stats_r,
                       const uint8_t *cls_a, int32_t *parent, int32_t *parent_px, int32_t *n_overlap, uint8_t *cls_r,
                       int32_t *overflow, int32_t *n_spilled, int B, int H, int W, int cap, void *workspace,
                       size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels_a && labels_r && counts_r && parent && parent_px && n_overlap && overflow && workspace &&
                      check_shape(B, H, W) && cap >= 1,
                  "bad arguments");
    const size_t rows = (size_t)B * cap;
    Carver cv(workspace, workspace_bytes);
    const LabelParentWs ws = label_parent_carve(cv, rows);
    int *cand = ws.cand, *spilled = ws.spilled, *spill_list = ws.spill_list, *n_spill = ws.n_spill;
    if (!cv.fits("label_parent")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int grid = (int)((rows + 255) / 256 < 4096 ? (rows + 255) / 256 : 4096);
    PCSEG_LAUNCH(lp_clear_kernel, dim3(grid), dim3(256), 0, s, counts_r, B, cap, cand, spilled, n_spill, overflow);
    PCSEG_CHECK_LAUNCH();
    const dim3 cgrid((unsigned)((W + 1023) / 1024), (unsigned)((H + RUN_ROWS - 1) / RUN_ROWS), (unsigned)B);
    const bool vec = W % 4 == 0 && ((uintptr_t)labels_a % 16) == 0 && ((uintptr_t)labels_r % 16) == 0;
    if (vec)
        PCSEG_LAUNCH(lp_count_kernel<true>, cgrid, dim3(256), 0, s, labels_a, labels_r, counts_r, H, W, cap, cand, spilled, spill_list,
                     n_spill);
    else
        PCSEG_LAUNCH(lp_count_kernel<false>, cgrid, dim3(256), 0, s, labels_a, labels_r, counts_r, H, W, cap, cand, spilled, spill_list,
                     n_spill);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(lp_spill_kernel, dim3(512), dim3(256), 0, s, labels_a, labels_r, (const long long *)stats_r, (const int *)spill_list,
                 (const int *)n_spill, H, W, cap, parent, parent_px, n_overlap);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(lp_final_kernel, dim3(grid), dim3(256), 0, s, counts_r, cls_a, B, cap, (const int *)cand, (const int *)spilled,
                 (const int *)n_spill, parent, parent_px, n_overlap, cls_r, overflow, n_spilled);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

size_t pcseg_refined_workspace_bytes(int B, int cap)
{
    if (B < 1 || cap < 1) return 0;
    return carved_bytes(refined_carve, B, cap);
}

static int refined_check(const pcseg_refined_inputs *in)
{
    return in && in->B >= 1 && in->cap >= 1 && in->n_slots >= 0 && in->n_slots <= RF_T && in->frame_ids && in->counts && in->kind &&
           in->slot_of && in->cells && in->n_markers && in->ws_stats && in->parent && in->parent_px && in->n_overlap && in->cls_r &&
           in->kind_r && in->slot_r && in->cells_r && in->type_stats_r && in->nan_flag_r;
}

int pcseg_refined_layout(const pcseg_refined_inputs *in, int64_t *totals, void *workspace, size_t workspace_bytes,
                         pcseg_stream_t stream)
{
    PCSEG_REQUIRE(refined_check(in) && totals && workspace, "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const RefinedWs ws = refined_carve(cv, in->B, in->cap);
    long long *n_points = ws.n_points, *offsets = ws.offsets;
    if (!cv.fits("refined_layout")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    PCSEG_LAUNCH(rf_count_kernel, dim3(in->B), dim3(256), 0, s, *in, n_points);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(rf_scan_kernel, dim3(1), dim3(64), 0, s, (const long long *)n_points, in->parent_overflow, in->B, offsets,
                 (long long *)totals);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_refined_table_write(const pcseg_refined_inputs *in, const void *table_workspace, size_t table_workspace_bytes,
                              double *refined, double *resolution, double *frames, double *xy, int32_t *slot, int32_t *id,
                              int64_t *frame_offsets, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    const bool points = xy || slot || id || frame_offsets;
    PCSEG_REQUIRE(refined_check(in) && table_workspace && refined && resolution && frames && workspace &&
                      (!points || (xy && slot && id && frame_offsets)),
                  "bad arguments");
    Carver tv(const_cast<void *>(table_workspace), table_workspace_bytes);
    const TableOffsets tb = table_offsets(tv, in->B);
    Carver cv(workspace, workspace_bytes);
    const RefinedWs ws = refined_carve(cv, in->B, in->cap);
    const long long *pt_offsets = ws.offsets;
    int *acc = ws.acc;
    if (!tv.fits("refined_table_write") || !cv.fits("refined_table_write")) return PCSEG_ERR_WORKSPACE;
    PCSEG_LAUNCH(rf_write_kernel, dim3(in->B), dim3(256), 0, (hipStream_t)stream, *in, tb, pt_offsets, acc, refined, resolution,
                 frames, xy, slot, id, (long long *)frame_offsets);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
