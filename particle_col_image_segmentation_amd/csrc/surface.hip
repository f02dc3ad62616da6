// Distance of every cell to the particle surface and colonisation profiles, batched
// (HCN_nanosims_rois_activity_distance_5iso_YG.m:271-309: distance of every ROI to the aggregate boundary).
//
// Surface S of a 0/1 mask M = pixels of M with a 4-neighbour outside M (outside the image counts as outside M): the point
// set of bwboundaries.  Everything works on BIT WORDS: uint32 (B, H, WW), WW = ceil(W / 32), bit j of word w of a row =
// pixel column 32 w + j, bits at columns >= W are 0.
//
// Launches (all asynchronous, no host read):
//   sf_mask_bits_kernel   one wave per 64 pixels of a row: byte -> bit with a ballot (any width, any alignment)
//   sf_surface_kernel     one thread per word: S = M & ~(up & down & left & right); row counts by integer atomics
//   sf_row_scan_kernel    one block per frame: exclusive prefix of the row counts, the frame's count
//   sf_frame_scan_kernel  one block: exclusive prefix over the frames (B + 1 offsets)
//   sf_points_kernel      one wave per row: the set bits as (row, col), raster order (count -> scan -> write)
//   sf_search_kernel      one wave per query: lanes own the rows r0, r0 + 1, r0 - 1, r0 + 2, .. outward from the query's
//                         row; a lane walks its row's words left and right of the query column (clz / ctz) until it
//                         meets a bit or the column distance alone exceeds the best d2; a row is skipped once
//                         fl(dr * dr) > best d2 and the wave stops when that holds for 64 rows in a row.  All prunes are
//                         STRICT (an equal d2 with a smaller raster index must still be seen) and safe in floating
//                         point because rounding is monotone: d2 = fl(fl(dr*dr) + fl(dc*dc)) >= fl(dr*dr), fl(dc*dc).
//                         A wave-wide minimum on (d2, raster index) ends every round of 64 rows.  Lane 0 also counts the
//                         query into the (frame, side, slot) histogram: one 64-bit global atomic (integer: any order).
//   sf_zero_image_kernel  the image pcseg_edt_sq_u8 takes: 0 on S, 1 elsewhere
//   sf_shell_kernel       D2 of every pixel against integer thresholds: LDS histogram per block and side, one 64-bit
//                         global atomic per non-zero bin
//   sf_hist_finish_kernel column 0 of every histogram row = sum of its bins and overflow
#include "table_common.h"

// each product and the sum of d2 rounded on their own (no FMA), everywhere in this file
#pragma clang fp contract(off)

namespace pcseg {

constexpr double SF_QUERY_LIMIT = 16777216.0;  // |coordinate| above 2^24 (or NaN): no distance (d2 stays far below 2^53)

__global__ void __launch_bounds__(256) sf_mask_bits_kernel(const uint8_t *__restrict__ in, unsigned long long value_bits,
                                                            uint32_t *__restrict__ mbits, int64_t rows, int W, int WW)
{
    const int lane = lane_id();
    const int chunks = (W + 63) >> 6;
    const int64_t total = rows * chunks;
    for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < total; it += (int64_t)gridDim.x * 4) {
        const int64_t row = it / chunks;
        const int c = (int)(it - row * chunks);
        const int col = c * 64 + lane;
        bool bit = false;
        if (col < W) {
            const unsigned v = in[row * W + col];
            bit = v < 64 && ((value_bits >> v) & 1ull);
        }
        const unsigned long long m = __ballot(bit);
        if (lane == 0) mbits[row * WW + 2 * c] = (uint32_t)m;
        if (lane == 1 && 2 * c + 1 < WW) mbits[row * WW + 2 * c + 1] = (uint32_t)(m >> 32);
    }
}

__global__ void __launch_bounds__(256) sf_surface_kernel(const uint32_t *__restrict__ mbits, uint32_t *__restrict__ bits,
                                                          int32_t *__restrict__ rowcnt, int32_t *__restrict__ rowarea, int64_t rows,
                                                          int H, int WW)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * WW) return;
    const int64_t row = idx / WW;
    const int w = (int)(idx - row * WW), r = (int)(row % H);
    const uint32_t m = mbits[idx];
    uint32_t s = 0;
    if (m) {
        const uint32_t up = r > 0 ? mbits[idx - WW] : 0u, dn = r < H - 1 ? mbits[idx + WW] : 0u;
        const uint32_t lf = (m << 1) | (w > 0 ? mbits[idx - 1] >> 31 : 0u);
        const uint32_t rt = (m >> 1) | (w < WW - 1 ? mbits[idx + 1] << 31 : 0u);
        s = m & ~(up & dn & lf & rt);
    }
    bits[idx] = s;
    if (s) atomicAdd(&rowcnt[row], __popc(s));
    if (m) atomicAdd(&rowarea[row], __popc(m));
}

// rowoff[b * H + r] = surface points of frame b above row r; counts[b] = the frame's points, area[b] = its mask pixels
__global__ void __launch_bounds__(256) sf_row_scan_kernel(const int32_t *__restrict__ rowcnt, const int32_t *__restrict__ rowarea,
                                                           int32_t *__restrict__ rowoff, int64_t *__restrict__ counts,
                                                           int64_t *__restrict__ area, int H)
{
    __shared__ int wsum[4];
    __shared__ unsigned long long s_area;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) s_area = 0;
    __syncthreads();
    if (area) {
        unsigned long long mine = 0;
        for (int r = threadIdx.x; r < H; r += 256) mine += (unsigned long long)rowarea[(int64_t)b * H + r];
        if (mine) atomicAdd(&s_area, mine);
    }
    const int32_t *cnt = rowcnt + (int64_t)b * H;
    int32_t *off = rowoff + (int64_t)b * H;
    const int per = (H + 255) / 256, lo = min(H, (int)threadIdx.x * per), hi = min(H, lo + per);
    int v = 0;
    for (int r = lo; r < hi; ++r) v += cnt[r];
    int total;
    int acc = block_exclusive_scan<256>(v, &total, wsum);  // (its barriers also order the adds to s_area before the read below)
    for (int r = lo; r < hi; ++r) {
        off[r] = acc;
        acc += cnt[r];
    }
    if (threadIdx.x == 0) {
        counts[b] = total;
        if (area) area[b] = (int64_t)s_area;
    }
}

// offsets[b] = exclusive sum of counts[0..b), offsets[B] = total
__global__ void __launch_bounds__(256) sf_frame_scan_kernel(const int64_t *__restrict__ counts, int64_t *__restrict__ offsets, int B)
{
    __shared__ long long wsum[4];
    const int per = (B + 255) / 256, lo = min(B, (int)threadIdx.x * per), hi = min(B, lo + per);
    long long v = 0;
    for (int b = lo; b < hi; ++b) v += counts[b];
    long long total;
    long long acc = block_exclusive_scan<256>(v, &total, wsum);
    for (int b = lo; b < hi; ++b) {
        offsets[b] = acc;
        acc += counts[b];
    }
    if (threadIdx.x == 0) offsets[B] = total;
}

__global__ void __launch_bounds__(256) sf_points_kernel(const uint32_t *__restrict__ bits, const int32_t *__restrict__ rowcnt,
                                                         const int32_t *__restrict__ rowoff, const int64_t *__restrict__ offsets,
                                                         int32_t *__restrict__ points, int64_t points_cap, int64_t rows, int H, int WW)
{
    const int lane = lane_id();
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        if (rowcnt[row] == 0) continue;  // wave-uniform
        const int64_t b = row / H;
        const int r = (int)(row - b * H);
        int64_t base = offsets[b] + rowoff[row];
        for (int w0 = 0; w0 < WW; w0 += 64) {
            const int w = w0 + lane;
            uint32_t s = w < WW ? bits[row * WW + w] : 0u;
            const int c = __popc(s);
            const int inc = wave_inclusive_sum(c);
            int64_t pos = base + inc - c;
            while (s) {
                const int bit = __ffs((int)s) - 1;
                s &= s - 1;
                if (pos < points_cap) {
                    points[2 * pos] = r;
                    points[2 * pos + 1] = w * 32 + bit;
                }
                ++pos;
            }
            base += __shfl(inc, 63);
        }
    }
}

struct SfSearchArgs {
    const double *rc;        // (n, 2) query (row, col)
    const int32_t *slot;     // (n) type slot of the query (histogram only), may be NULL
    const int64_t *foff;     // (B + 1)
    const uint32_t *bits;    // (B, H, WW)
    const int64_t *counts;   // (B) surface points per frame, may be NULL (then an empty frame is searched in full)
    const uint8_t *mask;     // (B, H, W), may be NULL
    const double *thr;       // m + 1 thresholds on d2, NULL = no histogram
    unsigned long long *hist;  // (B, 2, K, m + 2)
    double *dist;
    int32_t *nearest;
    uint8_t *inside;
    int32_t *rows_visited;   // (n) rows whose words were read (measurement aid), may be NULL
    int64_t n;
    double scale;
    int B, H, W, WW, K, m;
};

__device__ __forceinline__ void sf_take(double d2, int idx, double &bd, int &bidx)
{
    const bool better = d2 < bd || (d2 == bd && idx < bidx);
    bd = better ? d2 : bd;
    bidx = better ? idx : bidx;
}

__global__ void __launch_bounds__(256) sf_search_kernel(SfSearchArgs a)
{
    const int lane = lane_id();
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.n) return;  // wave-uniform
    const int b = last_le(a.foff, a.B, q), H = a.H, W = a.W, WW = a.WW;
    const double qr = a.rc[2 * q], qc = a.rc[2 * q + 1];
    const double inf = __longlong_as_double(0x7FF0000000000000LL), nan = __longlong_as_double(0x7FF8000000000000LL);
    const bool ok = fabs(qr) <= SF_QUERY_LIMIT && fabs(qc) <= SF_QUERY_LIMIT && (a.counts == nullptr || a.counts[b] > 0);
    double best = inf;
    int bidx = 0x7FFFFFFF, visited = 0;
    if (ok) {
        const double fr = floor(qr + 0.5), fc = floor(qc);
        const int r0 = fr < 0.0 ? 0 : (fr > (double)(H - 1) ? H - 1 : (int)fr);
        const int cl = fc < 0.0 ? -1 : (fc > (double)(W - 1) ? W - 1 : (int)fc);   // columns <= cl lie left of (or on) the query
        const int cr = fc < -1.0 ? 0 : (fc >= (double)(W - 1) ? W : (int)fc + 1);  // columns >= cr right of it (W: none)
        const uint32_t *fbits = a.bits + (int64_t)b * H * WW;
        for (int base = 0;; base += 64) {
            // lane j of the round: row r0 (j = 0), r0 + t (odd j), r0 - t (even j), t = (j + 1) / 2: on each side |dr| grows
            // with j, so once no lane of a round is live none of any later round can be
            const int j = base + lane, t = (j + 1) >> 1, row = (j & 1) ? r0 + t : r0 - t;
            const double dr = qr - (double)row, dr2 = dr * dr;
            const bool live = row >= 0 && row < H && !(dr2 > best);
            if (__ballot(live) == 0) break;
            double lbest = best;
            int lidx = bidx;
            if (live) {
                ++visited;
                const uint32_t *rp = fbits + rowoff(row, WW);
                const int rbase = __mul24(row, W);
                if (cl >= 0) {
                    int w = cl >> 5;
                    uint32_t m = rp[w] & (0xFFFFFFFFu >> (31 - (cl & 31)));
                    for (;;) {
                        if (m) {
                            const int col = w * 32 + 31 - __clz((int)m);
                            const double dc = qc - (double)col;
                            sf_take(dr2 + dc * dc, rbase + col, lbest, lidx);
                            break;
                        }
                        if (--w < 0) break;
                        const double dc = qc - (double)(w * 32 + 31);  // the nearest column of the next word
                        if (dr2 + dc * dc > lbest) break;
                        m = rp[w];
                    }
                }
                if (cr < W) {
                    int w = cr >> 5;
                    uint32_t m = rp[w] & (0xFFFFFFFFu << (cr & 31));
                    for (;;) {
                        if (m) {
                            const int col = w * 32 + __ffs((int)m) - 1;
                            const double dc = qc - (double)col;
                            sf_take(dr2 + dc * dc, rbase + col, lbest, lidx);
                            break;
                        }
                        if (++w >= WW) break;
                        const double dc = qc - (double)(w * 32);
                        if (dr2 + dc * dc > lbest) break;
                        m = rp[w];
                    }
                }
            }
            for (int o = 32; o >= 1; o >>= 1) {
                const double od = __shfl_xor(lbest, o);
                const int oi = __shfl_xor(lidx, o);
                sf_take(od, oi, lbest, lidx);
            }
            best = lbest;
            bidx = lidx;
        }
    }
    if (a.rows_visited) {
        for (int o = 32; o >= 1; o >>= 1) visited += __shfl_xor(visited, o);
    }
    if (lane != 0) return;
    const bool found = bidx != 0x7FFFFFFF;
    a.dist[q] = found ? __ddiv_rn(__dsqrt_rn(best), a.scale) : nan;
    a.nearest[2 * q] = found ? bidx / W : -1;
    a.nearest[2 * q + 1] = found ? bidx % W : -1;
    if (a.rows_visited) a.rows_visited[q] = visited;
    int side = 0;
    if (found && a.mask) {
        const double pr = floor(qr + 0.5), pc = floor(qc + 0.5);
        if (pr >= 0.0 && pr <= (double)(H - 1) && pc >= 0.0 && pc <= (double)(W - 1))
            side = a.mask[((int64_t)b * H + (int)pr) * W + (int)pc] != 0;
    }
    if (a.inside) a.inside[q] = (uint8_t)side;
    if (a.thr && found) {
        const int s = a.slot[q];
        if (s >= 0 && s < a.K) {
            const int klo = last_le(a.thr, a.m + 1, best);  // thr[klo] <= d2 < thr[klo + 1] (thr[0] = 0; klo = m: no upper bound)
            atomicAdd(&a.hist[(((int64_t)b * 2 + side) * a.K + s) * (a.m + 2) + 1 + klo], 1ull);
        }
    }
}

__global__ void __launch_bounds__(256) sf_hist_finish_kernel(unsigned long long *__restrict__ hist, int64_t rows, int m)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    unsigned long long *row = hist + r * (m + 2);
    unsigned long long sum = 0;
    for (int k = 0; k <= m; ++k) sum += row[1 + k];
    row[0] = sum;
}

__global__ void __launch_bounds__(256) sf_zero_image_kernel(const uint32_t *__restrict__ bits, uint8_t *__restrict__ img, int64_t rows,
                                                             int W, int WW)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * W) return;
    const int64_t row = idx / W;
    const int col = (int)(idx - row * W);
    img[idx] = ((bits[row * WW + (col >> 5)] >> (col & 31)) & 1u) ? 0 : 1;
}

// grid (blocks per frame, B); LDS: m + 1 thresholds (int64), then 2 (m + 1) counters
__global__ void __launch_bounds__(256) sf_shell_kernel(const int32_t *__restrict__ d2, const uint8_t *__restrict__ mask,
                                                        const int64_t *__restrict__ counts, const long long *__restrict__ thr, int m,
                                                        unsigned long long *__restrict__ shells, int HW)
{
    extern __shared__ __align__(16) unsigned char sf_lds[];
    long long *s_thr = (long long *)sf_lds;
    unsigned *s_hist = (unsigned *)(s_thr + m + 1);
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int k = tid; k <= m; k += 256) s_thr[k] = thr[k];
    for (int k = tid; k < 2 * (m + 1); k += 256) s_hist[k] = 0;
    __syncthreads();
    const bool empty = counts[b] == 0;  // no surface: the EDT's virtual zero pixel must not leak, everything is `over`
    const int32_t *fd = d2 + (int64_t)b * HW;
    const uint8_t *fm = mask + (int64_t)b * HW;
    for (int p = blockIdx.x * 256 + tid; p < HW; p += gridDim.x * 256) {
        const int side = fm[p] != 0;
        const int k = empty ? m : last_le(s_thr, m + 1, (long long)fd[p]);  // thr[k] <= d2 < thr[k + 1]
        atomicAdd(&s_hist[side * (m + 1) + k], 1u);
    }
    __syncthreads();
    for (int k = tid; k < 2 * (m + 1); k += 256) {
        const unsigned v = s_hist[k];
        const int side = k / (m + 1);
        if (v) atomicAdd(&shells[((int64_t)b * 2 + side) * (m + 2) + 1 + (k - side * (m + 1))], (unsigned long long)v);
    }
}

// refined points (label id, frame by frame) -> their centroids as the `refined` table prints them: sum / area
__global__ void __launch_bounds__(256) sf_pack_refined_kernel(const int64_t *__restrict__ ws_stats, int cap, const int32_t *__restrict__ id,
                                                               const int64_t *__restrict__ foff, int64_t n, int B, double *__restrict__ rc)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = last_le(foff, B, i);
    const int r = id[i] - 1;
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    double crow = nan, ccol = nan;
    if (r >= 0 && r < cap) {
        const int64_t *st = ws_stats + ((int64_t)b * cap + r) * 8;
        const double area = (double)st[0];
        crow = __ddiv_rn((double)st[1], area);
        ccol = __ddiv_rn((double)st[2], area);
    }
    rc[2 * i] = crow;
    rc[2 * i + 1] = ccol;
}

struct SfWorkspace {
    uint32_t *mbits;
    int32_t *rowcnt, *rowarea, *rowoff;  // (rowcnt and rowarea are one allocation: zeroed together)
    double *thr;
};

static SfWorkspace sf_carve(Carver &cv, int B, int H, int W)
{
    SfWorkspace w;
    const size_t WW = (size_t)(W + 31) / 32;
    w.mbits = cv.take<uint32_t>((size_t)B * H * WW);
    w.rowcnt = cv.take<int32_t>(2 * (size_t)B * H);
    w.rowarea = w.rowcnt + (size_t)B * H;
    w.rowoff = cv.take<int32_t>((size_t)B * H);
    w.thr = cv.take<double>(MAX_HIST_BINS + 1);
    return w;
}

struct SfShellWorkspace {
    uint8_t *img;
    int32_t *d2;
    long long *thr;
    void *edt;
    size_t edt_bytes;
};

static SfShellWorkspace sf_shell_carve(Carver &cv, int B, int H, int W)
{
    SfShellWorkspace w;
    w.img = cv.take<uint8_t>((size_t)B * H * W);
    w.d2 = cv.take<int32_t>((size_t)B * H * W);
    w.thr = cv.take<long long>(MAX_HIST_BINS + 1);
    w.edt_bytes = pcseg_edt_workspace_bytes(B, H, W);
    w.edt = cv.take<uint8_t>(w.edt_bytes);
    return w;
}

static int sf_grid(int64_t items, int per_block)
{
    const int64_t g = (items + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_surface_workspace_bytes(int B, int H, int W)
{
    if (!check_shape(B, H, W)) return 0;
    return carved_bytes(sf_carve, B, H, W);
}

int pcseg_surface_points(const uint8_t *in, uint64_t value_bits, uint32_t *bits, int64_t *counts, int64_t *offsets, int64_t *area,
                         int32_t *points, int64_t points_cap, int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(in && bits && counts && offsets && workspace && check_shape(B, H, W) && points_cap >= 0 &&
                      (points != nullptr || points_cap == 0),
                  "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const SfWorkspace w = sf_carve(cv, B, H, W);
    if (!cv.fits("surface_points")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int WW = (W + 31) / 32;
    const int64_t rows = (int64_t)B * H;
    PCSEG_CHECK_HIP(hipMemsetAsync(w.rowcnt, 0, sizeof(int32_t) * 2 * (size_t)rows, s));
    PCSEG_LAUNCH(sf_mask_bits_kernel, dim3(sf_grid(rows * ((W + 63) / 64), 16)), dim3(256), 0, s, in, (unsigned long long)value_bits, w.mbits,
                 rows, W, WW);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(sf_surface_kernel, dim3((unsigned)((rows * WW + 255) / 256)), dim3(256), 0, s, (const uint32_t *)w.mbits, bits, w.rowcnt,
                 w.rowarea, rows, H, WW);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(sf_row_scan_kernel, dim3(B), dim3(256), 0, s, (const int32_t *)w.rowcnt, (const int32_t *)w.rowarea, w.rowoff,
                 counts, area, H);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(sf_frame_scan_kernel, dim3(1), dim3(256), 0, s, (const int64_t *)counts, offsets, B);
    PCSEG_CHECK_LAUNCH();
    if (points) {
        PCSEG_LAUNCH(sf_points_kernel, dim3(sf_grid(rows, 4)), dim3(256), 0, s, (const uint32_t *)bits, (const int32_t *)w.rowcnt,
                     (const int32_t *)w.rowoff, (const int64_t *)offsets, points, points_cap, rows, H, WW);
        PCSEG_CHECK_LAUNCH();
    }
    return PCSEG_OK;
}

int pcseg_surface_distances(const double *rc, const int32_t *slot, const int64_t *frame_offsets, int64_t n_points,
                            const uint32_t *bits, const int64_t *counts, const uint8_t *mask, int B, int H, int W, double scale,
                            const double *edges, int n_edges, int K, double *dist, int32_t *nearest, uint8_t *inside, int64_t *hist,
                            int32_t *rows_visited, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    const bool edges_ok = n_edges == 0 ? (edges == nullptr && hist == nullptr)
                                       : (hist_edges_ok(edges, n_edges) && hist && slot && mask && K >= 1 && K <= MAX_TYPE_SLOTS);
    PCSEG_REQUIRE(rc && frame_offsets && bits && dist && nearest && workspace && check_shape(B, H, W) && n_points >= 0 &&
                      n_points < ((int64_t)1 << 31) && scale > 0.0 && std::isfinite(scale) && edges_ok,
                  "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const SfWorkspace w = sf_carve(cv, B, H, W);
    if (!cv.fits("surface_distances")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int m = n_edges > 0 ? n_edges - 1 : 0;
    if (n_edges > 0) {
        const int rc = upload_values(s, w.thr, n_edges, [=](int k) { return d2_threshold(edges[k], scale); });
        if (rc != PCSEG_OK) return rc;
        PCSEG_CHECK_HIP(hipMemsetAsync(hist, 0, sizeof(int64_t) * (size_t)B * 2 * K * (m + 2), s));
    }
    if (n_points > 0) {
        SfSearchArgs a;
        a.rc = rc; a.slot = slot; a.foff = frame_offsets; a.bits = bits; a.counts = counts; a.mask = mask;
        a.thr = n_edges > 0 ? w.thr : nullptr;
        a.hist = (unsigned long long *)hist;
        a.dist = dist; a.nearest = nearest; a.inside = inside; a.rows_visited = rows_visited;
        a.n = n_points; a.scale = scale; a.B = B; a.H = H; a.W = W; a.WW = (W + 31) / 32; a.K = K; a.m = m;
        PCSEG_LAUNCH(sf_search_kernel, dim3((unsigned)((n_points + 3) / 4)), dim3(256), 0, s, a);
        PCSEG_CHECK_LAUNCH();
    }
    if (n_edges > 0) {
        const int64_t rows = (int64_t)B * 2 * K;
        PCSEG_LAUNCH(sf_hist_finish_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (unsigned long long *)hist, rows, m);
        PCSEG_CHECK_LAUNCH();
    }
    return PCSEG_OK;
}

int pcseg_surface_thresholds(const double *edges, int n_edges, double scale, int64_t *out)
{
    PCSEG_REQUIRE(out && hist_edges_ok(edges, n_edges) && scale > 0.0 && std::isfinite(scale), "bad arguments");
    for (int k = 0; k < n_edges; ++k) out[k] = d2_threshold_int(edges[k], scale);
    return PCSEG_OK;
}

size_t pcseg_surface_shells_workspace_bytes(int B, int H, int W)
{
    if (!check_shape(B, H, W)) return 0;
    return carved_bytes(sf_shell_carve, B, H, W);
}

int pcseg_surface_shells(const uint32_t *bits, const int64_t *counts, const uint8_t *mask, int B, int H, int W, double scale,
                         const double *edges, int n_edges, int64_t *shells, void *workspace, size_t workspace_bytes,
                         pcseg_stream_t stream)
{
    PCSEG_REQUIRE(bits && counts && mask && shells && workspace && check_shape(B, H, W) && B <= 65535 && scale > 0.0 &&
                      std::isfinite(scale) && hist_edges_ok(edges, n_edges),
                  "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const SfShellWorkspace w = sf_shell_carve(cv, B, H, W);
    if (!cv.fits("surface_shells")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int m = n_edges - 1, WW = (W + 31) / 32, HW = H * W;
    const int64_t rows = (int64_t)B * H;
    int rc = upload_values(s, w.thr, n_edges, [=](int k) { return (long long)d2_threshold_int(edges[k], scale); });
    if (rc != PCSEG_OK) return rc;
    PCSEG_CHECK_HIP(hipMemsetAsync(shells, 0, sizeof(int64_t) * (size_t)B * 2 * (m + 2), s));
    PCSEG_LAUNCH(sf_zero_image_kernel, dim3((unsigned)((rows * W + 255) / 256)), dim3(256), 0, s, bits, w.img, rows, W, WW);
    PCSEG_CHECK_LAUNCH();
    rc = pcseg_edt_sq_u8(w.img, w.d2, B, H, W, -1, w.edt, w.edt_bytes, stream);
    if (rc != PCSEG_OK) return rc;
    int per_frame = (HW + 256 * 16 - 1) / (256 * 16);
    per_frame = per_frame > 128 ? 128 : per_frame;
    const size_t lds = sizeof(long long) * (m + 1) + sizeof(unsigned) * 2 * (size_t)(m + 1);
    PCSEG_LAUNCH(sf_shell_kernel, dim3(per_frame, B), dim3(256), lds, s, (const int32_t *)w.d2, mask, counts, (const long long *)w.thr, m,
                 (unsigned long long *)shells, HW);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(sf_hist_finish_kernel, dim3((unsigned)(((int64_t)B * 2 + 255) / 256)), dim3(256), 0, s, (unsigned long long *)shells,
                 (int64_t)B * 2, m);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_surface_pack_cells(const double *cells, int ncol, const uint8_t *class_slot, int B, const void *table_workspace,
                             size_t table_workspace_bytes, double *rc, int32_t *slot, int32_t *id, int64_t *frame_offsets,
                             pcseg_stream_t stream)
{
    PCSEG_REQUIRE(cells && class_slot && table_workspace && rc && slot && id && frame_offsets && B >= 1 && ncol >= 14,
                  "bad arguments");
    return pack_cells<false>("surface_pack_cells", cells, ncol, class_slot, B, table_workspace, table_workspace_bytes, rc, slot, id,
                             frame_offsets, stream);
}

int pcseg_surface_pack_refined(const int64_t *ws_stats, int cap, const int32_t *id, const int64_t *frame_offsets, int64_t n_points,
                               int B, double *rc, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(ws_stats && id && frame_offsets && rc && B >= 1 && cap >= 1 && n_points >= 0 && n_points < ((int64_t)1 << 31),
                  "bad arguments");
    if (n_points == 0) return PCSEG_OK;
    PCSEG_LAUNCH(sf_pack_refined_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws_stats, cap, id,
                 frame_offsets, n_points, B, rc);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
