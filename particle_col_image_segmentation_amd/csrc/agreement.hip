// Agreement of two label images of a frame, a truth image T and a test image S: the contingency table n(t, s) = number of
// pixels with T = t and S = s, and what follows from it per label and per frame -- areas, best partners, IoU, the matches at
// a list of IoU thresholds and the integer sums behind the adapted Rand error.  Integers throughout (any atomic order gives
// the same table); the only floating-point operation is the one division of an IoU.
//
// pcseg_label_contingency / pcseg_contingency_write: the two-call protocol of pair_table.h.
//   ag_count_kernel      the column-run walk of label_reduce.h over BOTH images with the pair (t, s) as the key: a lane owns 4
//                        columns of a 32-row block, a vertical run of a constant pair adds up in registers, runs of
//                        neighbouring lanes with the same pair are summed by the segmented shuffle, and one table update per
//                        run and wave goes into the frame's open-addressing table (key t << 32 | s, one counter).  Every pair
//                        but (0, 0) is kept, so the marginals are row sums.  One read of each image, no per-pixel atomic.
//   pair_write_kernel    (pair_table.h, with AgEmit) the used slots of a frame as rows (key, frame, n), in table order.  Was
//                        ag_write_kernel
// pcseg_agreement_match: on the rows sorted by (frame, t, s)
//   ag_area_kernel       A_t, B_s, S_pp and the column sum of s = 0 by integer atomics, one thread per row
//   ag_best_kernel       per row with t, s >= 1: the partner counts, and the row competes for "best partner" of its t and of
//                        its s by a compare-and-swap loop on the label's best-row word under a STRICT total order (n / U by
//                        cross-multiplication, then the smaller partner) -- the winner does not depend on the order of arrival
//   ag_final_kernel      per label: partner, overlap, IoU, match bits; per frame: counts, N1, S_a, S_b, TP_k
#include "label_reduce.h"
#include "pair_table.h"

namespace pcseg {

constexpr int AG_NV = 1;       // one counter per pair: n < 2^30 (check_shape)
constexpr int AG_ABOVE_CAP = 2;  // overflow bit: a label above its cap was seen (and read as 0)
constexpr int AG_MAX_THR = 8;

struct AgRun {
    long long key;  // t << 32 | s; 0 = nothing
    int n;
};

struct AgRaw {
    int4 t, s;
};
__device__ __forceinline__ void landed(const AgRaw &q) { landed(q.t); landed(q.s); }

// VEC: W % 4 == 0 and both images 16-byte aligned (int4 loads); otherwise four guarded loads per row and image
template <bool VEC>
struct AgWalk {
    using Key = long long;
    using Raw = AgRaw;
    using Run = AgRun;
    const int *pt, *ps;  // the frame's two images
    int c, W, cap_t, cap_s;
    int *above;  // the lane's "saw a label above its cap" (a register of the kernel)
    PairTable<AG_NV> tab;
    __device__ __forceinline__ Raw load(int y) const
    {
        return Raw{row_labels4<VEC>(pt + rowoff(y, W), c, W), row_labels4<VEC>(ps + rowoff(y, W), c, W)};
    }
    __device__ __forceinline__ void keys(const Raw &q, Key k[4]) const
    {
        const int tv[4] = {q.t.x, q.t.y, q.t.z, q.t.w}, sv[4] = {q.s.x, q.s.y, q.s.z, q.s.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *above |= (tv[j] > cap_t) | (sv[j] > cap_s);
            // (one unsigned compare: negative values and values above the cap are background)
            const unsigned t = (unsigned)tv[j] <= (unsigned)cap_t ? (unsigned)tv[j] : 0u;
            const unsigned s = (unsigned)sv[j] <= (unsigned)cap_s ? (unsigned)sv[j] : 0u;
            k[j] = (long long)(((unsigned long long)t << 32) | s);
        }
    }
    __device__ __forceinline__ Run run(Key key, int start, int end, int) const { return Run{key, end - start}; }
    static __device__ __forceinline__ Run shfl(const Run &q, int off) { return Run{q.key, __shfl_down(q.n, off)}; }
    static __device__ __forceinline__ void merge(Run &q, const Run &o) { q.n += o.n; }
    __device__ __forceinline__ void commit(const Run &q) const { pair_add(tab, (unsigned long long)q.key, {(unsigned)q.n}); }
};

template <bool VEC>
__global__ void __launch_bounds__(256) ag_count_kernel(const int *__restrict__ lt, const int *__restrict__ ls, int cap_t, int cap_s,
                                                       int H, int W, unsigned long long *__restrict__ keys, unsigned *__restrict__ cnt,
                                                       int *__restrict__ overflow, int pair_cap)
{
    const TileIndex ti = xcd_tile_index();  // (a frame's blocks on one XCD: their atomics on the frame's table meet in one L2)
    const int b = ti.z;
    const int64_t npx = (int64_t)H * W;
    const int c = (ti.x * 256 + threadIdx.x) * 4;
    const int r0 = ti.y * RUN_ROWS;
    int above = 0;
    column_run_walk(AgWalk<VEC>{lt + b * npx, ls + b * npx, c, W, cap_t, cap_s, &above, pair_table_of<AG_NV>(keys, cnt, overflow, pair_cap, b)},
                    c, r0, min(H, r0 + RUN_ROWS));
    if (__any(above) && lane_id() == 0) atomicOr(overflow + b, AG_ABOVE_CAP);
}

// a used slot as the row (key, frame, n) of pair_table.h's writer
struct AgEmit {
    static constexpr int NV = AG_NV;
    long long *key_out;
    int *frame_out;
    long long *n_out;
    __device__ __forceinline__ void operator()(int b, unsigned long long key, const unsigned *c, long long row) const
    {
        key_out[row] = (long long)key;
        frame_out[row] = b;
        n_out[row] = (long long)c[0];
    }
};

// ---- the match step
// frame_ints columns
enum { AG_N_TRUTH = 0, AG_N_ROIS = 1, AG_N1 = 2, AG_SPP = 3, AG_SA = 4, AG_SB = 5, AG_TP = 6 };

struct AgThr {
    double v[AG_MAX_THR];
    int n;
};

struct AgRows {
    const long long *key, *n, *offsets;  // rows sorted by (frame, t, s); offsets (B + 1)
    int B, cap_t, cap_s;
};

__device__ __forceinline__ void add64(long long *p, long long v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }

// the frame of row i: the last b with offsets[b] <= i (frames without row share their offset with the next one)
__device__ __forceinline__ int ag_frame_of(const AgRows &R, long long i)
{
    int lo = 0, hi = R.B;  // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (R.offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// a row's labels, false where one lies outside the caps (such a row is ignored: it indexes nothing)
__device__ __forceinline__ bool ag_row(const AgRows &R, long long i, int &t, int &s)
{
    const unsigned long long key = (unsigned long long)R.key[i];
    const unsigned ut = (unsigned)(key >> 32), us = (unsigned)key;
    t = (int)ut;
    s = (int)us;
    return ut <= (unsigned)R.cap_t && us <= (unsigned)R.cap_s;
}

// (S_pp is one word per frame and the rows of a wave nearly always belong to one frame: the wave adds its squares up first --
// one atomic per wave instead of one per row; figures in DESIGN.md section 18)
__global__ void __launch_bounds__(256) ag_area_kernel(AgRows R, long long rows, long long *__restrict__ area_t,
                                                       long long *__restrict__ area_s, long long *__restrict__ frame_ints, int n_cols)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < rows;  // (every lane stays for the wave sum)
    int t = 0, s = 0;
    const bool ok = in && ag_row(R, i, t, s);
    const int b = in ? ag_frame_of(R, i) : -1;
    const long long n = ok ? R.n[i] : 0;
    long long sq = t >= 1 ? n * n : 0;
    if (ok) {
        long long *fi = frame_ints + (int64_t)b * n_cols;
        if (t >= 1) {
            add64(area_t + (int64_t)b * R.cap_t + t - 1, n);
            if (s == 0) add64(fi + AG_SB, n);  // the column sum of s = 0, squared by ag_best_kernel
        }
        if (s >= 1) add64(area_s + (int64_t)b * R.cap_s + s - 1, n);
    }
    const int b0 = __shfl(b, 0);  // (lane 0 holds the wave's first row: in the frame range if any lane is)
    if (__all(!in || b == b0)) {
        for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off);
        if (lane_id() == 0 && sq) add64(frame_ints + (int64_t)b0 * n_cols + AG_SPP, sq);
    } else if (sq) {
        add64(frame_ints + (int64_t)b * n_cols + AG_SPP, sq);
    }
}

// row i against the label's best row so far: `slot` holds 1 + the best row's position in the frame (0: none).  A row is better
// if its n / U is larger -- n1 U2 > n2 U1 in unsigned 64 bits: n < 2^30, U < 2^31 -- or equal with the smaller partner.
// own: the label's area; other: the areas of the partners' side; low: the partner is the key's low word
__device__ __forceinline__ void ag_compete(const AgRows &R, long long off, int rel, long long n1, int p1, long long own,
                                           const long long *__restrict__ other, bool low, int *slot)
{
    const unsigned long long u1 = (unsigned long long)(own + other[p1 - 1] - n1);
    int cur = ld_agent(slot);
    for (;;) {
        if (cur) {
            const long long j = off + cur - 1;
            const unsigned long long kj = (unsigned long long)R.key[j];
            const int p2 = low ? (int)(unsigned)kj : (int)(unsigned)(kj >> 32);
            const long long n2 = R.n[j];
            const unsigned long long u2 = (unsigned long long)(own + other[p2 - 1] - n2);
            const unsigned long long a = (unsigned long long)n1 * u2, c = (unsigned long long)n2 * u1;
            if (!(a > c || (a == c && p1 < p2))) return;
        }
        const int old = atomicCAS(slot, cur, rel + 1);
        if (old == cur) return;
        cur = old;  // (another row got in: every change of the word is an improvement under a strict order, so this ends)
    }
}

__global__ void __launch_bounds__(256) ag_best_kernel(AgRows R, long long rows, const long long *__restrict__ area_t,
                                                       const long long *__restrict__ area_s, int *__restrict__ best_t,
                                                       int *__restrict__ best_s, long long *__restrict__ frame_ints, int n_cols)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int b = ag_frame_of(R, i);
    const long long off = R.offsets[b];
    if (i == off) {  // (one thread per frame that has rows; a frame without row has a column sum of 0)
        long long *sb = frame_ints + (int64_t)b * n_cols + AG_SB;
        *sb = *sb * *sb;
    }
    int t, s;
    if (!ag_row(R, i, t, s) || t < 1 || s < 1) return;
    const long long n = R.n[i];
    const long long *at = area_t + (int64_t)b * R.cap_t, *as = area_s + (int64_t)b * R.cap_s;
    int *bt = best_t + ((int64_t)b * R.cap_t + t - 1) * 3, *bs = best_s + ((int64_t)b * R.cap_s + s - 1) * 3;
    atomicAdd(bt + 2, 1);
    atomicAdd(bs + 2, 1);
    const int rel = (int)(i - off);
    ag_compete(R, off, rel, n, s, at[t - 1], as, true, bt);
    ag_compete(R, off, rel, n, t, as[s - 1], at, false, bs);
}

// n(0, s) of frame b: its rows are sorted by key and those of t = 0 carry key = s
__device__ __forceinline__ long long ag_n0(const AgRows &R, int b, int s)
{
    long long lo = R.offsets[b], hi = R.offsets[b + 1];
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (R.key[mid] < (long long)s) lo = mid + 1;
        else hi = mid;
    }
    return (lo < R.offsets[b + 1] && R.key[lo] == (long long)s) ? R.n[lo] : 0;
}

// blockIdx.z: 0 the truth side, 1 the test side
__global__ void __launch_bounds__(256) ag_final_kernel(AgRows R, AgThr thr, const long long *__restrict__ area_t,
                                                        const long long *__restrict__ area_s, int *__restrict__ best_t,
                                                        int *__restrict__ best_s, double *__restrict__ iou_t, double *__restrict__ iou_s,
                                                        uint8_t *__restrict__ match_t, uint8_t *__restrict__ match_s,
                                                        long long *__restrict__ frame_ints, int n_cols)
{
    const bool truth = blockIdx.z == 0;
    const int cap = truth ? R.cap_t : R.cap_s, ocap = truth ? R.cap_s : R.cap_t;
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= cap) return;
    const int64_t at = (int64_t)b * cap + i;
    const long long A = (truth ? area_t : area_s)[at];
    const long long *other = (truth ? area_s : area_t) + (int64_t)b * ocap;
    int *best = (truth ? best_t : best_s) + at * 3;
    long long *fi = frame_ints + (int64_t)b * n_cols;
    if (A > 0) {
        add64(fi + (truth ? AG_N_TRUTH : AG_N_ROIS), 1);
        if (truth) {
            add64(fi + AG_N1, A);
            add64(fi + AG_SA, A * A);
        } else {
            const long long cs = A - ag_n0(R, b, i + 1);  // sum over t >= 1 of n(t, s)
            add64(fi + AG_SB, cs * cs);
        }
    }
    double iou = __longlong_as_double(0x7FF8000000000000ll);
    unsigned m = 0;
    const int rel = best[0];
    if (rel) {
        const long long row = R.offsets[b] + rel - 1;
        const unsigned long long key = (unsigned long long)R.key[row];
        const int p = truth ? (int)(unsigned)key : (int)(unsigned)(key >> 32);
        const long long n = R.n[row];
        const long long U = A + other[p - 1] - n;
        iou = (double)n / (double)U;
        best[0] = p;
        best[1] = (int)n;
        for (int k = 0; k < thr.n; ++k)
            if (2 * n > U && iou >= thr.v[k]) {
                m |= 1u << k;
                if (truth) add64(fi + AG_TP + k, 1);
            }
    }
    (truth ? iou_t : iou_s)[at] = iou;
    (truth ? match_t : match_s)[at] = (uint8_t)m;
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_contingency_workspace_bytes(int B, int pair_cap)
{
    if (B < 1 || pair_cap < 1) return 0;
    return carved_bytes(pairs_carve<AG_NV>, B, pair_cap, 0);
}

int pcseg_label_contingency(const int32_t *labels_t, const int32_t *labels_s, int cap_t, int cap_s, int pair_cap, int32_t *overflow,
                            int64_t *offsets, int64_t *totals, int B, int H, int W, void *workspace, size_t workspace_bytes,
                            pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels_t && labels_s && overflow && offsets && totals && workspace && check_shape(B, H, W) && cap_t >= 1 &&
                      cap_s >= 1 && pair_cap >= 1 && B <= 65535,
                  "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const PairWs<AG_NV> ws = pairs_carve<AG_NV>(cv, B, pair_cap, 0);
    if (!cv.fits("label_contingency")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = pairs_begin(ws, overflow, B, pair_cap, s)) return rc;
    const dim3 grid((W + 1023) / 1024, (H + RUN_ROWS - 1) / RUN_ROWS, B);
    const bool vec = W % 4 == 0 && (((uintptr_t)labels_t | (uintptr_t)labels_s) & 15) == 0;
    if (vec)
        PCSEG_LAUNCH(ag_count_kernel<true>, grid, dim3(256), 0, s, labels_t, labels_s, cap_t, cap_s, H, W, ws.keys, ws.cnt, overflow, pair_cap);
    else
        PCSEG_LAUNCH(ag_count_kernel<false>, grid, dim3(256), 0, s, labels_t, labels_s, cap_t, cap_s, H, W, ws.keys, ws.cnt, overflow, pair_cap);
    PCSEG_CHECK_LAUNCH();
    return pairs_finish(ws, overflow, offsets, totals, B, pair_cap, s);
}

int pcseg_contingency_write(int pair_cap, const int64_t *offsets, int64_t *key, int32_t *frame, int64_t *n, int B,
                            const void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(offsets && key && frame && n && workspace && B >= 1 && B <= 65535 && pair_cap >= 1, "bad arguments");
    return pairs_write("contingency_write", workspace, workspace_bytes, B, pair_cap, 0, offsets,
                       AgEmit{(long long *)key, frame, (long long *)n}, stream);
}

int pcseg_agreement_match(const int64_t *key, const int64_t *n, const int64_t *offsets, int64_t rows, int cap_t, int cap_s,
                          const double *thresholds, int n_thr, int64_t *area_t, int64_t *area_s, int32_t *best_t, double *iou_t,
                          int32_t *best_s, double *iou_s, uint8_t *match_t, uint8_t *match_s, int64_t *frame_ints, int B,
                          pcseg_stream_t stream)
{
    PCSEG_REQUIRE(offsets && area_t && area_s && best_t && iou_t && best_s && iou_s && match_t && match_s && frame_ints && B >= 1 &&
                      B <= 65535 && cap_t >= 1 && cap_s >= 1 && rows >= 0 && (rows == 0 || (key && n)),
                  "bad arguments");
    PCSEG_REQUIRE(n_thr >= 0 && n_thr <= AG_MAX_THR && (n_thr == 0 || thresholds), "0 to 8 thresholds");
    AgThr thr;
    thr.n = n_thr;
    for (int k = 0; k < AG_MAX_THR; ++k) {
        thr.v[k] = k < n_thr ? thresholds[k] : 2.0;
        PCSEG_REQUIRE(k >= n_thr || (thr.v[k] >= 0.5 && thr.v[k] <= 1.0), "a threshold must lie in [0.5, 1]");
    }
    hipStream_t s = (hipStream_t)stream;
    const int n_cols = AG_TP + n_thr;
    PCSEG_CHECK_HIP(hipMemsetAsync(area_t, 0, sizeof(int64_t) * (size_t)B * cap_t, s));
    PCSEG_CHECK_HIP(hipMemsetAsync(area_s, 0, sizeof(int64_t) * (size_t)B * cap_s, s));
    PCSEG_CHECK_HIP(hipMemsetAsync(best_t, 0, sizeof(int32_t) * 3 * (size_t)B * cap_t, s));
    PCSEG_CHECK_HIP(hipMemsetAsync(best_s, 0, sizeof(int32_t) * 3 * (size_t)B * cap_s, s));
    PCSEG_CHECK_HIP(hipMemsetAsync(frame_ints, 0, sizeof(int64_t) * (size_t)B * n_cols, s));
    const AgRows R{(const long long *)key, (const long long *)n, (const long long *)offsets, B, cap_t, cap_s};
    if (rows > 0) {
        PCSEG_REQUIRE(rows < ((int64_t)1 << 39), "too many rows");
        const dim3 grid((unsigned)((rows + 255) / 256));
        PCSEG_LAUNCH(ag_area_kernel, grid, dim3(256), 0, s, R, (long long)rows, (long long *)area_t, (long long *)area_s,
                     (long long *)frame_ints, n_cols);
        PCSEG_CHECK_LAUNCH();
        PCSEG_LAUNCH(ag_best_kernel, grid, dim3(256), 0, s, R, (long long)rows, (const long long *)area_t, (const long long *)area_s,
                     best_t, best_s, (long long *)frame_ints, n_cols);
        PCSEG_CHECK_LAUNCH();
    }
    const int cap = cap_t > cap_s ? cap_t : cap_s;
    PCSEG_LAUNCH(ag_final_kernel, dim3((cap + 255) / 256, B, 2), dim3(256), 0, s, R, thr, (const long long *)area_t,
                 (const long long *)area_s, best_t, best_s, iou_t, iou_s, match_t, match_s, (long long *)frame_ints, n_cols);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
