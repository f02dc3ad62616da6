// Per-type nearest neighbours and pair-distance histograms of point sets, frame by frame (refine_boundaries.py:8-12,
// goal 3: for every cell of a strain the distance to its nearest neighbour of the same strain and of every other
// strain, and the distances between every pair of cells).  Exact: d2 = dx*dx + dy*dy with each product and the sum
// rounded on their own (cell_distance_kernel in tables.hip is compiled to fma(dx, dx, dy*dy): up to 1 ulp apart), d = sqrt(d2) / scale,
// minima taken on d2; histogram bins compare d2 against per-edge d2 thresholds found on the host by bisection over the
// same formula, so bin membership is exactly edges[k] <= d < edges[k+1].
//
// Launches (all asynchronous, no host read):
//   nb_partition_kernel  one block per frame: the frame's points, grouped by type slot (slots >= K last), into
//                        workspace arrays; per-frame slot starts and the frame's number of work items
//   nb_items_scan_kernel one block: exclusive prefix of the work items over the frames
//   nb_pairs_kernel      persistent grid: work item = (frame, 256-point query tile, candidate split); candidate tiles of
//                        ONE slot stream through LDS (every lane reads the same candidate: a broadcast), queries in
//                        registers; per (split, query, slot) minimum into the workspace; pairs j > i (sorted order) into
//                        an LDS histogram, flushed with one global atomic per non-zero bin
//   nb_merge_kernel      one thread per point: minimum over the splits, -> distance, in the caller's point order
//   nb_hist_finish_kernel one thread per (frame, slot pair): n_pairs and the overflow count = n_pairs - sum of bins
#include "table_common.h"

namespace pcseg {

constexpr int NB_TILE = 256;
constexpr int NB_MAX_K = MAX_TYPE_SLOTS;
constexpr int NB_GRID = 1024;      // persistent blocks: 4 per CU
constexpr int NB_MAX_SPLITS = 8;

// candidate splits per query tile: enough work items to cover the persistent grid twice when the batch has few tiles
static int nb_splits(int64_t n, int B)
{
    const int64_t tiles = (n + NB_TILE - 1) / NB_TILE + B;
    const int64_t s = (2 * NB_GRID + tiles - 1) / tiles;
    return (int)(s < 1 ? 1 : (s > NB_MAX_SPLITS ? NB_MAX_SPLITS : s));
}

__device__ __forceinline__ int nb_pair_index(int a, int b, int K)
{
    // unordered slot pair (a <= b) -> row of the K (K + 1) / 2 rows, in (a, b) lexicographic order
    return a * K - a * (a - 1) / 2 + (b - a);
}

__device__ __forceinline__ int nb_lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
}

// sstart[b * (K + 2) + t] = first point of slot t inside frame b (t = K: points of no slot, K + 1: frame size)
__global__ void __launch_bounds__(256) nb_partition_kernel(const double *__restrict__ xy, const int32_t *__restrict__ slot,
                                                            const int32_t *__restrict__ id, const int64_t *__restrict__ foff,
                                                            int K, int S, double2 *__restrict__ sxy, int32_t *__restrict__ sid,
                                                            int32_t *__restrict__ sorig, int32_t *__restrict__ sstart,
                                                            int32_t *__restrict__ items)
{
    __shared__ int s_cnt[NB_MAX_K + 1], s_cur[NB_MAX_K + 1];
    const int b = blockIdx.x, lane = lane_id();
    const int64_t f0 = foff[b];
    const int n = (int)(foff[b + 1] - f0);
    if (threadIdx.x <= NB_MAX_K) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int cnt[NB_MAX_K + 1] = {0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += 256) {
        const int s = slot[f0 + i];
        const int c = (s >= 0 && s < K) ? s : K;
#pragma unroll
        for (int t = 0; t <= NB_MAX_K; ++t) cnt[t] += c == t;
    }
#pragma unroll
    for (int t = 0; t <= NB_MAX_K; ++t)
        if (cnt[t]) atomicAdd(&s_cnt[t], cnt[t]);
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        int32_t *st = sstart + (int64_t)b * (K + 2);
        for (int t = 0; t <= K; ++t) {
            st[t] = acc;
            s_cur[t] = acc;
            acc += s_cnt[t];
        }
        st[K + 1] = acc;
        items[b] = (s_cnt[K] == n ? 0 : (n - s_cnt[K] + NB_TILE - 1) / NB_TILE) * S;
    }
    __syncthreads();
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        const bool act = i < n;
        int c = -1;
        if (act) {
            const int s = slot[f0 + i];
            c = (s >= 0 && s < K) ? s : K;
        }
        int pos = 0;
        for (int t = 0; t <= K; ++t) {
            const unsigned long long m = __ballot(c == t);
            if (m == 0) continue;  // wave-uniform
            const int leader = __ffsll((long long)m) - 1;
            int w = 0;
            if (lane == leader) w = atomicAdd(&s_cur[t], __popcll(m));
            w = __shfl(w, leader);
            if (c == t) pos = w + nb_lanes_below(m);
        }
        if (act) {
            sxy[f0 + pos] = make_double2(xy[2 * (f0 + i)], xy[2 * (f0 + i) + 1]);
            sid[f0 + pos] = id[f0 + i];
            sorig[f0 + pos] = (int32_t)(f0 + i);
        }
    }
}

// prefix[b] = exclusive sum of items[0..b), prefix[B] = total
__global__ void __launch_bounds__(256) nb_items_scan_kernel(const int32_t *__restrict__ items, int32_t *__restrict__ prefix, int B)
{
    __shared__ int wsum[4];
    const int per = (B + 255) / 256, lo = min(B, (int)threadIdx.x * per), hi = min(B, lo + per);
    int v = 0;
    for (int b = lo; b < hi; ++b) v += items[b];
    int total;
    int acc = block_exclusive_scan<256>(v, &total, wsum);
    for (int b = lo; b < hi; ++b) {
        prefix[b] = acc;
        acc += items[b];
    }
    if (threadIdx.x == 0) prefix[B] = total;
}

struct NbArgs {
    const double2 *sxy;
    const int32_t *sid;
    const int32_t *sstart;
    const int32_t *prefix;
    const int64_t *foff;
    double *part_d2;   // (S, n, K)
    int32_t *part_id;  // (S, n, K)
    const double *thr;  // m + 1 thresholds on d2 (device), NULL = no histogram
    unsigned long long *hist;  // (B, P, m + 2): [n_pairs, bins.., over]
    int64_t n;
    int B, K, S, m;
};

// one candidate tile of slot-uniform points against the lane's query.  CHECK: the tile overlaps the query tile, so the
// query itself is skipped (by index) and only candidates j > i enter the histogram; HIST: the tile holds pairs to count
template <bool CHECK, bool HIST>
__device__ __forceinline__ void nb_scan_tile(const double2 *__restrict__ cxy, const int32_t *__restrict__ cid, int cnt, int j0,
                                             int i, double qx, double qy, double &bd, int &bid, const double *__restrict__ thr,
                                             int m, unsigned *__restrict__ hrow)
{
#pragma clang fp contract(off)  // each product and the sum rounded on their own (no FMA)
    const double tlast = HIST ? thr[m] : 0.0;
    for (int k = 0; k < cnt; ++k) {
        const double2 p = cxy[k];
        const int cand = cid[k];
        const double dx = qx - p.x, dy = qy - p.y;
        // written out rather than as __dadd_rn(__dmul_rn(..)): those are plain operators in hipcc's headers and -O3
        // contracts them to fma(dx, dx, dy * dy) (as it does in cell_distance_kernel); the pragma above forbids that
        const double d2 = dx * dx + dy * dy;
        bool better = d2 < bd || (d2 == bd && cand < bid);
        if (CHECK) better = better && j0 + k != i;
        bd = better ? d2 : bd;
        bid = better ? cand : bid;
        // thr[bin] <= d2 < thr[bin + 1]
        if (HIST && (!CHECK || j0 + k > i) && d2 < tlast) atomicAdd(&hrow[last_le(thr, m, d2)], 1u);
    }
}

__global__ void __launch_bounds__(256) nb_pairs_kernel(NbArgs a)
{
    extern __shared__ __align__(16) unsigned char nb_lds[];
    double2 *c_xy = (double2 *)nb_lds;
    int32_t *c_id = (int32_t *)(nb_lds + NB_TILE * sizeof(double2));
    double *s_thr = (double *)(nb_lds + NB_TILE * (sizeof(double2) + sizeof(int32_t)));
    const bool hist_on = a.thr != nullptr;
    unsigned *s_hist = (unsigned *)(s_thr + (hist_on ? a.m + 1 : 0));
    const int K = a.K, S = a.S, m = a.m, P = K * (K + 1) / 2, tid = threadIdx.x;
    if (hist_on)
        for (int k = tid; k <= m; k += 256) s_thr[k] = a.thr[k];
    const double nan = __longlong_as_double(0x7FF8000000000000LL), inf = __longlong_as_double(0x7FF0000000000000LL);
    const int total = a.prefix[a.B];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int b = last_le(a.prefix, a.B, item), local = item - a.prefix[b], qt = local / S, c = local - qt * S;
        const int64_t f0 = a.foff[b];
        const int32_t *st = a.sstart + (int64_t)b * (K + 2);
        const int nvalid = st[K], q0 = qt * NB_TILE, i = q0 + tid;
        const bool active = i < nvalid;
        int qslot = 0;
        double qx = nan, qy = nan;  // an idle lane's distances are NaN: no minimum, no histogram count
        if (active) {
            const double2 q = a.sxy[f0 + i];
            qx = q.x; qy = q.y;
            while (qslot + 1 < K && st[qslot + 1] <= i) ++qslot;
        }
        const int per = (nvalid + S - 1) / S, c0 = min(nvalid, c * per), c1 = min(nvalid, c0 + per);
        if (hist_on) {
            __syncthreads();  // the previous item's flush has read the histogram
            for (int k = tid; k < P * m; k += 256) s_hist[k] = 0;
        }
        for (int t = 0; t < K; ++t) {
            const int s0 = max(st[t], c0), s1 = min(st[t + 1], c1);
            double bd = inf;
            int bid = 0x7FFFFFFF;
            unsigned *hrow = s_hist + (hist_on ? nb_pair_index(min(qslot, t), max(qslot, t), K) * m : 0);
            for (int j0 = s0; j0 < s1; j0 += NB_TILE) {
                const int cnt = min(NB_TILE, s1 - j0);
                __syncthreads();  // every lane is done with the previous tile
                if (tid < cnt) {
                    c_xy[tid] = a.sxy[f0 + j0 + tid];
                    c_id[tid] = a.sid[f0 + j0 + tid];
                }
                __syncthreads();
                const bool overlap = j0 < q0 + NB_TILE && j0 + cnt > q0;
                const bool pairs = hist_on && j0 + cnt - 1 > q0;  // some candidate lies after some query
                if (overlap) {
                    if (pairs) nb_scan_tile<true, true>(c_xy, c_id, cnt, j0, i, qx, qy, bd, bid, s_thr, m, hrow);
                    else nb_scan_tile<true, false>(c_xy, c_id, cnt, j0, i, qx, qy, bd, bid, s_thr, m, hrow);
                } else if (pairs) {
                    nb_scan_tile<false, true>(c_xy, c_id, cnt, j0, i, qx, qy, bd, bid, s_thr, m, hrow);
                } else {
                    nb_scan_tile<false, false>(c_xy, c_id, cnt, j0, i, qx, qy, bd, bid, s_thr, m, hrow);
                }
            }
            if (active) {
                const int64_t o = ((int64_t)c * a.n + f0 + i) * K + t;
                a.part_d2[o] = bd;
                a.part_id[o] = bid;
            }
        }
        if (hist_on) {
            __syncthreads();
            unsigned long long *g = a.hist + (int64_t)b * P * (m + 2);
            for (int k = tid; k < P * m; k += 256) {
                const unsigned v = s_hist[k];
                const int p = k / m;
                if (v) atomicAdd(&g[(int64_t)p * (m + 2) + 1 + (k - p * m)], (unsigned long long)v);
            }
        }
    }
}

// point gi of the grouped order -> dist / nn_id rows of the caller's point sorig[gi]
__global__ void __launch_bounds__(256) nb_merge_kernel(NbArgs a, const int32_t *__restrict__ sorig, double scale,
                                                        double *__restrict__ dist, int32_t *__restrict__ nn_id)
{
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= a.n) return;
    const int K = a.K, b = last_le(a.foff, a.B, gi);
    const int32_t *st = a.sstart + (int64_t)b * (K + 2);
    const int i = (int)(gi - a.foff[b]);
    const int64_t o = sorig[gi];
    const double nan = __longlong_as_double(0x7FF8000000000000LL), inf = __longlong_as_double(0x7FF0000000000000LL);
    int s = K;
    for (int t = 0; t < K; ++t)
        if (st[t] <= i && i < st[t + 1]) s = t;
    for (int t = 0; t < K; ++t) {
        double out = nan;
        int oid = -1;
        if (s < K && st[t + 1] - st[t] - (t == s) > 0) {
            double bd = inf;
            int bid = 0x7FFFFFFF;
            for (int c = 0; c < a.S; ++c) {
                const double d2 = a.part_d2[((int64_t)c * a.n + gi) * K + t];
                const int cand = a.part_id[((int64_t)c * a.n + gi) * K + t];
                const bool better = d2 < bd || (d2 == bd && cand < bid);
                bd = better ? d2 : bd;
                bid = better ? cand : bid;
            }
            out = __ddiv_rn(__dsqrt_rn(bd), scale);
            oid = bid;
        }
        dist[o * K + t] = out;
        nn_id[o * K + t] = oid;
    }
}

__global__ void __launch_bounds__(256) nb_hist_finish_kernel(NbArgs a)
{
    const int K = a.K, P = K * (K + 1) / 2, m = a.m;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (int64_t)a.B * P) return;
    const int b = (int)(r / P), p = (int)(r - (int64_t)b * P);
    int sa = 0;
    while (nb_pair_index(sa, K - 1, K) < p) ++sa;  // the last row of slot a is (a, K - 1)
    const int sb = sa + p - nb_pair_index(sa, sa, K);
    const int32_t *st = a.sstart + (int64_t)b * (K + 2);
    const unsigned long long na = st[sa + 1] - st[sa], nb = st[sb + 1] - st[sb];
    const unsigned long long n_pairs = sa == sb ? na * (na - (na > 0)) / 2 : na * nb;
    unsigned long long *row = a.hist + r * (m + 2);
    unsigned long long sum = 0;
    for (int k = 0; k < m; ++k) sum += row[1 + k];
    row[0] = n_pairs;
    row[m + 1] = n_pairs - sum;
}

struct NbWorkspace {
    double2 *sxy;
    int32_t *sid, *sorig, *sstart, *items, *prefix, *part_id;
    double *part_d2, *thr;
};

static NbWorkspace nb_carve(Carver &cv, int64_t n, int B, int K, int n_edges, int S)
{
    NbWorkspace w;
    w.sxy = cv.take<double2>((size_t)n);
    w.sid = cv.take<int32_t>((size_t)n);
    w.sorig = cv.take<int32_t>((size_t)n);
    w.sstart = cv.take<int32_t>((size_t)B * (K + 2));
    w.items = cv.take<int32_t>((size_t)B);
    w.prefix = cv.take<int32_t>((size_t)B + 1);
    w.part_d2 = cv.take<double>((size_t)S * n * K);
    w.part_id = cv.take<int32_t>((size_t)S * n * K);
    w.thr = cv.take<double>((size_t)(n_edges > 0 ? n_edges : 1));
    return w;
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_neighbours_workspace_bytes(int64_t n_points, int B, int K, int n_edges)
{
    if (n_points < 0 || B < 1 || K < 1 || K > NB_MAX_K || n_edges < 0) return 0;
    return carved_bytes(nb_carve, n_points, B, K, n_edges, nb_splits(n_points, B));
}

int pcseg_point_neighbours(const double *xy, const int32_t *slot, const int32_t *id, const int64_t *frame_offsets, int64_t n_points,
                           int B, int K, double scale, const double *edges, int n_edges, double *dist, int32_t *nn_id,
                           int64_t *pair_hist, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    const bool edges_ok = n_edges == 0 ? (edges == nullptr && pair_hist == nullptr) : (hist_edges_ok(edges, n_edges) && pair_hist);
    PCSEG_REQUIRE(xy && slot && id && frame_offsets && dist && nn_id && workspace && B >= 1 && K >= 1 && K <= NB_MAX_K &&
                      n_points >= 0 && n_points < ((int64_t)1 << 24) && scale > 0.0 && std::isfinite(scale) && edges_ok,
                  "bad arguments");
    const int S = nb_splits(n_points, B), m = n_edges > 0 ? n_edges - 1 : 0, P = K * (K + 1) / 2;
    Carver cv(workspace, workspace_bytes);
    const NbWorkspace w = nb_carve(cv, n_points, B, K, n_edges, S);
    if (!cv.fits("point_neighbours")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    NbArgs a;
    a.sxy = w.sxy; a.sid = w.sid; a.sstart = w.sstart; a.prefix = w.prefix; a.foff = frame_offsets;
    a.part_d2 = w.part_d2; a.part_id = w.part_id;
    a.thr = n_edges > 0 ? w.thr : nullptr;
    a.hist = (unsigned long long *)pair_hist;
    a.n = n_points; a.B = B; a.K = K; a.S = S; a.m = m;
    if (n_edges > 0) {
        const int rc = upload_values(s, w.thr, n_edges, [=](int k) { return d2_threshold(edges[k], scale); });
        if (rc != PCSEG_OK) return rc;
        PCSEG_CHECK_HIP(hipMemsetAsync(pair_hist, 0, sizeof(int64_t) * (size_t)B * P * (m + 2), s));
    }
    PCSEG_LAUNCH(nb_partition_kernel, dim3(B), dim3(256), 0, s, xy, slot, id, frame_offsets, K, S, w.sxy, w.sid, w.sorig, w.sstart,
                 w.items);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(nb_items_scan_kernel, dim3(1), dim3(256), 0, s, (const int32_t *)w.items, w.prefix, B);
    PCSEG_CHECK_LAUNCH();
    if (n_points > 0) {
        const int64_t items_max = ((n_points + NB_TILE - 1) / NB_TILE + B) * S;
        const int grid = (int)(items_max < NB_GRID ? items_max : NB_GRID);
        const size_t lds = NB_TILE * (sizeof(double2) + sizeof(int32_t)) +
                           (n_edges > 0 ? sizeof(double) * (m + 1) + sizeof(unsigned) * (size_t)P * m : 0);
        PCSEG_LAUNCH(nb_pairs_kernel, dim3(grid), dim3(256), lds, s, a);
        PCSEG_CHECK_LAUNCH();
        PCSEG_LAUNCH(nb_merge_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, s, a, (const int32_t *)w.sorig, scale,
                     dist, nn_id);
        PCSEG_CHECK_LAUNCH();
    }
    if (n_edges > 0) {
        PCSEG_LAUNCH(nb_hist_finish_kernel, dim3((unsigned)(((int64_t)B * P + 255) / 256)), dim3(256), 0, s, a);
        PCSEG_CHECK_LAUNCH();
    }
    return PCSEG_OK;
}

int pcseg_neighbours_pack_cells(const double *cells, int ncol, const uint8_t *class_slot, int B, const void *table_workspace,
                                size_t table_workspace_bytes, double *xy, int32_t *slot, int32_t *id, int64_t *frame_offsets,
                                pcseg_stream_t stream)
{
    PCSEG_REQUIRE(cells && class_slot && table_workspace && xy && slot && id && frame_offsets && B >= 1 && ncol >= 14,
                  "bad arguments");
    return pack_cells<true>("neighbours_pack_cells", cells, ncol, class_slot, B, table_workspace, table_workspace_bytes, xy, slot, id,
                            frame_offsets, stream);
}

}  // extern "C"
