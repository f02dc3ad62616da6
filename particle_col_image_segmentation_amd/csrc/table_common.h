// What the table-stage translation units (tables.hip, neighbours.hip, refined.hip, surface.hip) share: the layout of the
// table workspace, the class-value -> type-slot table, the block scan of the row writers, small host -> device uploads
// as kernel arguments, histogram edges and their exact thresholds, and the cells -> point-set packer.  Nothing in here
// multiplies and adds floating-point numbers, so it does not matter under which contraction mode an includer compiles.
#pragma once
#include <cmath>

#include "common.h"

namespace pcseg {

constexpr int MAX_HIST_BINS = 1024;  // bins of a distance histogram (pair_hist, surface_hist, surface_shells)
constexpr int MAX_TYPE_SLOTS = 4;    // cell-type slots of a point set
constexpr int ARG_CHUNK = 256;       // values handed to the device per launch, as a kernel argument

// ---- the table workspace (pcseg_table_workspace_bytes): THE definition of its head.  pcseg_table_layout leaves, for
// every frame b and row kind k, counts[b * 3 + k] rows and their first row offsets[b * 3 + k] in the dense table of that
// kind (exclusive prefix over the frames); tables.hip carves its private arrays behind them.  Every function that is
// handed a `table_workspace` reads it through table_offsets() and nothing else.
enum TableRows { ROWS_ROIS = 0, ROWS_CELLS = 1, ROWS_GROUPS = 2, ROW_KINDS = 3 };

struct TableOffsets {
    const long long *counts, *offsets;
    __device__ __forceinline__ long long count(int b, TableRows k) const { return counts[b * ROW_KINDS + k]; }
    __device__ __forceinline__ long long first(int b, TableRows k) const { return offsets[b * ROW_KINDS + k]; }
};

inline TableOffsets table_offsets(Carver &cv, int B)
{
    TableOffsets t;
    t.counts = cv.take<long long>(3 * (size_t)B);
    t.offsets = cv.take<long long>(3 * (size_t)B);
    return t;
}

struct ClassSlots {
    uint8_t slot[256];  // class value -> cell-type slot, 255 = not a cell type
    explicit ClassSlots(const uint8_t *table) { memcpy(slot, table, 256); }
    __device__ __forceinline__ int of(int cls) const  // the slot, -1 = not a cell type
    {
        const int s = slot[cls & 255];
        return s == 255 ? -1 : s;
    }
};

// the largest index i in [0, n) with arr[i] <= v, given arr[0] <= v and arr non-decreasing: the frame (or work-item
// owner) of a point in an offsets array -- empty frames share an offset, the last of them wins -- or the bin of a value
// in a threshold array.  The comparison is on the caller's own types.
template <typename T, typename V>
__device__ __forceinline__ int last_le(const T *arr, int n, V v)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (arr[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- up to ARG_CHUNK host values per launch into device memory, without a staging buffer or a host copy to wait for
template <typename T>
struct ArgChunk {
    T v[ARG_CHUNK];
};

template <typename T>
__global__ void __launch_bounds__(256) put_chunk_kernel(ArgChunk<T> c, int k0, int cnt, T *__restrict__ out)
{
    if ((int)threadIdx.x < cnt) out[k0 + threadIdx.x] = c.v[threadIdx.x];
}

// dst[k] = fn(k) for k in [0, n)
template <typename T, typename F>
inline int upload_values(hipStream_t stream, T *dst, int n, F fn)
{
    ArgChunk<T> c;
    for (int k0 = 0; k0 < n; k0 += ARG_CHUNK) {
        const int cnt = n - k0 < ARG_CHUNK ? n - k0 : ARG_CHUNK;
        for (int k = 0; k < cnt; ++k) c.v[k] = fn(k0 + k);
        PCSEG_LAUNCH(put_chunk_kernel<T>, dim3(1), dim3(256), 0, stream, c, k0, cnt, dst);
        PCSEG_CHECK_LAUNCH();
    }
    return PCSEG_OK;
}

// ---- histogram edges: m + 1 finite values, edges[0] = 0, strictly increasing, 1 <= m <= MAX_HIST_BINS
inline bool hist_edges_ok(const double *edges, int n_edges)
{
    if (!edges || n_edges < 2 || n_edges > MAX_HIST_BINS + 1) return false;
    for (int k = 0; k < n_edges; ++k)
        if (!std::isfinite(edges[k]) || (k == 0 ? edges[0] != 0.0 : !(edges[k] > edges[k - 1]))) return false;
    return true;
}

// Bin membership is exactly edges[k] <= d < edges[k + 1] with d = sqrt(d2) / scale as the kernels round it: the device
// compares d2 against per-edge thresholds on d2 that these two bisections find over the same formula (d is
// non-decreasing in d2).
// the smallest non-negative double t with d(t) >= e: a bisection over the ordered bit patterns
inline double d2_threshold(double e, double scale)
{
    auto val = [](uint64_t u) { double d; memcpy(&d, &u, 8); return d; };
    auto d = [scale](double d2) { return std::sqrt(d2) / scale; };
    uint64_t lo = 0, hi = 0x7FF0000000000000ULL;  // d(+inf) = inf >= e
    if (d(val(lo)) >= e) return 0.0;
    while (hi - lo > 1) {  // d(lo) < e <= d(hi)
        const uint64_t mid = lo + (hi - lo) / 2;
        if (d(val(mid)) >= e) hi = mid; else lo = mid;
    }
    return val(hi);
}

// the smallest integer n >= 0 with d((double)n) >= e (INT64_MAX when no n up to 2^53 reaches it)
inline int64_t d2_threshold_int(double e, double scale)
{
    auto d = [scale](int64_t n) { return std::sqrt((double)n) / scale; };
    if (d(0) >= e) return 0;
    int64_t lo = 0, hi = (int64_t)1 << 53;
    if (!(d(hi) >= e)) return INT64_MAX;
    while (hi - lo > 1) {  // d(lo) < e <= d(hi)
        const int64_t mid = lo + (hi - lo) / 2;
        if (d(mid) >= e) hi = mid; else lo = mid;
    }
    return hi;
}

// ---- the rows of `cells` (table_write_kernel) as a point set: coordinates, type slot (-1: none), label, frame offsets.
// XY1: (x, y) = (centroid_col + 1, centroid_row + 1), positions as MATLAB reports them (pcseg_point_neighbours);
// otherwise (centroid_row, centroid_col), 0-based (pcseg_surface_distances)
template <bool XY1>
__global__ void __launch_bounds__(256) pack_cells_kernel(const double *__restrict__ cells, int ncol, TableOffsets to, ClassSlots slots,
                                                          int B, double *__restrict__ pt, int32_t *__restrict__ slot,
                                                          int32_t *__restrict__ id, int64_t *__restrict__ foff)
{
    const int b = blockIdx.x;
    const long long row0 = to.first(b, ROWS_CELLS);
    const int n = (int)to.count(b, ROWS_CELLS);
    if (threadIdx.x == 0) {
        foff[b] = row0;
        if (b == B - 1) foff[B] = row0 + n;
    }
    for (int i = threadIdx.x; i < n; i += 256) {
        const double *r = cells + (row0 + i) * ncol;
        pt[2 * (row0 + i)] = XY1 ? r[6] + 1.0 : r[5];
        pt[2 * (row0 + i) + 1] = XY1 ? r[5] + 1.0 : r[6];
        slot[row0 + i] = slots.of((int)r[2]);
        id[row0 + i] = (int32_t)r[1];
    }
}

// behind pcseg_neighbours_pack_cells (XY1) and pcseg_surface_pack_cells, which check their arguments
template <bool XY1>
inline int pack_cells(const char *who, const double *cells, int ncol, const uint8_t *class_slot, int B, const void *table_workspace,
                      size_t table_workspace_bytes, double *pt, int32_t *slot, int32_t *id, int64_t *frame_offsets,
                      pcseg_stream_t stream)
{
    Carver cv(const_cast<void *>(table_workspace), table_workspace_bytes);
    const TableOffsets to = table_offsets(cv, B);
    if (!cv.fits(who)) return PCSEG_ERR_WORKSPACE;
    PCSEG_LAUNCH(pack_cells_kernel<XY1>, dim3(B), dim3(256), 0, (hipStream_t)stream, cells, ncol, to, ClassSlots(class_slot), B, pt, slot,
                 id, frame_offsets);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // namespace pcseg
