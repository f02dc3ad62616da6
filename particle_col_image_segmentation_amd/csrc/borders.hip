// Borders between touching regions of a label image L, weighed by a probability image V, and the merge of the regions whose
// border is weak (the definitions: include/pcseg.h).  Integers and exact float32 minima throughout: any atomic order gives the
// same table, the same map and the same merged image.
//
// pcseg_label_borders / pcseg_label_borders_write: the two-call protocol of pair_table.h.
//   border_fill_kernel   the column walk of terr_pairs_kernel (voronoi.hip): a lane owns one column of a 32-row block and keeps one
//                        open accumulator per link direction (right, down, and for conn = 8 down-right, down-left); equal
//                        consecutive pairs add up in registers (links 32-bit, sum 64-bit, saddle a min of float bits), at the end
//                        of the block neighbouring lanes with the same open pair are summed by the segmented shuffle and the head
//                        lane makes one table update.  A row is fetched ONCE, as the row below the one being linked: its left and
//                        right neighbours come from the neighbouring lanes by shuffle (the first and the last lane of a wave fetch
//                        the one column the shuffle cannot give), and it becomes the current row of the next step in registers.
//                        A link belongs to its upper (for "right": its left) pixel, so every seam link has one owner: the block
//                        fetches the row below its last one, and the columns beside its first and last.
//   pair_write_kernel    (pair_table.h, with BorderEmit) the used slots of a frame as rows (key, frame, links, sum, saddle), in
//                        table order.  Was border_write_kernel
// pcseg_border_merge:
//   border_merge_kernel  one block per frame: union-find over the labels 1 .. count with a joined pair as an edge (hooking to the
//                        smaller label, fenced walks), parents in LDS where cap + 1 fits and in the workspace otherwise; the
//                        groups' numbers are a block scan over the roots, in label order
// pcseg_relabel_map:
//   relabel_map_kernel   out = map[b, L]
#include "label_reduce.h"
#include "pair_table.h"
#include "union_find.h"

namespace pcseg {

constexpr int BD_COLS = 256;            // columns of a block: one per lane
constexpr int BD_ROWS = RUN_ROWS;       // rows of a block
constexpr int BD_LDS_LABELS = 8192;     // cap + 1 up to which the merge keeps its parents in LDS (32 KB)
constexpr int BD_MERGE_THREADS = 1024;  // threads of the merge's one block per frame
constexpr int BD_ABOVE_CAP = 2;         // flag bit: a label above cap was seen (and read as 0)
constexpr int BD_VALUE = 4;             // flag bit: a NaN or a value outside [0, 1] was seen (read as 0 / clamped)
constexpr int BD_CORRUPT = 8;           // flag bit: the merge met a parent entry outside its fence
constexpr unsigned BD_NO_SADDLE = 0xFFFFFFFFu;

// the slot of a pair: its links, its saddle and the 64-bit sum of its link values in the four counters of a PairTable<4> slot --
// [0] links, [1] ~(bits of the smallest link value) under an atomic max: a zero-filled slot reads as "no value yet" (bits
// 0xFFFFFFFF, above every float in [0, 1]), [2..3] the sum as ONE aligned 64-bit word (the counters start on a 256-byte
// boundary and a slot is 16 bytes)
constexpr int BORDER_NV = 4;
enum { BORDER_LINKS = 0, BORDER_SADDLE = 1, BORDER_SUM = 2 };

// rint(v 2^32) of a float32 in [0, 1], ties to even, in integer arithmetic.  From 2^-9 on a float32 is a multiple of 2^-32 and
// the result is a shift of its mantissa; below, the mantissa is rounded at the bit that 2^-32 leaves
__device__ __forceinline__ unsigned long long prob_fixed(float v)
{
    const unsigned u = __float_as_uint(v);
    const int e = (int)(u >> 23);  // (no sign bit: v >= +0)
    const unsigned m = (u & 0x7FFFFFu) | 0x800000u;
    const int sh = e - 118;  // v = m 2^(e - 150)
    if (sh >= 0) return (unsigned long long)m << sh;  // (e <= 127: at most 2^32)
    const int s = -sh;
    if (e == 0 || s > 25) return 0;
    const unsigned q = m >> s, rem = m & ((1u << s) - 1u), half = 1u << (s - 1);
    return q + (unsigned)(rem > half || (rem == half && (q & 1u)));
}

struct BdPx {
    int l;    // 0 .. cap
    float v;  // [0, 1]
};

// a pixel as the definitions read it; raises the lane's flag bits
__device__ __forceinline__ BdPx bd_read(int l, float v, int cap, int &flags)
{
    flags |= (l > cap ? BD_ABOVE_CAP : 0) | (!(v >= 0.f && v <= 1.f) ? BD_VALUE : 0);
    return BdPx{(unsigned)l <= (unsigned)cap ? l : 0, v > 0.f ? (v < 1.f ? v : 1.f) : 0.f};  // (NaN and -0: +0)
}

struct BdRaw {
    int l, le;  // the lane's column and its wave-edge column
    float v, ve;
};
__device__ __forceinline__ void landed(const BdRaw &q) { asm volatile("" ::"v"(q.l), "v"(q.le), "v"(q.v), "v"(q.ve) : "memory"); }

struct BdAcc {
    unsigned long long key;  // a << 32 | b, a < b; 0 = none
    unsigned long long sum;
    unsigned n, saddle;  // saddle: the bits of the smallest link value
};

template <int CONN>
__global__ void __launch_bounds__(256) border_fill_kernel(const int *__restrict__ lab, const float *__restrict__ val, long long val_stride,
                                                           int cap, int H, int W, unsigned long long *__restrict__ keys,
                                                           unsigned *__restrict__ cnt, int *__restrict__ overflow, int pair_cap)
{
    const TileIndex ti = xcd_tile_index();
    const int b = ti.z;
    const PairTable<BORDER_NV> tab = pair_table_of<BORDER_NV>(keys, cnt, overflow, pair_cap, b);
    const int c = ti.x * BD_COLS + threadIdx.x;
    const int r0 = ti.y * BD_ROWS, r1 = min(H, r0 + BD_ROWS);
    const int *fl = lab + (int64_t)b * H * W;
    const float *fv = val + (int64_t)b * val_stride;
    const int lane = lane_id();
    // the column a shuffle cannot give: the first lane of a wave fetches its left neighbour, the last lane its right one
    const int ce = lane == 0 ? c - 1 : c + 1;
    const bool in = c < W, edge = (lane == 0 || lane == WAVE - 1) && ce >= 0 && ce < W;
    int flags = 0;
    // (every lane stays for the shuffles: a lane past the width carries label 0 and links nothing)
    auto load = [&](int r) {
        BdRaw q{0, 0, 0.f, 0.f};
        if (r < H) {
            const int64_t off = rowoff(r, W);
            if (in) {
                q.l = fl[off + c];
                q.v = fv[off + c];
            }
            if (edge) {
                q.le = fl[off + ce];
                q.ve = fv[off + ce];
            }
        }
        return q;
    };
    // own pixel, left and right neighbour of a fetched row
    auto spread = [&](const BdRaw &q, BdPx &own, BdPx &left, BdPx &right) {
        own = bd_read(q.l, q.v, cap, flags);
        const BdPx e = bd_read(q.le, q.ve, cap, flags);
        left = BdPx{__shfl_up(own.l, 1), __shfl_up(own.v, 1)};
        right = BdPx{__shfl_down(own.l, 1), __shfl_down(own.v, 1)};
        if (lane == 0) left = e;
        if (lane == WAVE - 1) right = e;
    };
    auto commit = [&](const BdAcc &a) {
        const int s = pair_slot(tab, a.key);
        if (s < 0) return;
        unsigned *at = tab.cnt + BORDER_NV * (size_t)s;
        atomicAdd(at + BORDER_LINKS, a.n);
        atomicMax(at + BORDER_SADDLE, ~a.saddle);
        atomicAdd(reinterpret_cast<unsigned long long *>(at + BORDER_SUM), a.sum);
    };
    auto feed = [&](BdAcc &a, const BdPx &p, const BdPx &q) {
        if (p.l > 0 && q.l > 0 && p.l != q.l) {
            const unsigned long long key = ((unsigned long long)(unsigned)min(p.l, q.l) << 32) | (unsigned)max(p.l, q.l);
            if (key != a.key) {
                if (a.key) commit(a);
                a = BdAcc{key, 0ull, 0u, BD_NO_SADDLE};
            }
            const float ridge = fmaxf(p.v, q.v);
            ++a.n;
            a.sum += prob_fixed(ridge);
            a.saddle = min(a.saddle, __float_as_uint(ridge));  // (non-negative floats order like their bits)
        }
    };
    BdAcc acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = BdAcc{0ull, 0ull, 0u, BD_NO_SADDLE};
    BdPx own, left, right;
    spread(load(r0), own, left, right);
    BdRaw next = load(r0 + 1);
    for (int r = r0; r < r1; ++r) {
        const BdRaw now = next;  // row r + 1: the seam row of the next block for r + 1 = r1, nothing past the frame
        landed(now);
        if (r + 2 <= r1) next = load(r + 2);
        BdPx dn, dl, dr;
        spread(now, dn, dl, dr);
        feed(acc[0], own, right);
        feed(acc[1], own, dn);
        if (CONN == 8) {
            feed(acc[2], own, dr);
            feed(acc[3], own, dl);
        }
        own = dn;
        right = dr;
    }
#pragma unroll
    for (int k = 0; k < (CONN == 8 ? 4 : 2); ++k) {
        BdAcc a = acc[k];
        const WaveSeg seg = wave_segment(a.key);
        segment_reduce(
            a, seg.remain,
            [](const BdAcc &x, int off) { return BdAcc{x.key, __shfl_down(x.sum, off), __shfl_down(x.n, off), __shfl_down(x.saddle, off)}; },
            [](BdAcc &x, const BdAcc &o) { x.sum += o.sum; x.n += o.n; x.saddle = min(x.saddle, o.saddle); });
        if (seg.head && a.key) commit(a);
    }
    if (__any(flags)) {
        for (int off = 32; off >= 1; off >>= 1) flags |= __shfl_xor(flags, off);
        if (lane == 0) atomicOr(overflow + b, flags);
    }
}

// a used slot as the row (key, frame, links, sum, saddle) of pair_table.h's writer
struct BorderEmit {
    static constexpr int NV = BORDER_NV;
    long long *key_out;
    int *frame_out, *links_out;
    long long *sum_out;
    float *saddle_out;
    __device__ __forceinline__ void operator()(int b, unsigned long long key, const unsigned *c, long long row) const
    {
        key_out[row] = (long long)key;
        frame_out[row] = b;
        links_out[row] = (int)c[BORDER_LINKS];
        sum_out[row] = (long long)*reinterpret_cast<const unsigned long long *>(c + BORDER_SUM);
        saddle_out[row] = __uint_as_float(~c[BORDER_SADDLE]);
    }
};

// (1024 threads: one block per frame scans the whole table, 64 blocks on 256 CUs -- the kernel is latency, not work)
// LDS: cap + 1 <= BD_LDS_LABELS, the parents live in the block's LDS; otherwise in gpar (B, cap + 1)
template <bool LDS>
__global__ void __launch_bounds__(BD_MERGE_THREADS) border_merge_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ cnt,
                                                            int pair_cap, int cap, const int *__restrict__ counts,
                                                            unsigned long long t_fixed, float t_float, int by_saddle,
                                                            int *__restrict__ flags, int *__restrict__ gpar, int *__restrict__ map,
                                                            int *__restrict__ n_merged)
{
    __shared__ int spar[LDS ? BD_LDS_LABELS : 1];
    __shared__ int wsum[BD_MERGE_THREADS / WAVE];
    __shared__ int corrupt;
    const int b = blockIdx.x, tid = threadIdx.x;
    int *par = LDS ? spar : gpar + (int64_t)b * (cap + 1);
    int *m = map + (int64_t)b * (cap + 1);
    const int count = counts ? min(max(counts[b], 0), cap) : cap;
    if (flags[b] & PAIR_TABLE_FULL) {  // (the whole block: an incomplete table is no graph)
        for (int l = tid; l <= cap; l += BD_MERGE_THREADS) m[l] = l <= count ? l : 0;
        if (tid == 0) n_merged[b] = count;
        return;
    }
    if (tid == 0) corrupt = 0;
    for (int l = tid; l <= cap; l += BD_MERGE_THREADS) __hip_atomic_store(par + l, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const unsigned long long *k = keys + (int64_t)b * pair_cap;
    const unsigned *v = cnt + (int64_t)b * pair_cap * BORDER_NV;
    for (int i = tid; i < pair_cap; i += BD_MERGE_THREADS) {
        const unsigned long long key = k[i];
        const unsigned la = (unsigned)(key >> 32), lb = (unsigned)key;
        if (key == 0 || la < 1 || lb < 1 || la > (unsigned)count || lb > (unsigned)count || la == lb) continue;
        const unsigned *c = v + BORDER_NV * (size_t)i;
        const unsigned long long links = c[BORDER_LINKS], sum = *reinterpret_cast<const unsigned long long *>(c + BORDER_SUM);
        const bool joined = by_saddle ? __uint_as_float(~c[BORDER_SADDLE]) < t_float : sum < t_fixed * links;
        if (joined) unite_glb(par, (int)la, (int)lb, &corrupt);
    }
    __syncthreads();
    // the roots are their groups' smallest members: numbering them in label order is the numbering by smallest member
    int base = 0;
    for (int l0 = 0; l0 <= cap; l0 += BD_MERGE_THREADS) {
        const int l = l0 + tid;
        const bool root = l >= 1 && l <= count && find_glb(par, l, &corrupt) == l;
        int tot;
        const int pos = block_exclusive_scan<BD_MERGE_THREADS>((int)root, &tot, wsum);
        if (l <= cap) m[l] = root ? base + pos + 1 : 0;
        base += tot;
    }
    __syncthreads();
    for (int l = 1 + tid; l <= count; l += BD_MERGE_THREADS) {
        const int r = find_glb(par, l, &corrupt);  // (fenced: 0 <= r <= l)
        if (r != l) m[l] = m[r];
    }
    __syncthreads();
    if (tid == 0) {
        n_merged[b] = base;
        if (corrupt) atomicOr(flags + b, BD_CORRUPT);
    }
}

// VEC: W % 4 == 0 and both images 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(256) relabel_map_kernel(const int *__restrict__ lab, const int *__restrict__ map, int cap,
                                                           int *__restrict__ out, int npx)
{
    const int b = blockIdx.y;
    const int *m = map + (int64_t)b * (cap + 1);
    const int *in = lab + (int64_t)b * npx;
    int *o = out + (int64_t)b * npx;
    auto look = [&](int l) { return (unsigned)l <= (unsigned)cap ? m[l] : 0; };
    const int i = (blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= npx) return;
    if (VEC) {
        const int4 q = ld_labels4(in + i);
        *reinterpret_cast<int4 *>(o + i) = make_int4(look(q.x), look(q.y), look(q.z), look(q.w));
    } else {
        o[i] = look(in[i]);
    }
}

// the workspace: the tables, and behind them (B, cap + 1) parents of the merge for where they do not fit its LDS
static inline size_t border_parents(int B, int cap) { return (size_t)B * ((size_t)cap + 1); }

static PairWs<BORDER_NV> border_carve(Carver &cv, int B, int pair_cap, int cap)
{
    return pairs_carve<BORDER_NV>(cv, B, pair_cap, border_parents(B, cap));
}

static inline bool border_sizes_ok(int B, int pair_cap, int cap) { return B >= 1 && B <= 65535 && pair_cap >= 1 && cap >= 1 && cap < (1 << 30); }

}  // namespace pcseg

using namespace pcseg;

extern "C" {

int pcseg_border_block(int32_t *rows_cols_lds)
{
    PCSEG_REQUIRE(rows_cols_lds, "bad arguments");
    rows_cols_lds[0] = BD_ROWS;
    rows_cols_lds[1] = BD_COLS;
    rows_cols_lds[2] = BD_LDS_LABELS;
    return PCSEG_OK;
}

size_t pcseg_label_borders_workspace_bytes(int B, int pair_cap, int cap)
{
    if (!border_sizes_ok(B, pair_cap, cap)) return 0;
    return carved_bytes(border_carve, B, pair_cap, cap);
}

int pcseg_label_borders(const int32_t *labels, const float *values, int64_t value_stride, int cap, int conn, int pair_cap,
                        int32_t *overflow, int64_t *offsets, int64_t *totals, int B, int H, int W, void *workspace,
                        size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels && values && overflow && offsets && totals && workspace && check_shape(B, H, W) &&
                      border_sizes_ok(B, pair_cap, cap) && value_stride >= (int64_t)H * W,
                  "bad arguments");
    PCSEG_REQUIRE(conn == 4 || conn == 8, "conn must be 4 or 8");
    Carver cv(workspace, workspace_bytes);
    const PairWs<BORDER_NV> ws = border_carve(cv, B, pair_cap, cap);
    if (!cv.fits("label_borders")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = pairs_begin(ws, overflow, B, pair_cap, s)) return rc;
    const dim3 grid((W + BD_COLS - 1) / BD_COLS, (H + BD_ROWS - 1) / BD_ROWS, B);
    if (conn == 8)
        PCSEG_LAUNCH(border_fill_kernel<8>, grid, dim3(256), 0, s, labels, values, (long long)value_stride, cap, H, W, ws.keys,
                     ws.cnt, overflow, pair_cap);
    else
        PCSEG_LAUNCH(border_fill_kernel<4>, grid, dim3(256), 0, s, labels, values, (long long)value_stride, cap, H, W, ws.keys,
                     ws.cnt, overflow, pair_cap);
    PCSEG_CHECK_LAUNCH();
    return pairs_finish(ws, overflow, offsets, totals, B, pair_cap, s);
}

int pcseg_label_borders_write(int pair_cap, int cap, const int64_t *offsets, int64_t *key, int32_t *frame, int32_t *links, int64_t *sum,
                              float *saddle, int B, const void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(offsets && key && frame && links && sum && saddle && workspace && border_sizes_ok(B, pair_cap, cap), "bad arguments");
    return pairs_write("label_borders_write", workspace, workspace_bytes, B, pair_cap, border_parents(B, cap), offsets,
                       BorderEmit{(long long *)key, frame, links, (long long *)sum, saddle}, stream);
}

int pcseg_border_merge(int pair_cap, int cap, const int32_t *counts, double below, int by, int32_t *flags, int32_t *map,
                       int32_t *n_merged, int B, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(flags && map && n_merged && workspace && border_sizes_ok(B, pair_cap, cap), "bad arguments");
    PCSEG_REQUIRE(below >= 0.0 && below <= 1.0, "the threshold must lie in [0, 1]");
    PCSEG_REQUIRE(by == PCSEG_BORDER_BY_MEAN || by == PCSEG_BORDER_BY_SADDLE, "by must be PCSEG_BORDER_BY_MEAN or PCSEG_BORDER_BY_SADDLE");
    Carver cv(workspace, workspace_bytes);
    const PairWs<BORDER_NV> ws = border_carve(cv, B, pair_cap, cap);
    if (!cv.fits("border_merge")) return PCSEG_ERR_WORKSPACE;
    const unsigned long long t_fixed = (unsigned long long)__builtin_rint(below * 4294967296.0);
    const float t_float = (float)below;
    const int by_saddle = by == PCSEG_BORDER_BY_SADDLE;
    hipStream_t s = (hipStream_t)stream;
    if (cap + 1 <= BD_LDS_LABELS)
        PCSEG_LAUNCH(border_merge_kernel<true>, dim3(B), dim3(BD_MERGE_THREADS), 0, s, (const unsigned long long *)ws.keys,
                     (const unsigned *)ws.cnt, pair_cap, cap, counts, t_fixed, t_float, by_saddle, flags, ws.tail, map, n_merged);
    else
        PCSEG_LAUNCH(border_merge_kernel<false>, dim3(B), dim3(BD_MERGE_THREADS), 0, s, (const unsigned long long *)ws.keys,
                     (const unsigned *)ws.cnt, pair_cap, cap, counts, t_fixed, t_float, by_saddle, flags, ws.tail, map, n_merged);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_relabel_map(const int32_t *labels, const int32_t *map, int cap, int32_t *out, int B, int H, int W, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels && map && out && check_shape(B, H, W) && cap >= 1 && cap < (1 << 30) && B <= 65535, "bad arguments");
    const int npx = H * W;
    const bool vec = W % 4 == 0 && (((uintptr_t)labels | (uintptr_t)out) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        PCSEG_LAUNCH(relabel_map_kernel<true>, dim3((npx / 4 + 255) / 256, B), dim3(256), 0, s, labels, map, cap, out, npx);
    else
        PCSEG_LAUNCH(relabel_map_kernel<false>, dim3((npx + 255) / 256, B), dim3(256), 0, s, labels, map, cap, out, npx);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
