// Nearest-label transform (the exact Euclidean feature transform of a label image) and what follows from it per ROI:
// territories (discrete Voronoi cells, optionally limited to a reach) and the adjacency graph of the territories
// (scipy.ndimage.distance_transform_edt(return_indices=True), skimage.segmentation.expand_labels; include/pcseg.h).
//
// Integers only, so nothing depends on the order of the atomics.  The vertical pass (bit words whose targets are the SITES,
// carries, a row's distances, the staging of a row block) is column_pass.h, shared with edt.hip, where its carry kernel lives.
// Launches (asynchronous, no host read):
//   vor_bits_kernel      site bits of the label image, 32 rows of a column per word (a site: a label in 1 .. cap that `sel` keeps)
//   col_carry_kernel     (edt.hip) per column and word: distance from the word's first / last row to the nearest site above / below it
//   vor_row_kernel       a row block's vertical distances staged in LDS as (g, site above, site below); per pixel an expanding
//                        search over the column offsets k = 0, 1, .. that stops only when k * k > best, so that EQUALLY near
//                        sites are all seen: (d2, label, raster index) is minimised lexicographically, and a column's upper AND
//                        lower site are both taken when they are equally far.  The label image is read only for candidates
//                        with d2 <= best
//   terr_reduce_kernel   the column-run walk of label_reduce.h over key = (nearest label within reach, on the mask): pixels, pixels
//                        on the mask and the frame-border flag of a vertical run in closed form, the largest d2 of a run tracked
//                        beside the walk; LDS slot table, eight-lanes-per-row flush
//   terr_pairs_kernel    the 4-neighbour links between territories (right and down neighbour), equal links of a column run and of
//                        neighbouring lanes added up first, then into a per-frame open-addressing table keyed by (a, b) (64-bit
//                        compare-and-swap, bounded probing, integer atomics); a full table raises the frame's flag.  The table,
//                        its probing rule and the count / scan kernels behind offsets and totals are pair_table.h's
//   pair_write_kernel    (pair_table.h, with TerrEmit) the compacted rows (and the number of distinct partners per ROI and type
//                        slot).  Was terr_pairs_write_kernel
#include <type_traits>

#include "column_pass.h"
#include "label_reduce.h"
#include "pair_table.h"

// (no floating point in here; the pragma keeps any that is added later rounded operation by operation, as surface.hip)
#pragma clang fp contract(off)

namespace pcseg {

// staged vertical distance of a column without site: its square is >= 2^31 > any d2 of a frame (check_shape: H, W <= 32768
// and H W < 2^30 give d2 < 2^31), and adding k * k (k <= 32767 + 3) still fits 32 bits
constexpr unsigned VOR_G_NONE = 46341u;
constexpr unsigned VOR_UP = 1u << 16, VOR_DN = 1u << 17;  // the staged cell: g | VOR_UP (a site g rows up) | VOR_DN (g rows down)
constexpr unsigned VOR_BEST0 = 0x7FFFFFFFu;

struct SiteTest {
    const uint8_t *sel;  // the frame's row of the selection, or null
    int cap;
    __device__ __forceinline__ bool operator()(int l) const { return l >= 1 && l <= cap && (!sel || sel[l - 1] != 0); }
};

// one thread per (word, column): site bits of 32 rows (rows past the frame's end re-read its last row and are masked out)
__global__ void __launch_bounds__(256) vor_bits_kernel(const int *__restrict__ labels, const uint8_t *__restrict__ sel, int cap,
                                                        unsigned *__restrict__ bits, int H, int W, int nch)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int ch = blockIdx.y, b = blockIdx.z;
    if (c >= W) return;
    const int *lab = labels + (int64_t)b * H * W + c;
    const SiteTest site{sel ? sel + (int64_t)b * cap : nullptr, cap};
    const int r0 = ch * COL_ROWS;
    int v[COL_ROWS];
#pragma unroll
    for (int j = 0; j < COL_ROWS; ++j) v[j] = lab[rowoff(min(r0 + j, H - 1), W)];
    unsigned word = 0;
#pragma unroll
    for (int j = 0; j < COL_ROWS; ++j)
        if (site(v[j])) word |= 1u << j;
    word &= col_valid(min(COL_ROWS, H - r0));
    bits[((int64_t)b * nch + ch) * W + c] = word;
}

template <int RB>
__global__ void __launch_bounds__(256) vor_row_kernel(const int *__restrict__ labels, const unsigned *__restrict__ bits,
                                                       const uint16_t *__restrict__ up, const uint16_t *__restrict__ dn,
                                                       const int *__restrict__ any_site, int *__restrict__ d2_out,
                                                       int *__restrict__ near_out, int *__restrict__ site_out, int H, int W, int nch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned cells[];  // [RB][W + 2]: one guard cell either side of a row
    const int P = W + 2;
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * RB;
    const int nrows = min(RB, H - r0);
    const int64_t fbase = (int64_t)b * H * W;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int WPR = RB >= 4 ? 1 : 4 / RB, RSTEP = 4 / WPR;  // waves per row; rows the block's four waves cover at a time
    if (!any_site[b]) {  // a frame without site: d2 = -1, nearest label 0, site -1
        for (int j = wave / WPR; j < nrows; j += RSTEP)
            for (int c = lane + 64 * (wave % WPR); c < W; c += 64 * WPR) {
                const int64_t gi = fbase + rowoff(r0 + j, W) + c;
                d2_out[gi] = -1;
                near_out[gi] = 0;
                if (site_out) site_out[gi] = -1;
            }
        return;
    }
    // the staged cell: distance to the nearest site of the column and on which side(s) it lies
    col_stage_rows<RB>(bits, up, dn, b, r0, H, W, nch, [&](int j, int c, unsigned du, unsigned dd) {
        const unsigned g = min(du, dd);
        cells[j * P + c + 1] = g == COL_NONE ? VOR_G_NONE : g | (du == g ? VOR_UP : 0u) | (dd == g ? VOR_DN : 0u);
    });
    if (threadIdx.x < 2 * RB) cells[(threadIdx.x >> 1) * P + ((threadIdx.x & 1) ? W + 1 : 0)] = VOR_G_NONE;
    __syncthreads();
    const int *lab = labels + fbase;
    for (int j = wave / WPR; j < nrows; j += RSTEP)
        for (int c = lane + 64 * (wave % WPR); c < W; c += 64 * WPR) {
            const int r = r0 + j;
            const unsigned *gr = cells + j * P + 1;  // gr[-1] and gr[W] are the guard cells
            unsigned best = VOR_BEST0;
            int lbl = 0, q = -1;
            // column cc holds its nearest site(s) at squared distance d <= best: the label image decides between equals
            auto take = [&](int cc, unsigned cell, unsigned d) {
                const int g = (int)(cell & 0xFFFFu);
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    if (!(cell & (side ? VOR_DN : VOR_UP))) continue;
                    const int rr = side ? r + g : r - g;
                    if ((unsigned)rr >= (unsigned)H) continue;
                    const int idx = (int)rowoff(rr, W) + cc;
                    const int l = lab[idx];
                    if (d < best || l < lbl || (l == lbl && idx < q)) {  // (d <= best here)
                        best = d;
                        lbl = l;
                        q = idx;
                    }
                }
            };
            auto dist = [](unsigned cell, unsigned kk) { const unsigned g = cell & 0xFFFFu; return __umul24(g, g) + kk; };
            {
                const unsigned cell = gr[c], d = dist(cell, 0u);
                if (d <= best) take(c, cell, d);
            }
            // offsets k .. k + 3 on both sides per trip (eight LDS reads issued together); indices are clamped onto the guard
            // cells, which never qualify.  The exit test is STRICT (k * k > best): a column at k * k == best can still hold an
            // equally near site of a smaller label.  Offsets of a trip beyond that bound cost more than best and fall through
            const int klim = max(c, W - 1 - c);
            for (int k = 1; k <= klim && (unsigned)(k * k) <= best; k += 4) {
                unsigned gl[4], gq[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    gl[t] = gr[max(c - k - t, -1)];
                    gq[t] = gr[min(c + k + t, W)];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const unsigned kk = (unsigned)((k + t) * (k + t));
                    const unsigned dl = dist(gl[t], kk), dq = dist(gq[t], kk);
                    if (dl <= best) take(c - k - t, gl[t], dl);
                    if (dq <= best) take(c + k + t, gq[t], dq);
                }
            }
            const int64_t gi = fbase + rowoff(r, W) + c;
            d2_out[gi] = (int)best;
            near_out[gi] = lbl;
            if (site_out) site_out[gi] = q;
        }
}

// ---- the label of a pixel within reach
__global__ void __launch_bounds__(256) terr_labels_kernel(const int *__restrict__ near, const int *__restrict__ d2, int R2,
                                                           int *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int d = d2[i];
        out[i] = (d >= 0 && d <= R2) ? near[i] : 0;
    }
}

// ---- territory rows
struct TerrRun {
    int key;  // label << 1 | on the mask; 0 = none
    int n, on, clip;
};

struct TerrRaw {
    int4 n, d;
    unsigned m;  // four mask bytes
};
__device__ __forceinline__ void landed(const TerrRaw &q) { landed(q.n); landed(q.d); landed(q.m); }

struct TerrSlots {
    int *tags;
    int (*cnt)[4];  // px, on_px, reach2_max, clipped
    unsigned long long *gout;  // the frame's rows
};

// VEC: W % 4 == 0, near / d2 16-byte and the mask 4-byte aligned
template <bool VEC>
struct TerrWalk {
    using Key = int;
    using Raw = TerrRaw;
    using Run = TerrRun;
    const int *near, *d2;
    const uint8_t *mask;  // may be null
    int c, H, W, R2, cap;
    TerrSlots ls;
    // the largest d2 of each column's open run, tracked beside the walk (a run's maximum has no closed form)
    mutable int open_label[4] = {0, 0, 0, 0}, open_max[4] = {0, 0, 0, 0};

    __device__ __forceinline__ Raw load(int r) const
    {
        Raw q;
        q.n = row_labels4<VEC>(near + rowoff(r, W), c, W);
        q.d = row_labels4<VEC>(d2 + rowoff(r, W), c, W);
        q.m = 0;
        if (mask && c < W) {
            const uint8_t *at = mask + rowoff(r, W) + c;
            if (VEC) {
                q.m = *reinterpret_cast<const unsigned *>(at);
            } else {
                q.m = at[0];
                if (c + 1 < W) q.m |= (unsigned)at[1] << 8;
                if (c + 2 < W) q.m |= (unsigned)at[2] << 16;
                if (c + 3 < W) q.m |= (unsigned)at[3] << 24;
            }
        }
        return q;
    }
    __device__ __forceinline__ void max_commit(int l, int v) const
    {
        if (l <= 0) return;
        const int slot = slot_claim(ls.tags, l);
        if (slot >= 0) atomicMax(&ls.cnt[slot][2], v);
        else atomicMax(&ls.gout[(int64_t)(l - 1) * 4 + 2], (unsigned long long)v);
    }
    __device__ __forceinline__ void keys(const Raw &q, Key k[4]) const
    {
        const int nv[4] = {q.n.x, q.n.y, q.n.z, q.n.w}, dv[4] = {q.d.x, q.d.y, q.d.z, q.d.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // (columns beyond the frame's width load zeros: never a label)
            const int l = (nv[j] >= 1 && nv[j] <= cap && dv[j] >= 0 && dv[j] <= R2) ? nv[j] : 0;
            k[j] = l ? (l << 1) | (int)(((q.m >> (8 * j)) & 255u) != 0) : 0;
            if (l != open_label[j]) {
                max_commit(open_label[j], open_max[j]);
                open_label[j] = l;
                open_max[j] = 0;
            }
            if (l) open_max[j] = max(open_max[j], dv[j]);
        }
    }
    __device__ __forceinline__ void max_flush() const
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) max_commit(open_label[j], open_max[j]);
    }
    __device__ __forceinline__ Run run(Key key, int start, int end, int col) const
    {
        const int n = end - start;
        return Run{key, n, (key & 1) ? n : 0, (int)(start == 0 || end == H || col == 0 || col == W - 1)};
    }
    static __device__ __forceinline__ Run shfl(const Run &a, int off)
    {
        return Run{a.key, __shfl_down(a.n, off), __shfl_down(a.on, off), __shfl_down(a.clip, off)};
    }
    static __device__ __forceinline__ void merge(Run &a, const Run &o) { a.n += o.n; a.on += o.on; a.clip |= o.clip; }
    __device__ __forceinline__ void commit(const Run &a) const
    {
        const int l = a.key >> 1;
        const int slot = slot_claim(ls.tags, l);
        if (slot >= 0) {
            atomicAdd(&ls.cnt[slot][0], a.n);
            if (a.on) atomicAdd(&ls.cnt[slot][1], a.on);
            if (a.clip) atomicOr(&ls.cnt[slot][3], 1);
        } else {
            unsigned long long *t = ls.gout + (int64_t)(l - 1) * 4;
            atomicAdd(&t[0], (unsigned long long)a.n);
            if (a.on) atomicAdd(&t[1], (unsigned long long)a.on);
            if (a.clip) atomicOr(&t[3], 1ull);
        }
    }
};

template <bool VEC>
__global__ void __launch_bounds__(256) terr_reduce_kernel(const int *__restrict__ near, const int *__restrict__ d2,
                                                           const uint8_t *__restrict__ mask, int R2, int cap, int H, int W,
                                                           unsigned long long *__restrict__ out)
{
    __shared__ int tags[LABEL_SLOTS];
    __shared__ int cnt[LABEL_SLOTS][4];
    const TileIndex ti = xcd_tile_index();  // (a frame's blocks on one XCD: their atomics on the frame's table meet in one L2)
    const int b = ti.z;
    unsigned long long *gout = out + (int64_t)b * cap * 4;
    for (int i = threadIdx.x; i < LABEL_SLOTS; i += 256) {
        tags[i] = 0;
        cnt[i][0] = 0; cnt[i][1] = 0; cnt[i][2] = 0; cnt[i][3] = 0;
    }
    __syncthreads();
    const int c = (ti.x * 256 + threadIdx.x) * 4;
    const int r0 = ti.y * RUN_ROWS;
    const int64_t fbase = (int64_t)b * H * W;
    const TerrWalk<VEC> walk{near + fbase, d2 + fbase, mask ? mask + fbase : nullptr, c, H, W, R2, cap, TerrSlots{tags, cnt, gout}};
    column_run_walk(walk, c, r0, min(H, r0 + RUN_ROWS));
    walk.max_flush();
    __syncthreads();
    slots_flush8(tags, [&](int i, int l, int f) {
        if (f >= 4) return;
        const int v = cnt[i][f];
        if (!v) return;
        unsigned long long *t = gout + (int64_t)(l - 1) * 4 + f;
        if (f < 2) atomicAdd(t, (unsigned long long)v);
        else if (f == 2) atomicMax(t, (unsigned long long)v);
        else atomicOr(t, 1ull);
    });
}

// ---- adjacency: the per-frame pair table (pair_table.h) with two counters per pair: border, contact
constexpr int TERR_NV = 2;

struct PairAcc {
    unsigned long long key;  // 0 = none
    unsigned n, ct;
};

// a lane owns one column and walks down RUN_ROWS rows: the links to the right and to the lower neighbour.  Equal links that
// follow each other in the column add up in registers (a border that runs down the frame), and at the end of the block
// neighbouring lanes with the same open pair are summed by the segmented reduction (a border that runs across it)
__global__ void __launch_bounds__(256) terr_pairs_kernel(const int *__restrict__ near, const int *__restrict__ d2, int R2, int H,
                                                          int W, unsigned long long *__restrict__ keys, unsigned *__restrict__ cnt,
                                                          int *__restrict__ overflow, int pair_cap)
{
    const TileIndex ti = xcd_tile_index();
    const int b = ti.z;
    const PairTable<TERR_NV> tab = pair_table_of<TERR_NV>(keys, cnt, overflow, pair_cap, b);
    const int c = ti.x * 256 + threadIdx.x;
    const int r0 = ti.y * RUN_ROWS, r1 = min(H, r0 + RUN_ROWS);
    const int *fn = near + (int64_t)b * H * W, *fd = d2 + (int64_t)b * H * W;
    const bool in = c < W, right = c + 1 < W;  // (every lane stays for the reductions: a lane past the width walks nothing)
    PairAcc accR{0, 0, 0}, accD{0, 0, 0};
    auto own = [R2](int n, int d) { return (n >= 1 && d >= 0 && d <= R2) ? n : 0; };
    auto feed = [&](PairAcc &a, int la, int da, int lb, int db) {
        if (la > 0 && lb > 0 && la != lb) {
            const unsigned long long key = ((unsigned long long)(unsigned)min(la, lb) << 32) | (unsigned)max(la, lb);
            if (key != a.key) {
                if (a.key) pair_add(tab, a.key, {a.n, a.ct});
                a = PairAcc{key, 0, 0};
            }
            ++a.n;
            a.ct += (da == 0 && db == 0);
        }
    };
    int n0 = 0, d0 = -1;
    if (in) {
        n0 = fn[rowoff(r0, W) + c];
        d0 = fd[rowoff(r0, W) + c];
    }
    for (int r = r0; r < r1; ++r) {
        int nr = 0, dr = -1, nd = 0, dd = -1;
        if (right) {
            nr = fn[rowoff(r, W) + c + 1];
            dr = fd[rowoff(r, W) + c + 1];
        }
        if (in && r + 1 < H) {
            nd = fn[rowoff(r + 1, W) + c];
            dd = fd[rowoff(r + 1, W) + c];
        }
        const int a = own(n0, d0);
        feed(accR, a, d0, own(nr, dr), dr);
        feed(accD, a, d0, own(nd, dd), dd);
        n0 = nd;
        d0 = dd;
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const PairAcc a = pass ? accD : accR;
        const WaveSeg seg = wave_segment(a.key);
        uint2 v = make_uint2(a.n, a.ct);
        segment_reduce(
            v, seg.remain, [](const uint2 &x, int off) { return make_uint2(__shfl_down(x.x, off), __shfl_down(x.y, off)); },
            [](uint2 &x, const uint2 &o) { x.x += o.x; x.y += o.y; });
        if (seg.head && a.key) pair_add(tab, a.key, {v.x, v.y});
    }
}

// a used slot as the row (key, frame position, (border, contact)) of pair_table.h's writer; with `degree` also
// degree (B, cap, 2 K) += 1 at [a][slot of b] and [b][slot of a], and at K + slot where the pair has contact
struct TerrEmit {
    static constexpr int NV = TERR_NV;
    const uint8_t *slot_of;
    int cap, K;
    long long *key_out;
    int *frame_out, *cnt_out, *degree;
    __device__ __forceinline__ void operator()(int b, unsigned long long key, const unsigned *c, long long row) const
    {
        const unsigned border = c[0], contact = c[1];
        key_out[row] = (long long)key;
        frame_out[row] = b;
        cnt_out[2 * row] = (int)border;
        cnt_out[2 * row + 1] = (int)contact;
        const unsigned la = (unsigned)(key >> 32), lb = (unsigned)key;
        // (& not &&: one test and one branch per slot; with && the writer's loop took a second one)
        if ((degree != nullptr) & (la >= 1) & (lb >= 1) & (la <= (unsigned)cap) & (lb <= (unsigned)cap)) {
            const int sa = slot_of[(int64_t)b * cap + la - 1], sb = slot_of[(int64_t)b * cap + lb - 1];
            int *da = degree + ((int64_t)b * cap + la - 1) * 2 * K, *db = degree + ((int64_t)b * cap + lb - 1) * 2 * K;
            if (sb < K) {
                atomicAdd(&da[sb], 1);
                if (contact) atomicAdd(&da[K + sb], 1);
            }
            if (sa < K) {
                atomicAdd(&db[sa], 1);
                if (contact) atomicAdd(&db[K + sa], 1);
            }
        }
    }
};

static inline int reach_arg(int64_t R2) { return (R2 < 0 || R2 > 0x7FFFFFFF) ? 0x7FFFFFFF : (int)R2; }

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_nearest_label_workspace_bytes(int B, int H, int W)
{
    if (!check_shape(B, H, W)) return 0;
    return carved_bytes(col_carve, B, H, W);
}

int pcseg_nearest_label_i32(const int32_t *labels, const uint8_t *sel, int cap, int32_t *d2, int32_t *near, int32_t *site, int B,
                            int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels && d2 && near && workspace && check_shape(B, H, W) && cap >= 1 && B <= 65535, "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const ColWs ws = col_carve(cv, B, H, W);
    if (!cv.fits("nearest_label_i32")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    PCSEG_CHECK_HIP(hipMemsetAsync(ws.any, 0, sizeof(int) * B, s));
    PCSEG_LAUNCH(vor_bits_kernel, dim3((W + 255) / 256, ws.nch, B), dim3(256), 0, s, labels, sel, cap, ws.bits, H, W, ws.nch);
    PCSEG_CHECK_LAUNCH();
    if (const int rc = col_carry_launch(ws, B, H, W, s)) return rc;
    // rows per block: four while a block's stage stays within 64 KB (W <= 4094: two and more blocks per CU; the occupancy
    // argument of the distance transform's row pass), else one (W = 32768: 128 KB, one block per CU)
    const size_t per_row = (size_t)(W + 2) * sizeof(unsigned);
    auto launch_rows = [&](auto rb_tag) -> int {
        constexpr int RB = decltype(rb_tag)::value;
        const size_t bytes = RB * per_row;
        if (bytes > 64 * 1024)
            PCSEG_CHECK_HIP(hipFuncSetAttribute((const void *)vor_row_kernel<RB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        PCSEG_LAUNCH((vor_row_kernel<RB>), dim3((H + RB - 1) / RB, B), dim3(256), bytes, s, labels, (const unsigned *)ws.bits,
                     (const uint16_t *)ws.up, (const uint16_t *)ws.dn, (const int *)ws.any, d2, near, site, H, W, ws.nch);
        return PCSEG_OK;
    };
    int rc;
    if (4 * per_row <= 64 * 1024) rc = launch_rows(std::integral_constant<int, 4>());
    else rc = launch_rows(std::integral_constant<int, 1>());
    if (rc) return rc;
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_territory_labels(const int32_t *near, const int32_t *d2, int64_t R2, int32_t *out, int64_t n, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(near && d2 && out && n >= 1 && n < ((int64_t)1 << 39), "bad arguments");
    PCSEG_LAUNCH(terr_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, near, d2, reach_arg(R2), out, n);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_territory_reduce(const int32_t *near, const int32_t *d2, const uint8_t *mask, int64_t R2, int cap, int64_t *out, int B,
                           int H, int W, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(near && d2 && out && check_shape(B, H, W) && cap >= 1 && cap < (1 << 30) && B <= 65535, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    PCSEG_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(int64_t) * 4 * (size_t)B * cap, s));
    const dim3 grid((W + 1023) / 1024, (H + RUN_ROWS - 1) / RUN_ROWS, B);
    const bool vec = W % 4 == 0 && (((uintptr_t)near | (uintptr_t)d2) & 15) == 0 && ((uintptr_t)mask & 3) == 0;
    if (vec)
        PCSEG_LAUNCH(terr_reduce_kernel<true>, grid, dim3(256), 0, s, near, d2, mask, reach_arg(R2), cap, H, W, (unsigned long long *)out);
    else
        PCSEG_LAUNCH(terr_reduce_kernel<false>, grid, dim3(256), 0, s, near, d2, mask, reach_arg(R2), cap, H, W, (unsigned long long *)out);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

size_t pcseg_territory_pairs_workspace_bytes(int B, int pair_cap)
{
    if (B < 1 || pair_cap < 1) return 0;
    return carved_bytes(pairs_carve<TERR_NV>, B, pair_cap, 0);
}

int pcseg_territory_pairs(const int32_t *near, const int32_t *d2, int64_t R2, int pair_cap, int32_t *overflow, int64_t *offsets,
                          int64_t *totals, int B, int H, int W, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(near && d2 && overflow && offsets && totals && workspace && check_shape(B, H, W) && pair_cap >= 1 && B <= 65535,
                  "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const PairWs<TERR_NV> ws = pairs_carve<TERR_NV>(cv, B, pair_cap, 0);
    if (!cv.fits("territory_pairs")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = pairs_begin(ws, overflow, B, pair_cap, s)) return rc;
    PCSEG_LAUNCH(terr_pairs_kernel, dim3((W + 255) / 256, (H + RUN_ROWS - 1) / RUN_ROWS, B), dim3(256), 0, s, near, d2, reach_arg(R2), H,
                 W, ws.keys, ws.cnt, overflow, pair_cap);
    PCSEG_CHECK_LAUNCH();
    return pairs_finish(ws, overflow, offsets, totals, B, pair_cap, s);
}

int pcseg_territory_pairs_write(int pair_cap, const int64_t *offsets, const uint8_t *slot_of, int cap, int n_types, int64_t *key,
                                int32_t *frame, int32_t *counts, int32_t *degree, int B, const void *workspace,
                                size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(offsets && key && frame && counts && workspace && B >= 1 && B <= 65535 && pair_cap >= 1, "bad arguments");
    PCSEG_REQUIRE(!degree || (slot_of && cap >= 1 && n_types >= 1 && n_types <= 4), "degree needs slot_of, cap and 1..4 type slots");
    return pairs_write("territory_pairs_write", workspace, workspace_bytes, B, pair_cap, 0, offsets,
                       TerrEmit{slot_of, cap, n_types, (long long *)key, frame, counts, degree}, stream);
}

}  // extern "C"
