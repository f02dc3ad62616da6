// Per-ROI skeletons: exact Guo-Hall thinning of an int32 label image (skimage.morphology.thin of scikit-image 0.18.3, every
// label on its own), the peel image, and per ROI the links, ends and junctions of its skeleton (include/pcseg.h).  A straight
// line with two ends is one rod, a junction a clump, a loop a ring of cells around a hole; area / length is the width.
// Integers only: a sub-iteration reads the old state and writes the new one, so the result does not depend on any order.
//
// State (the iteration never reads the 4-byte labels again):
//   link   one byte per pixel, bit i: neighbour i (E NE N NW W SW S SE) lies in the frame and carries the centre's label
//   alive  one bit per pixel in 32-bit row words, TWO copies: a launch reads one and writes the other (a tile's halo is its
//          neighbours' pixels, which other blocks of the same launch rewrite)
// Launches of pcseg_thin_labels:
//   thin_rule_kernel    the two 256-entry deletion tables from the predicates, as 2 x 8 words of 32 bits
//   thin_init_kernel    labels -> link bytes, both copies of the alive bits, peel = 65535 / 0, tiles with a pixel flagged
//   thin_list_kernel    flagged tiles -> the list of the next launch (flags cleared)
//   thin_tile_kernel    one block per listed tile: the 64 x 32 tile with a halo of SK_K pixels in LDS runs up to SK_K
//                       sub-iterations there -- what is known exactly shrinks by one pixel per sub-iteration and ends at
//                       the tile --, writes peel for the tile's pixels it deleted, the tile's alive words into the other
//                       copy, and flags itself and its 8 neighbours if it deleted a pixel
//   thin_iters_kernel   iters[b] from the last sub-iteration that deleted a pixel of the frame
// A tile that deleted nothing and whose 8 neighbours deleted nothing in a launch sees the same tile and halo at the start of
// the next one; SK_K is EVEN, so that launch starts with the same table and would repeat the same steps: the tile is left
// out until a neighbour deletes again.  (Both copies of its alive words agree at that point: it wrote the second one from
// an unchanged first.)  The host reads two counters per launch (pixels deleted, tiles listed) and stops when nothing was
// deleted.
// pcseg_region_skeleton: a 64 x 32 tile of labels and peel values with a 1-pixel halo in LDS; a lane walks 8 rows of one
// column, same-label neighbouring lanes are summed by the segmented wave reduction of label_reduce.h, then its slot table in
// LDS and integer atomics on the rows of the table.  (The column-run walk itself does not apply: a skeleton pixel's links
// depend on its 3 x 3 neighbourhood, not on the length of a vertical run.)
#include <algorithm>

#include "label_reduce.h"

// the two operations of length_px rounded on their own (no FMA)
#pragma clang fp contract(off)

namespace pcseg {

constexpr int SK_TW = 64, SK_TH = 32;  // pixels of a tile: two alive words per row, one wave per row
constexpr int SK_K = 8;                // halo of a tile = sub-iterations per launch
constexpr int SK_LW = SK_TW + 2 * SK_K, SK_LH = SK_TH + 2 * SK_K;
constexpr int SK_PER = (SK_LW * SK_LH + 255) / 256;  // pixels of the LDS region per thread
constexpr int SK_SKELETON = 65535, SK_MAX_SUB = 65534;
static_assert(SK_K % 2 == 0, "every launch starts with the first table");
static_assert(SK_K <= SK_TW && SK_K <= SK_TH, "a tile's halo lies inside its 8 neighbours");
static_assert(SK_TW == WAVE && SK_PER <= 32, "one wave per tile row; a thread's deletions of a sub-iteration are one 32-bit mask");

// N = sum 2^i b[i], b[0..7] = E NE N NW W SW S SE: is a pixel with this neighbour code deleted by the first (second = 0) or
// the second sub-iteration
__host__ __device__ inline bool thin_rule(int code, int second)
{
    int b[8];
    for (int i = 0; i < 8; ++i) b[i] = (code >> i) & 1;
    int g1 = 0, n1 = 0, n2 = 0;
    for (int i = 0; i < 8; i += 2) g1 += !b[i] && (b[(i + 1) & 7] || b[(i + 2) & 7]);
    for (int k = 1; k < 8; k += 2) {
        n1 += b[k] || b[k - 1];
        n2 += b[k] || b[(k + 1) & 7];
    }
    const int m = n1 < n2 ? n1 : n2;
    const bool g3 = second ? !((b[5] || b[6] || !b[3]) && b[4]) : !((b[1] || b[2] || !b[7]) && b[0]);
    return g1 == 1 && (m == 2 || m == 3) && g3;
}

struct SkWorkspace {
    uint32_t *bits[2];  // [B, H, wpr] alive
    uint8_t *link;      // [B, H, W]
    int *flags;         // [B * tiles] tile runs in the next launch
    int *list;          // [B * tiles]
    uint32_t *rule;     // [2][8]
    int *last;          // [B] last sub-iteration that deleted a pixel of the frame
    int *ctr;           // pixels deleted, tiles listed
};

static int sk_wpr(int W) { return (W + 31) / 32; }
static int sk_tx(int W) { return (W + SK_TW - 1) / SK_TW; }
static int sk_ty(int H) { return (H + SK_TH - 1) / SK_TH; }

// the ONE layout of the workspace
static SkWorkspace thin_carve(Carver &cv, int B, int H, int W)
{
    SkWorkspace w;
    const size_t tiles = (size_t)B * sk_tx(W) * sk_ty(H);
    w.bits[0] = cv.take<uint32_t>((size_t)B * H * sk_wpr(W));
    w.bits[1] = cv.take<uint32_t>((size_t)B * H * sk_wpr(W));
    w.link = cv.take<uint8_t>((size_t)B * H * W);
    w.flags = cv.take<int>(tiles);
    w.list = cv.take<int>(tiles);
    w.rule = cv.take<uint32_t>(16);
    w.last = cv.take<int>((size_t)B);
    w.ctr = cv.take<int>(2);
    return w;
}

// (pcseg_region_skeleton keeps nothing in its workspace: the size conventions of the other entries)
static void skeleton_carve(Carver &cv) { cv.take<char>(1); }

__global__ void __launch_bounds__(256) thin_rule_kernel(uint32_t *__restrict__ rule)
{
    const int code = threadIdx.x;
#pragma unroll
    for (int second = 0; second < 2; ++second) {
        const unsigned long long m = __ballot(thin_rule(code, second));
        if ((threadIdx.x & 31) == 0) rule[second * 8 + (code >> 5)] = (uint32_t)(m >> (threadIdx.x & 32));
    }
}

// block (64, 4): a wave per row, 64 columns from a multiple of 64
__global__ void __launch_bounds__(256) thin_init_kernel(const int *__restrict__ labels, uint8_t *__restrict__ link,
                                                         uint32_t *__restrict__ bits0, uint32_t *__restrict__ bits1,
                                                         uint16_t *__restrict__ peel, int *__restrict__ flags, int H, int W, int wpr,
                                                         int tx, int ty)
{
    const int b = blockIdx.z, r = blockIdx.y * 4 + threadIdx.y, c = blockIdx.x * WAVE + threadIdx.x;
    if (r >= H) return;  // (the whole wave)
    const int *g = labels + (int64_t)b * H * W;
    const bool in = c < W;
    const int l = in ? g[rowoff(r, W) + c] : 0;
    unsigned m = 0;
    if (l > 0) {
        const int dr[8] = {0, -1, -1, -1, 0, 1, 1, 1}, dc[8] = {1, 1, 0, -1, -1, -1, 0, 1};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int rr = r + dr[i], cc = c + dc[i];
            if (rr >= 0 && rr < H && cc >= 0 && cc < W && g[rowoff(rr, W) + cc] == l) m |= 1u << i;
        }
    }
    if (in) {
        const int64_t at = (int64_t)b * H * W + rowoff(r, W) + c;
        link[at] = (uint8_t)m;
        peel[at] = l > 0 ? SK_SKELETON : 0;
    }
    const unsigned long long alive = __ballot(l > 0);
    const int word = blockIdx.x * 2 + (threadIdx.x >> 5);
    if ((threadIdx.x & 31) == 0 && word < wpr) {
        const int64_t at = ((int64_t)b * H + r) * wpr + word;
        bits0[at] = bits1[at] = (uint32_t)(alive >> (threadIdx.x & 32));
    }
    if (threadIdx.x == 0 && alive) flags[((int64_t)b * ty + r / SK_TH) * tx + blockIdx.x] = 1;
}

__global__ void __launch_bounds__(256) thin_list_kernel(int *__restrict__ flags, int *__restrict__ list, int *__restrict__ ctr, int total)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total || !flags[i]) return;
    flags[i] = 0;
    list[atomicAdd(&ctr[1], 1)] = i;  // (any order: a launch's result does not depend on it)
}

__global__ void __launch_bounds__(256) thin_tile_kernel(const uint8_t *__restrict__ link, const uint32_t *__restrict__ src,
                                                         uint32_t *__restrict__ dst, uint16_t *__restrict__ peel,
                                                         const int *__restrict__ list, const uint32_t *__restrict__ rule,
                                                         int *__restrict__ flags, int *__restrict__ ctr, int *__restrict__ last, int H,
                                                         int W, int wpr, int tx, int ty, int sub0, int nsub)
{
    __shared__ uint8_t al[SK_LH * SK_LW], lk[SK_LH * SK_LW];
    __shared__ uint32_t tab[16];
    __shared__ int ndel, slast;
    const int tid = threadIdx.x;
    const int t = list[blockIdx.x];
    const int b = t / (tx * ty), ti = t - b * (tx * ty), tyi = ti / tx, txi = ti - tyi * tx;
    const int R0 = tyi * SK_TH - SK_K, C0 = txi * SK_TW - SK_K;
    const int64_t fbits = (int64_t)b * H * wpr, fpix = (int64_t)b * H * W;
    if (tid < 16) tab[tid] = rule[tid];
    if (tid == 0) {
        ndel = 0;
        slast = 0;
    }
#pragma unroll
    for (int j = 0; j < SK_PER; ++j) {
        const int idx = tid + 256 * j;
        if (idx >= SK_LH * SK_LW) break;
        const int rr = idx / SK_LW, r = R0 + rr, c = C0 + idx - rr * SK_LW;
        unsigned a = 0, k = 0;
        if (r >= 0 && r < H && c >= 0 && c < W) {
            a = (src[fbits + rowoff(r, wpr) + (c >> 5)] >> (c & 31)) & 1u;
            if (a) k = link[fpix + rowoff(r, W) + c];
        }
        al[idx] = (uint8_t)a;
        lk[idx] = (uint8_t)k;
    }
    __syncthreads();
    int mydel = 0, mylast = 0;
    for (int s = 1; s <= nsub; ++s) {
        const int second = (s & 1) ^ 1;  // (sub0 is even)
        unsigned del = 0;
#pragma unroll
        for (int j = 0; j < SK_PER; ++j) {
            const int idx = tid + 256 * j;
            if (idx >= SK_LH * SK_LW) break;
            const int rr = idx / SK_LW, cc = idx - rr * SK_LW;
            // exact after s sub-iterations: the pixels s or more from the region's rim (their neighbours are in the region)
            if (rr < s || rr >= SK_LH - s || cc < s || cc >= SK_LW - s || !al[idx]) continue;
            unsigned code = al[idx + 1] | (al[idx - SK_LW + 1] << 1) | (al[idx - SK_LW] << 2) | (al[idx - SK_LW - 1] << 3)
                            | (al[idx - 1] << 4) | (al[idx + SK_LW - 1] << 5) | (al[idx + SK_LW] << 6) | (al[idx + SK_LW + 1] << 7);
            code &= lk[idx];
            if ((tab[second * 8 + (code >> 5)] >> (code & 31)) & 1u) del |= 1u << j;
        }
        __syncthreads();
        for (unsigned m = del; m; m &= m - 1) {
            const int idx = tid + 256 * (__ffs((int)m) - 1);
            al[idx] = 0;
            const int rr = idx / SK_LW, cc = idx - rr * SK_LW;
            if (rr >= SK_K && rr < SK_K + SK_TH && cc >= SK_K && cc < SK_K + SK_TW) {  // the tile's own (alive: inside the frame)
                peel[fpix + rowoff(R0 + rr, W) + C0 + cc] = (uint16_t)(sub0 + s);
                ++mydel;
                mylast = s;
            }
        }
        __syncthreads();
    }
    if (mydel) {
        atomicAdd(&ndel, mydel);
        atomicMax(&slast, mylast);
    }
    // the tile's alive words into the other copy
    const int lane = lane_id();
    for (int row = tid >> 6; row < SK_TH; row += 4) {
        const unsigned long long m = __ballot(al[(SK_K + row) * SK_LW + SK_K + lane] != 0);
        const int r = tyi * SK_TH + row, word = txi * 2 + (lane >> 5);
        if ((lane & 31) == 0 && r < H && word < wpr) dst[fbits + rowoff(r, wpr) + word] = (uint32_t)(m >> (lane & 32));
    }
    __syncthreads();
    if (tid == 0 && ndel > 0) {
        atomicAdd(&ctr[0], ndel);
        atomicMax(&last[b], sub0 + slast);
        for (int y = max(tyi - 1, 0); y <= min(tyi + 1, ty - 1); ++y)
            for (int x = max(txi - 1, 0); x <= min(txi + 1, tx - 1); ++x) flags[((int64_t)b * ty + y) * tx + x] = 1;
    }
}

__global__ void __launch_bounds__(256) thin_iters_kernel(const int *__restrict__ last, int *__restrict__ iters, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) iters[b] = (last[b] + 1) >> 1;
}

// ---- the table
constexpr int SR_LW = SK_TW + 2, SR_LH = SK_TH + 2;  // the tile and a 1-pixel ring

__global__ void __launch_bounds__(256) skeleton_init_kernel(long long *__restrict__ out, const int *__restrict__ counts, int cap)
{
    const int b = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < min(max(counts[b], 0), cap) * 6) out[(int64_t)b * cap * 6 + idx] = 0;
}

struct SkSlots {
    int *tags;
    int (*cnt)[8];
};

// v.x = skel_px | n_orth << 16, v.y = n_diag | n_end << 16, v.z = n_junction, v.w = passes (a wave adds at most 1024 to a field)
__device__ __forceinline__ void skeleton_commit(const SkSlots &ls, long long *gout, int nl, int l, const uint4 &v)
{
    if (l > nl) return;
    const unsigned f[5] = {v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16, v.z};
    const int slot = slot_claim(ls.tags, l);
    if (slot >= 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (f[k]) atomicAdd(&ls.cnt[slot][k], (int)f[k]);
        if (v.w) atomicMax(&ls.cnt[slot][5], (int)v.w);
    } else {
        long long *t = gout + (int64_t)(l - 1) * 6;
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (f[k]) atomicAdd((unsigned long long *)&t[k], (unsigned long long)f[k]);
        if (v.w) atomicMax((unsigned long long *)&t[5], (unsigned long long)v.w);
    }
}

__global__ void __launch_bounds__(256) skeleton_table_kernel(const int *__restrict__ labels, const uint16_t *__restrict__ peel,
                                                              const int *__restrict__ counts, int H, int W, int cap,
                                                              long long *__restrict__ out)
{
    __shared__ int key[SR_LH][SR_LW];          // the label of a skeleton pixel, 0 elsewhere
    __shared__ unsigned short pas[SK_TH][SK_TW];  // the full iteration that deleted a pixel, 0 elsewhere
    __shared__ int tags[LABEL_SLOTS];
    __shared__ int cnt[LABEL_SLOTS][8];
    const TileIndex ti = xcd_tile_index();
    const int b = ti.z;
    const int nl = min(max(counts[b], 0), cap);
    const int *g = labels + (int64_t)b * H * W;
    const uint16_t *pl = peel + (int64_t)b * H * W;
    long long *gout = out + (int64_t)b * cap * 6;
    const int R0 = ti.y * SK_TH, C0 = ti.x * SK_TW;
    for (int i = threadIdx.x; i < LABEL_SLOTS; i += 256) {
        tags[i] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) cnt[i][k] = 0;
    }
    for (int idx = threadIdx.x; idx < SR_LH * SR_LW; idx += 256) {
        const int rr = idx / SR_LW, cc = idx - rr * SR_LW;
        const int r = R0 - 1 + rr, c = C0 - 1 + cc;
        int k = 0;
        unsigned p = 0;
        if (r >= 0 && r < H && c >= 0 && c < W) {
            const int l = g[rowoff(r, W) + c];
            if (l > 0) {
                p = pl[rowoff(r, W) + c];
                if (p == SK_SKELETON) k = l;
            }
        }
        key[rr][cc] = k;
        if (rr >= 1 && rr <= SK_TH && cc >= 1 && cc <= SK_TW) pas[rr - 1][cc - 1] = (unsigned short)(p == SK_SKELETON ? 0 : (p + 1) >> 1);
    }
    __syncthreads();
    const SkSlots ls{tags, cnt};
    // wave w walks rows 8 w .. 8 w + 7 of the tile, a lane one column
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    int cur = 0;
    uint4 acc = make_uint4(0, 0, 0, 0);
    for (int i = 0; i < 8; ++i) {
        const int rr = wv * 8 + i;
        const int r = R0 + rr, c = C0 + lane;
        if (r >= H || c >= W) continue;
        const int l = g[rowoff(r, W) + c];
        if (l <= 0) continue;
        if (l != cur) {
            if (cur > 0 && (acc.x | acc.y | acc.z | acc.w)) skeleton_commit(ls, gout, nl, cur, acc);
            cur = l;
            acc = make_uint4(0, 0, 0, 0);
        }
        const int k = key[rr + 1][lane + 1];
        if (k == 0) {
            acc.w = max(acc.w, (unsigned)pas[rr][lane]);
            continue;
        }
        auto on = [&](int dr, int dc) { return (unsigned)(key[rr + 1 + dr][lane + 1 + dc] == k); };
        const unsigned e = on(0, 1), n = on(-1, 0), w = on(0, -1), s = on(1, 0);
        // a diagonal pair is a link only if neither pixel next to both is a skeleton pixel of the label
        const unsigned ne = on(-1, 1) & ~(n | e) & 1u, nw = on(-1, -1) & ~(n | w) & 1u, sw = on(1, -1) & ~(s | w) & 1u,
                       se = on(1, 1) & ~(s | e) & 1u;
        const unsigned deg = e + n + w + s + ne + nw + sw + se;
        // every link is counted at its upper (or left) pixel
        acc.x += 1u | ((e + s) << 16);
        acc.y += (se + sw) | ((unsigned)(deg == 1) << 16);
        acc.z += deg >= 3;
    }
    if (!(acc.x | acc.y | acc.z | acc.w)) cur = 0;
    // lanes next to each other with the same label are summed into the first of them
    const WaveSeg seg = wave_segment(cur);
    segment_reduce(
        acc, seg.remain,
        [](const uint4 &a, int off) { return make_uint4(__shfl_down(a.x, off), __shfl_down(a.y, off), __shfl_down(a.z, off), __shfl_down(a.w, off)); },
        [](uint4 &a, const uint4 &o) { a.x += o.x; a.y += o.y; a.z += o.z; a.w = max(a.w, o.w); });
    if (seg.head && cur > 0) skeleton_commit(ls, gout, nl, cur, acc);
    __syncthreads();
    slots_flush8(tags, [&](int i, int l, int f) {
        const int v = cnt[i][f];
        if (f >= 6 || v == 0) return;
        long long *t = gout + (int64_t)(l - 1) * 6 + f;
        if (f < 5) atomicAdd((unsigned long long *)t, (unsigned long long)v);
        else atomicMax((unsigned long long *)t, (unsigned long long)v);
    });
}

__global__ void __launch_bounds__(256) skeleton_properties_kernel(const long long *__restrict__ stats, const long long *__restrict__ table,
                                                                   const int *__restrict__ counts, double *__restrict__ out, int cap)
{
    const int b = blockIdx.y;
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= min(counts[b], cap)) return;
    const int64_t row = (int64_t)b * cap + l;
    const long long A = stats[row * 8];
    const long long *sk = table + row * 6;
    double *o = out + row * 2;
    if (A <= 0) {  // a label without a pixel has no skeleton
        o[0] = o[1] = __builtin_nan("");
        return;
    }
    // (written out under this file's contract(off): the header's __dmul_rn / __dadd_rn are inline functions compiled under the
    // default contraction mode, and once inlined their product and sum were fused -- one ulp off numpy's value)
    const double diag = (double)sk[2] * 1.4142135623730951;
    const double len = (double)sk[1] + diag;
    o[0] = len;
    o[1] = (double)A / len;
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

size_t pcseg_thin_labels_workspace_bytes(int B, int H, int W)
{
    if (!check_shape(B, H, W)) return 0;
    return carved_bytes(thin_carve, B, H, W);
}

int pcseg_thin_labels(const int32_t *labels, uint16_t *peel, int32_t *iters, int B, int H, int W, int max_iter, void *workspace,
                      size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels && peel && iters && workspace && check_shape(B, H, W) && B <= 65535, "bad arguments");
    Carver cv(workspace, workspace_bytes);
    const SkWorkspace w = thin_carve(cv, B, H, W);
    if (!cv.fits("thin_labels")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int wpr = sk_wpr(W), tx = sk_tx(W), ty = sk_ty(H);
    const int64_t total64 = (int64_t)B * tx * ty;
    PCSEG_REQUIRE(total64 < ((int64_t)1 << 31), "bad arguments");
    const int total = (int)total64;
    // no shape needs more than min(H, W) / 2 + 1 full iterations: H + W of them (and the launch that would confirm the end)
    // without an end is an error, never a loop
    const int64_t bound = std::min<int64_t>(2 * ((int64_t)H + W), SK_MAX_SUB - SK_K) + SK_K;
    const int64_t budget = max_iter < 0 || 2 * (int64_t)max_iter > bound - SK_K ? bound : 2 * (int64_t)max_iter;
    PCSEG_CHECK_HIP(hipMemsetAsync(w.flags, 0, (size_t)total * sizeof(int), s));
    PCSEG_CHECK_HIP(hipMemsetAsync(w.last, 0, (size_t)B * sizeof(int), s));
    PCSEG_CHECK_HIP(hipMemsetAsync(w.ctr, 0, 2 * sizeof(int), s));
    PCSEG_LAUNCH(thin_rule_kernel, dim3(1), dim3(256), 0, s, w.rule);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(thin_init_kernel, dim3(tx, (H + 3) / 4, B), dim3(WAVE, 4), 0, s, labels, w.link, w.bits[0], w.bits[1], peel, w.flags, H, W,
                 wpr, tx, ty);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(thin_list_kernel, dim3((total + 255) / 256), dim3(256), 0, s, w.flags, w.list, w.ctr, total);
    PCSEG_CHECK_LAUNCH();
    int host[2] = {0, 0};
    PCSEG_CHECK_HIP(hipMemcpyAsync(host, w.ctr, sizeof(host), hipMemcpyDeviceToHost, s));
    PCSEG_CHECK_HIP(hipStreamSynchronize(s));
    int sub0 = 0, cur = 0;
    bool deleting = host[1] > 0;
    while (deleting && sub0 < budget) {
        const int n = host[1];
        const int nsub = (int)std::min<int64_t>(SK_K, budget - sub0);
        PCSEG_CHECK_HIP(hipMemsetAsync(w.ctr, 0, 2 * sizeof(int), s));
        PCSEG_LAUNCH(thin_tile_kernel, dim3(n), dim3(256), 0, s, (const uint8_t *)w.link, (const uint32_t *)w.bits[cur], w.bits[cur ^ 1], peel,
                     (const int *)w.list, (const uint32_t *)w.rule, w.flags, w.ctr, w.last, H, W, wpr, tx, ty, sub0, nsub);
        PCSEG_CHECK_LAUNCH();
        PCSEG_LAUNCH(thin_list_kernel, dim3((total + 255) / 256), dim3(256), 0, s, w.flags, w.list, w.ctr, total);
        PCSEG_CHECK_LAUNCH();
        PCSEG_CHECK_HIP(hipMemcpyAsync(host, w.ctr, sizeof(host), hipMemcpyDeviceToHost, s));
        PCSEG_CHECK_HIP(hipStreamSynchronize(s));
        sub0 += nsub;
        cur ^= 1;
        deleting = host[0] > 0;
    }
    if (deleting && sub0 >= bound) {
        set_error("thin_labels: thinning did not converge after %d sub-iterations", sub0);
        return PCSEG_ERR_CONVERGENCE;
    }
    PCSEG_LAUNCH(thin_iters_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (const int *)w.last, iters, B);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

size_t pcseg_region_skeleton_workspace_bytes(int B, int H, int W, int cap)
{
    if (!check_shape(B, H, W) || cap < 1) return 0;
    return carved_bytes(skeleton_carve);
}

int pcseg_region_skeleton(const int32_t *labels, const uint16_t *peel, const int32_t *counts, int64_t *table, int B, int H, int W,
                          int cap, void *workspace, size_t workspace_bytes, pcseg_stream_t stream)
{
    PCSEG_REQUIRE(labels && peel && counts && table && workspace && check_shape(B, H, W) && cap >= 1 && B <= 65535, "bad arguments");
    Carver cv(workspace, workspace_bytes);
    skeleton_carve(cv);
    if (!cv.fits("region_skeleton")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    long long *out = (long long *)table;
    PCSEG_LAUNCH(skeleton_init_kernel, dim3((unsigned)(((int64_t)cap * 6 + 255) / 256), B), dim3(256), 0, s, out, counts, cap);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(skeleton_table_kernel, dim3(sk_tx(W), sk_ty(H), B), dim3(256), 0, s, labels, peel, counts, H, W, cap, out);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

int pcseg_skeleton_properties(const int64_t *stats, const int64_t *table, const int32_t *counts, double *out, int B, int cap,
                              pcseg_stream_t stream)
{
    PCSEG_REQUIRE(stats && table && counts && out && B >= 1 && B <= 65535 && cap >= 1, "bad arguments");
    PCSEG_LAUNCH(skeleton_properties_kernel, dim3((cap + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, (const long long *)stats,
                 (const long long *)table, counts, out, cap);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
