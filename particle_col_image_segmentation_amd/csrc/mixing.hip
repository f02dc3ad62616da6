// Random-labelling envelopes for the pair-distance histograms (refine_boundaries.py:8-12, goal 3: are two strains closer
// together or further apart than chance?).  The points stay where they are; the strain labels are shuffled P times among
// the typed points of a frame (sequential sampling without replacement from a counter-based generator, see
// include/pcseg.h), and the histogram of neighbours.hip is counted for the observed labelling (p = 0) and every shuffle.
// Nothing in the distances changes under relabelling, only the row a pair lands in: d2 and the bin are found ONCE per pair,
// 64 permutations ride in the 64 lanes of a wave.  Exact integers; the bin rule is pcseg_point_neighbours' (d2 with
// contraction off against the d2 thresholds of table_common.h).
//
// Launches (all asynchronous, no host read):
//   mix_compact_kernel  one block per frame: the typed points (0 <= slot < K) in the caller's order into workspace arrays,
//                       the per-slot counts and the frame's number of work items
//   mix_scan_kernel     one block: exclusive prefix of the work items over the frames
//   mix_label_kernel    one block per (frame, group of 64 permutations), lane = permutation: the draws r of 128 points are
//                       hashed by all eight waves into LDS, then wave 0 walks the points in order with its rem[] in
//                       registers; the 64 labels of a point go to the label table as two 64-bit planes (low and high
//                       label bit, bit l = permutation 64 g + l): 16 bytes per point and group.  (The walk is sequential
//                       in the point index, so it is done once per group here and not by every block of the pair walk,
//                       which only sees tiles.)
//   mix_pairs_kernel    persistent grid; work item = (frame, group, tile pair I <= J of MIX_TILE points), every block a
//                       CONTIGUOUS run of items.  Both tiles' coordinates and labels sit in LDS.  A wave takes rows
//                       of I; for one row point i its 64 lanes test 64 points j at once (d2, in range of the bin
//                       chunk), the in-range pairs are compacted with a ballot, and only those are walked one by one with
//                       the lanes as permutations: the pair's d2 is read back wave-uniform and its bin counted against the
//                       thresholds held one per lane (ballot + popcount: no search, no divergence); j's labels are a 4-byte
//                       LDS read (sixteen 2-bit labels per word, four addresses per wave), the lane picks its label,
//                       looks the slot pair up and increments its own row of the LDS histogram (lane stride odd: the
//                       lanes of a wave never share an address and spread over the banks; the block's eight waves share
//                       the rows, so the increment is an LDS atomic add without return).  Flushed into the
//                       (B, P + 1, Q, m) counts with global 64-bit atomics when the run leaves a (frame, group), and every
//                       MIX_FLUSH_ITEMS items so that no 32-bit LDS counter can wrap.
//   mix_reduce_kernel   one wave per (frame, slot pair, 64 bins): per permutation the prefix over the bins, then obs, min,
//                       max, sum and the two rank counts of the plain and the cumulative counts.
#include "table_common.h"

namespace pcseg {

constexpr int MIX_TILE = 256;          // points of a tile of the pair walk: 2 tiles x 32 B per point = 16 KB of LDS
constexpr int MIX_THREADS = 512;       // of a pair-walk block: 8 waves share the tiles and the histogram
constexpr int MIX_GRID = 1024;         // persistent blocks: 4 per CU
constexpr int MIX_HIST_WORDS = 448;    // histogram words per permutation lane in LDS: Q x (bins of a chunk) <= this
constexpr int MIX_MAX_PERM = 65535;
constexpr int MIX_FLUSH_ITEMS = 1 << 15;  // a block adds its LDS histogram to the global counts at least this often
// LDS of a pair-walk block: tiles 16 KB + thresholds (chunk + 1) x 8 B + histogram 64 x (Q chunk | 1) x 4 B <= 16 + 3.6 + 112.3 KB

struct MixArgs {
    const double2 *cxy;        // typed points, frame by frame at the frame's offset
    const int32_t *cslot;
    const int32_t *meta;       // (B, MAX_TYPE_SLOTS + 1): points per slot, n_t
    const int64_t *prefix;     // (B + 1) work items
    const int64_t *foff;
    const int64_t *keys;
    ulonglong2 *lab;           // (G, n): label planes
    const double *thr;         // m + 1 thresholds on d2
    unsigned long long *counts;  // (B, P + 1, Q, m)
    int64_t n;
    unsigned long long seed;
    int B, K, P, G, m;
};

__device__ __forceinline__ int mix_tiles(int nt) { return (nt + MIX_TILE - 1) / MIX_TILE; }

__global__ void __launch_bounds__(256) mix_compact_kernel(const double *__restrict__ xy, const int32_t *__restrict__ slot,
                                                           const int64_t *__restrict__ foff, int K, int G, double2 *__restrict__ cxy,
                                                           int32_t *__restrict__ cslot, int32_t *__restrict__ meta,
                                                           int64_t *__restrict__ items)
{
    __shared__ int wsum[4];
    __shared__ int s_cnt[MAX_TYPE_SLOTS];
    const int b = blockIdx.x;
    const int64_t f0 = foff[b];
    const int n = (int)(foff[b + 1] - f0);
    if (threadIdx.x < MAX_TYPE_SLOTS) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int cnt[MAX_TYPE_SLOTS] = {0, 0, 0, 0};
    int done = 0;
    for (int base = 0; base < n; base += 256) {  // uniform trip count: the scan has barriers
        const int i = base + threadIdx.x;
        int s = -1;
        if (i < n) s = slot[f0 + i];
        const bool typed = s >= 0 && s < K;
        int total;
        const int pos = done + block_exclusive_scan<256>((int)typed, &total, wsum);
        if (typed) {
            cxy[f0 + pos] = make_double2(xy[2 * (f0 + i)], xy[2 * (f0 + i) + 1]);
            cslot[f0 + pos] = s;
#pragma unroll
            for (int t = 0; t < MAX_TYPE_SLOTS; ++t) cnt[t] += s == t;
        }
        done += total;
    }
#pragma unroll
    for (int t = 0; t < MAX_TYPE_SLOTS; ++t)
        if (cnt[t]) atomicAdd(&s_cnt[t], cnt[t]);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t *mt = meta + (int64_t)b * (MAX_TYPE_SLOTS + 1);
        for (int t = 0; t < MAX_TYPE_SLOTS; ++t) mt[t] = s_cnt[t];
        mt[MAX_TYPE_SLOTS] = done;
        const int64_t T = mix_tiles(done);
        items[b] = T * (T + 1) / 2 * G;
    }
}

// prefix[b] = exclusive sum of items[0..b), prefix[B] = total
__global__ void __launch_bounds__(256) mix_scan_kernel(const int64_t *__restrict__ items, int64_t *__restrict__ prefix, int B)
{
    __shared__ long long wsum[4];
    const int per = (B + 255) / 256, lo = min(B, (int)threadIdx.x * per), hi = min(B, lo + per);
    long long v = 0;
    for (int b = lo; b < hi; ++b) v += items[b];
    long long total;
    long long acc = block_exclusive_scan<256>(v, &total, wsum);
    for (int b = lo; b < hi; ++b) {
        prefix[b] = acc;
        acc += items[b];
    }
    if (threadIdx.x == 0) prefix[B] = total;
}

// the labelling of include/pcseg.h: lane = permutation 64 g + lane, p = 0 the observed slots.  r does not depend on the
// labels given so far (tot = n_t - i is known), only the choice of the slot does: the block's eight waves hash
// MIX_LABEL_CHUNK points at a time into LDS (the 64-bit multiplies are most of the work), then wave 0 walks them in order
constexpr int MIX_LABEL_THREADS = 512, MIX_LABEL_CHUNK = 128;

__global__ void __launch_bounds__(MIX_LABEL_THREADS) mix_label_kernel(MixArgs a)
{
    __shared__ unsigned s_r[MIX_LABEL_CHUNK * WAVE];  // r < tot < 2^24
    __shared__ int s_slot[MIX_LABEL_CHUNK];
    __shared__ ulonglong2 s_out[MIX_LABEL_CHUNK];
    constexpr int PER = MIX_LABEL_CHUNK / (MIX_LABEL_THREADS / WAVE);
    const int b = blockIdx.x / a.G, g = blockIdx.x - b * a.G, tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    const unsigned long long p = (unsigned long long)g * 64 + lane;
    const int32_t *mt = a.meta + (int64_t)b * (MAX_TYPE_SLOTS + 1);
    const int nt = mt[MAX_TYPE_SLOTS];
    const int64_t f0 = a.foff[b];
    unsigned rem0 = mt[0], rem1 = mt[1], rem2 = mt[2];
    const unsigned long long head = (((unsigned long long)a.keys[b] & 0xFFFFFFULL) << 40) ^ (p << 24);
    ulonglong2 *out = a.lab + (int64_t)g * a.n + f0;
    for (int c0 = 0; c0 < nt; c0 += MIX_LABEL_CHUNK) {  // block-uniform
        const int cnt = min(MIX_LABEL_CHUNK, nt - c0);
        if (tid < cnt) s_slot[tid] = a.cslot[f0 + c0 + tid];
        for (int t = wave * PER; t < min(cnt, (wave + 1) * PER); ++t) {
            const int i = c0 + t;
            unsigned long long z = (head ^ (unsigned long long)i) * 0x9E3779B97F4A7C15ULL + a.seed;
            z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
            z ^= z >> 27; z *= 0x94D049BB133111EBULL;
            z ^= z >> 31;
            s_r[t * WAVE + lane] = (unsigned)__umul64hi(z, (unsigned long long)(nt - i));
        }
        __syncthreads();
        if (wave == 0) {
            unsigned r = s_r[lane];
            for (int t = 0; t < cnt; ++t) {
                const unsigned rn = s_r[min(t + 1, MIX_LABEL_CHUNK - 1) * WAVE + lane];  // the next draw is on its way
                // the smallest slot with r < rem[0] + .. + rem[s]  (r < tot: slot 3 takes the rest)
                int s = (r >= rem0) + (r >= rem0 + rem1) + (r >= rem0 + rem1 + rem2);
                if (g == 0) {  // block-uniform: lane 0 of group 0 is the observed labelling
                    const int s0 = s_slot[t];
                    s = lane == 0 ? s0 : s;
                }
                rem0 -= s == 0; rem1 -= s == 1; rem2 -= s == 2;
                const unsigned long long lo = __ballot(s & 1), hi = __ballot(s & 2);
                if (lane == 0) s_out[t] = make_ulonglong2(lo, hi);
                r = rn;
            }
        }
        __syncthreads();
        if (tid < cnt) out[c0 + tid] = s_out[tid];  // (the next round's barrier comes before s_out is written again)
    }
}

__device__ __forceinline__ double mix_d2(double ax, double ay, double bx, double by)
{
#pragma clang fp contract(off)  // each product and the sum rounded on their own, as nb_scan_tile does
    const double dx = ax - bx, dy = ay - by;
    const double d2 = dx * dx + dy * dy;
    return d2;
}

// first tile pair index of row ti among the T (T + 1) / 2 pairs (ti <= tj), rows in order
__device__ __forceinline__ int64_t mix_row_start(int64_t ti, int64_t T) { return ti * T - ti * (ti - 1) / 2; }

// the bits of a 16-bit value spread to the even bit positions
__device__ __forceinline__ unsigned mix_spread16(unsigned x)
{
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    return (x | (x << 1)) & 0x55555555u;
}

// the two label planes of a point -> four words of sixteen 2-bit labels: permutation lane l in word l / 16 at bit 2 (l % 16),
// so that a lane gets its label with one 4-byte LDS read (four addresses per wave: broadcasts) and one bit-field extract
__device__ __forceinline__ uint4 mix_label_words(ulonglong2 pl)
{
    const unsigned l0 = (unsigned)pl.x, l1 = (unsigned)(pl.x >> 32), h0 = (unsigned)pl.y, h1 = (unsigned)(pl.y >> 32);
    return make_uint4(mix_spread16(l0 & 0xFFFF) | (mix_spread16(h0 & 0xFFFF) << 1), mix_spread16(l0 >> 16) | (mix_spread16(h0 >> 16) << 1),
                      mix_spread16(l1 & 0xFFFF) | (mix_spread16(h1 & 0xFFFF) << 1), mix_spread16(l1 >> 16) | (mix_spread16(h1 >> 16) << 1));
}

// bins [k0, k0 + mc) of the histogram in this launch
__global__ void __launch_bounds__(MIX_THREADS) mix_pairs_kernel(MixArgs a, int k0, int mc)
{
    extern __shared__ __align__(16) unsigned char mix_lds[];
    double2 *s_xy = (double2 *)mix_lds;                                      // [2][MIX_TILE]
    unsigned *s_lab = (unsigned *)(mix_lds + 2 * MIX_TILE * sizeof(double2));  // [2][MIX_TILE][4]
    double *s_thr = (double *)(mix_lds + 2 * MIX_TILE * (sizeof(double2) + sizeof(uint4)));
    unsigned *s_hist = (unsigned *)(s_thr + mc + 1);  // [64 lanes][mc][Q], lane stride odd
    const int K = a.K, Q = K * (K + 1) / 2, tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    const int stride = (Q * mc) | 1;  // odd: the 64 lanes of an increment spread over the banks
    // slot pair (x, y) -> its row among the Q rows in (a <= b) order, 4 bits each
    unsigned long long lut = 0;
    for (int x = 0; x < K; ++x)
        for (int y = 0; y < K; ++y) {
            const int lo = min(x, y), hi = max(x, y);
            lut |= (unsigned long long)(lo * K - lo * (lo - 1) / 2 + (hi - lo)) << (4 * (x * 4 + y));
        }
    for (int k = tid; k <= mc; k += MIX_THREADS) s_thr[k] = a.thr[k0 + k];
    for (int e = tid; e < 64 * stride; e += MIX_THREADS) s_hist[e] = 0;
    __syncthreads();
    const double tlo = s_thr[0], thi = s_thr[mc];
    // a pair's bin = #{k < mc: thr[k] <= d2} - 1, counted by the 64 lanes at once (d2 is wave-uniform by then): the first
    // 64 lower thresholds stay in a register, one per lane
    const double thr0 = lane < mc ? s_thr[lane] : __longlong_as_double(0x7FF0000000000000LL);
    const unsigned sh = (lane & 15) * 2, wsel = lane >> 4;
    const int64_t total = a.prefix[a.B];
    const int64_t per = (total + gridDim.x - 1) / gridDim.x;
    const int64_t first = per * blockIdx.x, last = min(total, first + per);
    int64_t cur = -1;  // (frame, group) the histogram holds counts of ...
    int held = 0;      // ... from this many items
    for (int64_t item = first; item <= last; ++item) {
        int b = 0, g = 0, ti = 0, tj = 0, nt = 0;
        int64_t key = -1;
        if (item < last) {
            b = last_le(a.prefix, a.B, item);
            nt = a.meta[(int64_t)b * (MAX_TYPE_SLOTS + 1) + MAX_TYPE_SLOTS];
            const int64_t T = mix_tiles(nt), np = T * (T + 1) / 2, local = item - a.prefix[b];
            g = (int)(local / np);
            const int64_t idx = local - g * np;
            int64_t r = (int64_t)(((double)(2 * T + 1) - sqrt((double)((2 * T + 1) * (2 * T + 1) - 8 * idx))) * 0.5);
            r = r < 0 ? 0 : (r > T - 1 ? T - 1 : r);
            while (r + 1 < T && mix_row_start(r + 1, T) <= idx) ++r;
            while (mix_row_start(r, T) > idx) --r;
            ti = (int)r;
            tj = (int)(r + idx - mix_row_start(r, T));
            key = (int64_t)b * a.G + g;
        }
        // block-uniform: add what the histogram holds to the counts of (frame, group) cur -- when the run leaves it, and
        // every MIX_FLUSH_ITEMS items, so that a 32-bit LDS counter holds at most 2^15 x MIX_TILE^2 = 2^31 pairs
        if ((key != cur || held >= MIX_FLUSH_ITEMS) && cur >= 0) {
            held = 0;
            __syncthreads();
            const int cb = (int)(cur / a.G), cg = (int)(cur - (int64_t)cb * a.G);
            const int row = Q * mc;
            for (int e = tid; e < 64 * row; e += MIX_THREADS) {  // consecutive threads: consecutive bins of the counts
                const int l = e / row, qk = e - l * row, q = qk / mc, k = qk - q * mc;
                const unsigned v = s_hist[l * stride + k * Q + q];
                s_hist[l * stride + k * Q + q] = 0;
                const int p = cg * 64 + l;
                if (v && p <= a.P)
                    atomicAdd(&a.counts[(((int64_t)cb * (a.P + 1) + p) * Q + q) * a.m + k0 + k], (unsigned long long)v);
            }
        }
        cur = key;
        ++held;
        if (item == last) break;
        const int64_t f0 = a.foff[b];
        const int i0 = ti * MIX_TILE, j0 = tj * MIX_TILE, ni = min(MIX_TILE, nt - i0), nj = min(MIX_TILE, nt - j0);
        const bool diag = ti == tj;
        __syncthreads();  // the previous item's reads of the tiles, and the flush, are done
        const ulonglong2 *glab = a.lab + (int64_t)g * a.n + f0;
        for (int t = tid; t < 2 * MIX_TILE; t += MIX_THREADS) {
            const int u = t & (MIX_TILE - 1);
            if (t < MIX_TILE ? u < ni : (!diag && u < nj)) {
                const int src = (t < MIX_TILE ? i0 : j0) + u;
                s_xy[t] = a.cxy[f0 + src];
                ((uint4 *)s_lab)[t] = mix_label_words(glab[src]);
            }
        }
        __syncthreads();
        const double2 *jxy = s_xy + (diag ? 0 : MIX_TILE);
        const unsigned *jlab = s_lab + (diag ? 0 : MIX_TILE) * 4 + wsel;
        unsigned *hrow = s_hist + lane * stride;
        for (int ii = wave; ii < ni; ii += MIX_THREADS / WAVE) {  // wave-uniform row point
            const double2 pi = s_xy[ii];
            const unsigned sa = (s_lab[ii * 4 + wsel] >> sh) & 3;
            const unsigned lutrow = (unsigned)(lut >> (16 * sa)) & 0xFFFF;  // this lane's label against 0 .. 3
            for (int jb = diag ? (ii + 1) & ~63 : 0; jb < nj; jb += 64) {
                const int jj = jb + lane;
                bool in = jj < nj && (!diag || jj > ii);
                double d2 = 0.0;
                if (in) {
                    const double2 pj = jxy[jj];
                    d2 = mix_d2(pi.x, pi.y, pj.x, pj.y);
                    in = d2 >= tlo && d2 < thi;
                }
                const int dlo = __double2loint(d2), dhi = __double2hiint(d2);
                unsigned long long mask = __ballot(in);
                while (mask) {  // wave-uniform: up to four in-range pairs at a time, the lanes are the permutations
                    int l[4];
                    bool on[4];
                    unsigned wj[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        on[u] = mask != 0;
                        l[u] = on[u] ? __ffsll((long long)mask) - 1 : 0;
                        mask &= mask - 1;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) wj[u] = jlab[(jb + l[u]) * 4];  // broadcast reads, all in flight
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (!on[u]) break;
                        const double pd2 = __hiloint2double(__builtin_amdgcn_readlane(dhi, l[u]), __builtin_amdgcn_readlane(dlo, l[u]));
                        int k = __popcll(__ballot(thr0 <= pd2)) - 1;
                        for (int c = 64; c < mc; c += 64) k += __popcll(__ballot(c + lane < mc && s_thr[min(c + lane, mc)] <= pd2));
                        const unsigned q = (lutrow >> (4 * ((wj[u] >> sh) & 3))) & 15;
                        atomicAdd(&hrow[k * Q + q], 1u);
                    }
                }
            }
        }
    }
}

// out = (12, B, Q, m): obs, lo, hi, sum, n_le, n_ge of the counts, then the same of the cumulative counts
__global__ void __launch_bounds__(64) mix_reduce_kernel(const unsigned long long *__restrict__ counts, long long *__restrict__ out,
                                                         int B, int P, int Q, int m)
{
    const int chunks = (m + 63) / 64, lane = lane_id();
    const int c = blockIdx.x % chunks;
    const int64_t bq = blockIdx.x / chunks;
    const int b = (int)(bq / Q), q = (int)(bq - (int64_t)b * Q), k = c * 64 + lane;
    unsigned long long obs = 0, cobs = 0, lo = 0, hi = 0, sum = 0, clo = 0, chi = 0, csum = 0;
    long long n_le = 0, n_ge = 0, cn_le = 0, cn_ge = 0;
    for (int p = 0; p <= P; ++p) {
        const unsigned long long *row = counts + (((int64_t)b * (P + 1) + p) * Q + q) * m;
        unsigned long long before = 0;  // the bins below this chunk
        for (int kk = lane; kk < c * 64; kk += 64) before += row[kk];
        if (c > 0) before = __shfl(wave_inclusive_sum(before), WAVE - 1);
        const unsigned long long v = k < m ? row[k] : 0;
        const unsigned long long cum = before + wave_inclusive_sum(v);
        if (p == 0) {
            obs = v; cobs = cum;
        } else {
            lo = p == 1 ? v : min(lo, v); hi = p == 1 ? v : max(hi, v); sum += v;
            n_le += v <= obs; n_ge += v >= obs;
            clo = p == 1 ? cum : min(clo, cum); chi = p == 1 ? cum : max(chi, cum); csum += cum;
            cn_le += cum <= cobs; cn_ge += cum >= cobs;
        }
    }
    if (k >= m) return;
    const int64_t plane = (int64_t)B * Q * m, o = ((int64_t)b * Q + q) * m + k;
    const long long vals[12] = {(long long)obs, (long long)lo, (long long)hi, (long long)sum, n_le, n_ge,
                                (long long)cobs, (long long)clo, (long long)chi, (long long)csum, cn_le, cn_ge};
#pragma unroll
    for (int t = 0; t < 12; ++t) out[t * plane + o] = vals[t];
}

struct MixWorkspace {
    double2 *cxy;
    int32_t *cslot, *meta;
    int64_t *items, *prefix;
    ulonglong2 *lab;
    double *thr;
    unsigned long long *counts;
};

static int mix_groups(int P) { return (P + 1 + 63) / 64; }

static MixWorkspace mix_carve(Carver &cv, int64_t n, int B, int K, int n_edges, int P, bool own_counts)
{
    MixWorkspace w;
    w.cxy = cv.take<double2>((size_t)n);
    w.cslot = cv.take<int32_t>((size_t)n);
    w.meta = cv.take<int32_t>((size_t)B * (MAX_TYPE_SLOTS + 1));
    w.items = cv.take<int64_t>((size_t)B);
    w.prefix = cv.take<int64_t>((size_t)B + 1);
    w.lab = cv.take<ulonglong2>((size_t)n * mix_groups(P));
    w.thr = cv.take<double>((size_t)n_edges);
    w.counts = own_counts ? cv.take<unsigned long long>((size_t)B * (P + 1) * (K * (K + 1) / 2) * (n_edges - 1)) : nullptr;
    return w;
}

static bool mix_shape_ok(int64_t n_points, int B, int K, int n_edges, int P)
{
    return n_points >= 0 && n_points < ((int64_t)1 << 24) && B >= 1 && K >= 1 && K <= MAX_TYPE_SLOTS && n_edges >= 2 &&
           n_edges <= MAX_HIST_BINS + 1 && P >= 0 && P <= MIX_MAX_PERM;
}

}  // namespace pcseg

using namespace pcseg;

extern "C" {

int pcseg_mixing_tile(void) { return MIX_TILE; }

size_t pcseg_mixing_workspace_bytes(int64_t n_points, int B, int K, int n_edges, int n_perm, int with_counts)
{
    if (!mix_shape_ok(n_points, B, K, n_edges, n_perm)) return 0;
    return carved_bytes(mix_carve, n_points, B, K, n_edges, n_perm, with_counts != 0);
}

int pcseg_pair_label_mixing(const double *xy, const int32_t *slot, const int64_t *frame_offsets, const int64_t *frame_keys,
                            int64_t n_points, int B, int K, double scale, const double *edges, int n_edges, int n_perm,
                            uint64_t seed, int64_t *counts, int64_t *envelope, void *workspace, size_t workspace_bytes,
                            pcseg_stream_t stream)
{
    PCSEG_REQUIRE(xy && slot && frame_offsets && frame_keys && envelope && workspace && mix_shape_ok(n_points, B, K, n_edges, n_perm) &&
                      scale > 0.0 && std::isfinite(scale) && hist_edges_ok(edges, n_edges),
                  "bad arguments");
    const int P = n_perm, m = n_edges - 1, Q = K * (K + 1) / 2, G = mix_groups(P);
    Carver cv(workspace, workspace_bytes);
    const MixWorkspace w = mix_carve(cv, n_points, B, K, n_edges, P, counts == nullptr);
    if (!cv.fits("pair_label_mixing")) return PCSEG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    MixArgs a;
    a.cxy = w.cxy; a.cslot = w.cslot; a.meta = w.meta; a.prefix = w.prefix; a.foff = frame_offsets; a.keys = frame_keys;
    a.lab = w.lab; a.thr = w.thr;
    a.counts = counts ? (unsigned long long *)counts : w.counts;
    a.n = n_points; a.seed = seed; a.B = B; a.K = K; a.P = P; a.G = G; a.m = m;
    const int rc = upload_values(s, w.thr, n_edges, [=](int k) { return d2_threshold(edges[k], scale); });
    if (rc != PCSEG_OK) return rc;
    const size_t count_bytes = sizeof(int64_t) * (size_t)B * (P + 1) * Q * m;
    PCSEG_CHECK_HIP(hipMemsetAsync(a.counts, 0, count_bytes, s));
    PCSEG_LAUNCH(mix_compact_kernel, dim3(B), dim3(256), 0, s, xy, slot, frame_offsets, K, G, w.cxy, w.cslot, w.meta, w.items);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(mix_scan_kernel, dim3(1), dim3(256), 0, s, (const int64_t *)w.items, w.prefix, B);
    PCSEG_CHECK_LAUNCH();
    if (n_points > 0) {
        PCSEG_REQUIRE((int64_t)B * G < ((int64_t)1 << 31), "too many (frame, permutation group) pairs");
        PCSEG_LAUNCH(mix_label_kernel, dim3((unsigned)(B * G)), dim3(MIX_LABEL_THREADS), 0, s, a);
        PCSEG_CHECK_LAUNCH();
        // the bins in chunks whose per-lane histogram fits MIX_HIST_WORDS (each chunk walks the pairs again)
        const int chunk = MIX_HIST_WORDS / Q < m ? MIX_HIST_WORDS / Q : m;
        // (an upper bound of the work items from the host's side: every frame at most its points / MIX_TILE + 1 tiles)
        const int64_t tiles = n_points / MIX_TILE + B;
        const int64_t items_max = tiles * (tiles + 1) / 2 * G;
        const int grid = (int)(items_max < MIX_GRID ? items_max : MIX_GRID);
        for (int k0 = 0; k0 < m; k0 += chunk) {
            const int mc = m - k0 < chunk ? m - k0 : chunk;
            const size_t lds = 2 * MIX_TILE * (sizeof(double2) + sizeof(ulonglong2)) + sizeof(double) * (mc + 1) +
                               sizeof(unsigned) * 64 * (size_t)((Q * mc) | 1);
            if (lds > 64 * 1024)
                PCSEG_CHECK_HIP(hipFuncSetAttribute((const void *)mix_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            PCSEG_LAUNCH(mix_pairs_kernel, dim3(grid), dim3(MIX_THREADS), lds, s, a, k0, mc);
            PCSEG_CHECK_LAUNCH();
        }
    }
    PCSEG_LAUNCH(mix_reduce_kernel, dim3((unsigned)((int64_t)B * Q * ((m + 63) / 64))), dim3(64), 0, s,
                 (const unsigned long long *)a.counts, (long long *)envelope, B, P, Q, m);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // extern "C"
