// The per-frame pair table of voronoi.hip (territory adjacency), agreement.hip (label contingency) and borders.hip (border
// strength; its slot: pair_add_border): open addressing over 64-bit keys with NV 32-bit counters per slot, the probing and
// overflow rule, and the count / scan kernels behind the `offsets` and `totals` of the two-call protocol (first call: fill,
// count, scan; one host read of totals; second call: compact the used slots into rows).  One definition of each.
#pragma once
#include "common.h"

namespace pcseg {

constexpr int PAIR_TABLE_FULL = 1;  // the bit of a frame's overflow word that says "table full" (other bits: the caller's)

template <int NV>
struct PairTable {
    unsigned long long *keys;  // [pair_cap] 0 = free
    unsigned *cnt;             // [pair_cap][NV]
    int *overflow;             // the frame's flag word
    int pair_cap;
};

// the table of frame b among B tables laid out one after the other
template <int NV>
__device__ __forceinline__ PairTable<NV> pair_table_of(unsigned long long *keys, unsigned *cnt, int *overflow, int pair_cap, int b)
{
    return PairTable<NV>{keys + (int64_t)b * pair_cap, cnt + (int64_t)b * pair_cap * NV, overflow + b, pair_cap};
}

// v[0 .. NV) added to key's counters (v[0] always, the others where they are not zero).
// bounded probing: at most pair_cap slots are looked at; a full table raises the flag and drops the pair.  Once the flag is up
// every later pair of the frame is dropped at once (its rows are incomplete anyway): without that each of them would walk the
// whole full table, pairs x pair_cap loads
template <int NV>
__device__ __forceinline__ void pair_add(const PairTable<NV> &t, unsigned long long key, const unsigned (&v)[NV])
{
    if (ld_agent(t.overflow) & PAIR_TABLE_FULL) return;
    unsigned s = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) % (unsigned)t.pair_cap;
    for (int i = 0; i < t.pair_cap; ++i) {
        unsigned long long cur = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&t.keys[s], 0ull, key);
            if (cur == 0) cur = key;
        }
        if (cur == key) {
            atomicAdd(&t.cnt[NV * (size_t)s], v[0]);
#pragma unroll
            for (int k = 1; k < NV; ++k)
                if (v[k]) atomicAdd(&t.cnt[NV * (size_t)s + k], v[k]);
            return;
        }
        s = s + 1 == (unsigned)t.pair_cap ? 0u : s + 1;
    }
    atomicOr(t.overflow, PAIR_TABLE_FULL);
}

// ---- the border slot (borders.hip): a pair's links, its saddle and the 64-bit sum of its link values in the four counters of a
// PairTable<4> slot -- [0] links, [1] ~(bits of the smallest link value) under an atomic max: a zero-filled slot reads as
// "no value yet" (bits 0xFFFFFFFF, above every float in [0, 1]), [2..3] the sum as ONE aligned 64-bit word (the counters start
// on a 256-byte boundary and a slot is 16 bytes).  pair_add's probing and overflow rule, with these three updates at the slot.
constexpr int BORDER_NV = 4;
enum { BORDER_LINKS = 0, BORDER_SADDLE = 1, BORDER_SUM = 2 };

__device__ __forceinline__ void pair_add_border(const PairTable<BORDER_NV> &t, unsigned long long key, unsigned links,
                                                unsigned long long sum, unsigned saddle_bits)
{
    if (ld_agent(t.overflow) & PAIR_TABLE_FULL) return;
    unsigned s = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) % (unsigned)t.pair_cap;
    for (int i = 0; i < t.pair_cap; ++i) {
        unsigned long long cur = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&t.keys[s], 0ull, key);
            if (cur == 0) cur = key;
        }
        if (cur == key) {
            unsigned *c = t.cnt + BORDER_NV * (size_t)s;
            atomicAdd(c + BORDER_LINKS, links);
            atomicMax(c + BORDER_SADDLE, ~saddle_bits);
            atomicAdd(reinterpret_cast<unsigned long long *>(c + BORDER_SUM), sum);
            return;
        }
        s = s + 1 == (unsigned)t.pair_cap ? 0u : s + 1;
    }
    atomicOr(t.overflow, PAIR_TABLE_FULL);
}

// used slots of a frame's table
static __global__ void __launch_bounds__(256) pair_count_kernel(const unsigned long long *__restrict__ keys, int pair_cap,
                                                                 long long *__restrict__ n_pairs)
{
    __shared__ int wsum[4];
    const int b = blockIdx.x;
    const unsigned long long *k = keys + (int64_t)b * pair_cap;
    int n = 0;
    for (int i = threadIdx.x; i < pair_cap; i += 256) n += k[i] != 0;
    int tot;
    block_exclusive_scan<256>(n, &tot, wsum);
    if (threadIdx.x == 0) n_pairs[b] = tot;
}

// offsets[0 .. B] of the frames' rows; totals = {rows, frames whose table was full}
static __global__ void __launch_bounds__(64) pair_scan_kernel(const long long *__restrict__ n_pairs, const int *__restrict__ overflow,
                                                               int B, long long *__restrict__ offsets, long long *__restrict__ totals)
{
    if (threadIdx.x != 0) return;
    long long acc = 0, over = 0;
    for (int b = 0; b < B; ++b) {
        offsets[b] = acc;
        acc += n_pairs[b];
        over += (overflow[b] & PAIR_TABLE_FULL) != 0;
    }
    offsets[B] = acc;
    totals[0] = acc;
    totals[1] = over;
}

// the workspace of the two calls: the tables and the frames' row counts
template <int NV>
struct PairWs {
    unsigned long long *keys;
    unsigned *cnt;
    long long *n_pairs;
};

template <int NV>
static PairWs<NV> pairs_carve(Carver &cv, int B, int pair_cap)
{
    PairWs<NV> ws;
    ws.keys = cv.take<unsigned long long>((size_t)B * pair_cap);
    ws.cnt = cv.take<unsigned>((size_t)B * pair_cap * NV);
    ws.n_pairs = cv.take<long long>((size_t)B);
    return ws;
}

// clears the tables and the flags, to be followed by the caller's fill kernel and pairs_finish
template <int NV>
static int pairs_begin(const PairWs<NV> &ws, int32_t *overflow, int B, int pair_cap, hipStream_t s)
{
    PCSEG_CHECK_HIP(hipMemsetAsync(ws.keys, 0, sizeof(unsigned long long) * (size_t)B * pair_cap, s));
    PCSEG_CHECK_HIP(hipMemsetAsync(ws.cnt, 0, sizeof(unsigned) * NV * (size_t)B * pair_cap, s));
    PCSEG_CHECK_HIP(hipMemsetAsync(overflow, 0, sizeof(int32_t) * B, s));
    return PCSEG_OK;
}

// offsets and totals of the filled tables
template <int NV>
static int pairs_finish(const PairWs<NV> &ws, const int32_t *overflow, int64_t *offsets, int64_t *totals, int B, int pair_cap,
                        hipStream_t s)
{
    PCSEG_LAUNCH(pair_count_kernel, dim3(B), dim3(256), 0, s, (const unsigned long long *)ws.keys, pair_cap, ws.n_pairs);
    PCSEG_CHECK_LAUNCH();
    PCSEG_LAUNCH(pair_scan_kernel, dim3(1), dim3(64), 0, s, (const long long *)ws.n_pairs, (const int *)overflow, B,
                 (long long *)offsets, (long long *)totals);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // namespace pcseg
