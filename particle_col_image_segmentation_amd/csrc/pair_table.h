// The per-frame pair table of voronoi.hip (territory adjacency), agreement.hip (label contingency) and borders.hip (border
// strength): open addressing over 64-bit keys with NV 32-bit counters per slot, and the two-call protocol around it.  One
// definition of each:
//   pair_slot          the probing and overflow rule: the slot of a key, or -1 where the pair is dropped.  What is added at the
//                      slot is the caller's (pair_add: NV counters; borders.hip: links, saddle and a 64-bit sum)
//   pair_count_kernel, pair_scan_kernel   behind `offsets` and `totals` of the first call (pairs_begin, the caller's fill
//                      kernel, pairs_finish); then one host read of totals
//   pair_write_kernel  the second call (pairs_write): a frame's used slots compacted into rows, in table order; what a row
//                      holds is the caller's emit functor.  (Until this kernel the three files had a copy each:
//                      terr_pairs_write_kernel, ag_write_kernel, border_write_kernel -- the names in timings recorded before)
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

// the slot of key, claimed if the key is new; -1 where the pair is dropped.
// bounded probing: at most pair_cap slots are looked at; a full table raises the flag and drops the pair.  Once the flag is up
// every later pair of the frame is dropped at once (its rows are incomplete anyway): without that each of them would walk the
// whole full table, pairs x pair_cap loads
template <int NV>
__device__ __forceinline__ int pair_slot(const PairTable<NV> &t, unsigned long long key)
{
    if (ld_agent(t.overflow) & PAIR_TABLE_FULL) return -1;
    unsigned s = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) % (unsigned)t.pair_cap;
    for (int i = 0; i < t.pair_cap; ++i) {
        unsigned long long cur = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&t.keys[s], 0ull, key);
            if (cur == 0) cur = key;
        }
        if (cur == key) return (int)s;
        s = s + 1 == (unsigned)t.pair_cap ? 0u : s + 1;
    }
    atomicOr(t.overflow, PAIR_TABLE_FULL);
    return -1;
}

// v[0 .. NV) added to key's counters (v[0] always, the others where they are not zero)
template <int NV>
__device__ __forceinline__ void pair_add(const PairTable<NV> &t, unsigned long long key, const unsigned (&v)[NV])
{
    const int s = pair_slot(t, key);
    if (s < 0) return;
    atomicAdd(&t.cnt[NV * (size_t)s], v[0]);
#pragma unroll
    for (int k = 1; k < NV; ++k)
        if (v[k]) atomicAdd(&t.cnt[NV * (size_t)s + k], v[k]);
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
    int *tail;  // tail_ints values of the caller's behind the tables (borders.hip: the merge's parents)
};

template <int NV>
static PairWs<NV> pairs_carve(Carver &cv, int B, int pair_cap, size_t tail_ints)
{
    PairWs<NV> ws;
    ws.keys = cv.take<unsigned long long>((size_t)B * pair_cap);
    ws.cnt = cv.take<unsigned>((size_t)B * pair_cap * NV);
    ws.n_pairs = cv.take<long long>((size_t)B);
    ws.tail = cv.take<int>(tail_ints);
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

// the used slots of frame blockIdx.x, in table order, as rows offsets[b] ..: emit(b, key, c, row) writes the row of a used
// slot, c its Emit::NV counters (one block of 256 per frame walks the table in chunks of 256 slots)
template <class Emit>
__global__ void __launch_bounds__(256) pair_write_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ cnt,
                                                          int pair_cap, const long long *__restrict__ offsets, Emit emit)
{
    __shared__ int wsum[4];
    const int b = blockIdx.x;
    const unsigned long long *k = keys + (int64_t)b * pair_cap;
    const unsigned *v = cnt + (int64_t)b * pair_cap * Emit::NV;
    long long row0 = offsets[b];
    for (int base = 0; base < pair_cap; base += 256) {
        const int i = base + (int)threadIdx.x;
        const unsigned long long key = i < pair_cap ? k[i] : 0ull;
        int tot;
        const int pos = block_exclusive_scan<256>((int)(key != 0), &tot, wsum);
        if (key) emit(b, key, v + Emit::NV * (size_t)i, row0 + pos);
        row0 += tot;
    }
}

// the second call: the caller's workspace carved again (tail_ints: as pairs_carve) and the rows written
template <class Emit>
static int pairs_write(const char *who, const void *workspace, size_t workspace_bytes, int B, int pair_cap, size_t tail_ints,
                       const int64_t *offsets, Emit emit, pcseg_stream_t stream)
{
    Carver cv(const_cast<void *>(workspace), workspace_bytes);
    const PairWs<Emit::NV> ws = pairs_carve<Emit::NV>(cv, B, pair_cap, tail_ints);
    if (!cv.fits(who)) return PCSEG_ERR_WORKSPACE;
    PCSEG_LAUNCH(pair_write_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const unsigned long long *)ws.keys,
                 (const unsigned *)ws.cnt, pair_cap, (const long long *)offsets, emit);
    PCSEG_CHECK_LAUNCH();
    return PCSEG_OK;
}

}  // namespace pcseg
