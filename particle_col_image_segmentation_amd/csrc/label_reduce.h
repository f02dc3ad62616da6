// The shared layer of the per-label reductions (reduce.hip, shape.hip, refined.hip): the look-ahead fence, the segmented
// wave reduction, the tagged LDS slot table and the column-run walk.  One definition of each; a kernel brings a policy
// (what a run contributes, how it is committed), its LDS tables and its launch shape.
#pragma once
#include "common.h"

namespace pcseg {

// ---- look-ahead fence
// The row walks fetch row r + 1 before they process row r.  The compiler's wait-count pass cannot count loads across
// the loop's back edge: left alone it puts `s_waitcnt vmcnt(0)` at the first USE of row r -- after the loads of row r + 1
// went out -- and every step then waits a full memory latency (the plane-free pass ran at 1.3 TB/s for that reason).
// "Using" row r's registers in an empty asm ahead of the fetch moves that wait to the top of the step, where only row
// r's loads are outstanding.
__device__ __forceinline__ void landed(const int4 &q) { asm volatile("" ::"v"(q.x), "v"(q.y), "v"(q.z), "v"(q.w) : "memory"); }
__device__ __forceinline__ void landed(const float4 &q) { asm volatile("" ::"v"(q.x), "v"(q.y), "v"(q.z), "v"(q.w) : "memory"); }
__device__ __forceinline__ void landed(unsigned q) { asm volatile("" ::"v"(q) : "memory"); }

// ---- labels of a row
// four labels of a row as one 16-byte load
__device__ __forceinline__ int4 ld_labels4(const int *p) { return *reinterpret_cast<const int4 *>(p); }

// the labels of columns c .. c + 3 of the row that starts at `row`, zeros beyond the frame's width.
// VEC: W % 4 == 0 and a 16-byte aligned image: one 16-byte load; otherwise four guarded 4-byte loads
template <bool VEC>
__device__ __forceinline__ int4 row_labels4(const int *row, int c, int W)
{
    int4 q = make_int4(0, 0, 0, 0);
    if (c < W) {
        const int *at = row + c;
        if (VEC) {
            q = ld_labels4(at);
        } else {
            q.x = at[0];
            if (c + 1 < W) q.y = at[1];
            if (c + 2 < W) q.z = at[2];
            if (c + 3 < W) q.w = at[3];
        }
    }
    return q;
}

// ---- the wave segment: a run of neighbouring lanes with equal keys
struct WaveSeg {
    bool head;   // first lane of its segment
    int remain;  // lanes after this one in its segment
};

// all 64 lanes call this
template <typename K>
__device__ __forceinline__ WaveSeg wave_segment(K key)
{
    const int lane = lane_id();
    const K left = __shfl_up(key, 1);
    const bool head = lane == 0 || key != left;
    const unsigned long long heads = __ballot(head);
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    return WaveSeg{head, after ? __ffsll((long long)after) - 1 : 63 - lane};
}

// every lane ends with the merge of its own value and those of the lanes after it in its segment (the head: the whole
// segment).  shfl(a, off) is a's value off lanes up, merge(a, o) adds o to a.  All 64 lanes call this.
template <typename T, typename Shfl, typename Merge>
__device__ __forceinline__ void segment_reduce(T &a, int remain, Shfl shfl, Merge merge)
{
    // (kept a loop: unrolled, the six steps cost shape_moments_kernel 78 registers against 68, a wave per SIMD; the walks run
    // it twice a block)
#pragma nounroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const T o = shfl(a, off);
        if (off <= remain) merge(a, o);
    }
}

// ---- the tagged slot table: a block's LDS partials of its hot labels (background, particle), flushed once per block
constexpr int LABEL_SLOTS = 256;

// the slot of label l (> 0) if l owns or can claim it, -1 otherwise: the caller's adds then go straight to global memory.
// (direct-mapped on purpose.  Linear probing over eight slots keeps more labels in the block's LDS table, and measured
// SLOWER where it matters: the float64 plane sums of a colliding label then queue at an LDS float64 atomic instead of
// going to the memory-side one -- the fused sums pass 540 us against 407; the integer pass did not move, 197 against 202)
__device__ __forceinline__ int slot_claim(int *tags, int l)
{
    const int slot = l & (LABEL_SLOTS - 1);
    const int tag = atomicCAS(&tags[slot], 0, l);
    return (tag == 0 || tag == l) ? slot : -1;
}

// flush of a 256-thread block's table: EIGHT LANES PER SLOT, body(slot, label, lane in slot) for every claimed slot, so
// that one atomic instruction carries up to eight neighbouring 8-byte words of a table row's 64-byte line instead of 64
// lanes aiming at 64 different lines eight times over
template <typename Body>
__device__ __forceinline__ void slots_flush8(const int *tags, Body body)
{
    for (int base = 0; base < LABEL_SLOTS; base += 32) {
        const int i = base + (int)(threadIdx.x >> 3);
        const int l = tags[i];
        if (l) body(i, l, (int)(threadIdx.x & 7));
    }
}

// ---- the column-run walk
// A lane owns 4 adjacent columns (c .. c + 3) and walks DOWN the rows [r0, r1) of its block; a vertical run is (key, first
// row, end row) and what it contributes follows in closed form, so the walk itself does no per-pixel work.  What bounds
// such a pass is not the walk but the atomics of the commits, most of them aimed at the slot the neighbouring lanes aim
// at too.  So a finished run is PARKED in two registers, and at the end of the block the wave adds up the runs of
// ADJACENT LANES THAT CARRY THE SAME KEY with a segmented shuffle reduction -- a region a few dozen pixels wide is eight
// lanes -- and only the first lane of each segment commits.
// (measured on the plane-free pass: a four- and an eight-row load ring on the form without parking, 180 and 197 us against
// 179 -- not the loads; parking alone, every lane still committing for itself at the end: 200 us against 185 -- the
// atomics, not the branch.)
//
// The policy P supplies
//   P::Key                      a signed integer; > 0: a key that counts, anything else: none
//   P::Raw, p.load(r)           the lane's loads of row r (zeros beyond the frame's width: all 64 lanes walk, the
//                               reductions at the end want them), with a landed(Raw) overload
//   p.keys(raw, k)              the four keys of a loaded row
//   P::Run, p.run(key, start, end, col)   what the run [start, end) of column col contributes; Run has a member `key`
//   P::shfl(run, off), P::merge(a, o)     the run off lanes up (its key aside), and o added to a
//   p.commit(run)               one contribution with key > 0 into the kernel's table
constexpr int RUN_ROWS = 32;  // rows per block (block partials of the plane-free pass must fit 32 bits: <= 64)
static_assert(RUN_ROWS <= 64, "block-local sums are 32-bit");

template <typename P>
__device__ __forceinline__ void column_run_walk(const P &p, int c, int r0, int r1)
{
    using Key = typename P::Key;
    using Run = typename P::Run;
    Key cur[4] = {0, 0, 0, 0}, parked[4] = {0, 0, 0, 0};
    int start[4] = {0, 0, 0, 0}, parked_rows[4] = {0, 0, 0, 0};  // first row | end row << 16 (rows < 2^15)
    auto parked_run = [&](int j) { return p.run(parked[j], parked_rows[j] & 0xFFFF, parked_rows[j] >> 16, c + j); };
    typename P::Raw next = p.load(r0);
    for (int r = r0; r < r1; ++r) {
        const typename P::Raw now = next;
        landed(now);
        if (r + 1 < r1) next = p.load(r + 1);
        Key k[4];
        p.keys(now, k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k[j] != cur[j]) {
                if (cur[j] > 0) {
                    // (a column seldom ends two runs inside one block)
                    if (parked[j]) p.commit(parked_run(j));
                    parked[j] = cur[j];
                    parked_rows[j] = start[j] | (r << 16);
                }
                cur[j] = k[j];
                start[j] = r;
            }
        }
    }
    // end of the block: the open runs and the parked ones, each folded over the lane's four columns first (they usually sit
    // in the same region), then over the lanes
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        Run q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = pass == 0 ? p.run(cur[j], start[j], r1, c + j) : parked_run(j);
#pragma unroll
        for (int j = 1; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < j; ++i)
                if (q[j].key > 0 && q[j].key == q[i].key) {
                    P::merge(q[i], q[j]);
                    q[j].key = 0;
                }
        // a lane whose first column carries no key hands another column's run to the lane reduction instead
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (q[0].key <= 0 && q[j].key > 0) {
                q[0] = q[j];
                q[j].key = 0;
            }
        if (q[0].key < 0) q[0].key = 0;
        const WaveSeg seg = wave_segment(q[0].key);
        segment_reduce(q[0], seg.remain, [](const Run &a, int off) { return P::shfl(a, off); }, [](Run &a, const Run &o) { P::merge(a, o); });
        if (seg.head && q[0].key > 0) p.commit(q[0]);
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (q[j].key > 0) p.commit(q[j]);
    }
}

// the rows of ONE label image as the walk's keys: the labels themselves
template <bool VEC>
struct LabelRows {
    using Key = int;
    using Raw = int4;
    const int *lab;  // the frame
    int c, W;
    __device__ __forceinline__ Raw load(int r) const { return row_labels4<VEC>(lab + rowoff(r, W), c, W); }
    __device__ __forceinline__ void keys(const Raw &q, Key k[4]) const { k[0] = q.x; k[1] = q.y; k[2] = q.z; k[3] = q.w; }
};

}  // namespace pcseg
