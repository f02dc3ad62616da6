// Marked-tile rounds: the driver of the tile-iterated fixed points (watershed.hip: minimax levels and second-level keys;
// reconstruct.hip: grayscale reconstruction).  It knows nothing of what a tile holds or how large it is.
//
// The scheme.  A tile converges in LDS (the user's visit), is stored, and marks every neighbour tile that reads a rim pixel
// the visit changed.  A round visits the marked tiles: it reads one of two mark buffers and writes the other (take_mark,
// mark_tile); with a list, the first marker of a tile appends it to the next round's device list, which a small fixed grid
// walks (for_tiles).  The host enqueues a fixed number of grid rounds whatever the data -- nothing is read back -- and then
// a tail kernel, one block per frame, that finishes what is still marked (tail_rounds) under a round cap.
//
// What a user owes the scheme.  Its iteration is monotone, so whatever a tile reads from a neighbour's rim while that
// neighbour stores it -- an older or a newer value, never a mixture: stores are naturally aligned words -- is a bound of
// the fixed point.  A tile marks AFTER its store and in the buffer the NEXT round reads: the reader is visited again and
// then sees the stored value (kernel boundary; in a tail kernel the block's own barrier).  A tile is visited by one block
// per round, so its own pixels have one writer.  When a round marks nothing every tile is at its local fixed point for
// the halo values that are stored now, and the frame is at its fixed point.
#pragma once

#include "common.h"

namespace pcseg {

// ---- work lists.  Work that is a few tiles of a few frames is LISTED on the
// device and walked by a small fixed grid: a launch over every tile retires thousands of workgroups that read one byte and
// leave, each of which first has to find a CU with its LDS and wave slots free among the kernels of the other batches in
// flight (2 048 blocks of 1 024 threads and 58 KB for one K2 round; same box, fewer such grid rounds made the STEP faster
// although the serial time went up: 4.53-4.57 ms against 4.62-4.75, profiles/r04/ab_logs/r4f_*).  ONE walk serves every
// list: entries first, first + stride, .. below the count as it is when the kernel starts.
template <typename Body>
__device__ __forceinline__ void walk_list(const int *list, const int *count, int first, int stride, Body &&body)
{
    const int n = *count;
    for (int i = first; i < n; i += stride) body(list[i]);
}

// Tiles: entry = frame * tiles per frame + tile.  Blocks walk with the grid's stride; a body that uses LDS ends with a
// barrier: the next tile reuses it.
struct TileAt {
    int b, tx, ty;  // frame, tile column, tile row
};
struct TileList {
    const int *list;
    const int *count;  // number of entries
    int ntpf, tilesX;  // tiles per frame, tiles per tile row
    __device__ __forceinline__ TileAt at(int e) const  // the tile of entry e
    {
        const int b = e / ntpf, t = e % ntpf;
        return TileAt{b, t % tilesX, t / tilesX};
    }
};

template <typename Body>
__device__ __forceinline__ void for_tiles(const TileList &tl, Body &&body)
{
    walk_list(tl.list, tl.count, blockIdx.x, gridDim.x, [&](const int e) {
        const TileAt t = tl.at(e);
        body(t.b, t.tx, t.ty);
    });
}

// ---- tile marks.  One mark per tile, "a neighbour changed my halo", in two buffers: a
// round reads one and writes the other.  A visited tile takes its mark down itself: the buffer is all zero again when it
// becomes the output of the round after next, and no memset has to sit between two rounds.  Block-uniform: false = no
// mark, the block leaves the tile; every thread has read the mark before thread 0 clears it.
__device__ __forceinline__ bool take_mark(uint8_t *mark)
{
    if (!*mark) return false;
    __syncthreads();
    if (threadIdx.x == 0) *mark = 0;
    return true;
}

// Mark tile m (index into the mark buffer of the round after this one).  With a list the next round walks the marked
// tiles: the first marker of a tile appends it -- test-and-set on the mark's byte inside its 32-bit word.  PRECONDITION:
// the mark buffers are 256-byte aligned and padded to a multiple of that (Carver::take), so the word around byte m is
// the buffer's own.  Without a list (the next round scans the marks or looks at each tile's own): a plain byte store.
__device__ __forceinline__ void mark_tile(uint8_t *marks, int *list_out, int *count_out, int64_t m)
{
    if (list_out) {
        const unsigned bit = 1u << (8 * (int)(m & 3));
        const unsigned old = atomicOr(reinterpret_cast<unsigned *>(marks + (m & ~(int64_t)3)), bit);
        if (!(old & bit)) list_out[atomicAdd(count_out, 1)] = (int)m;
    } else {
        marks[m] = 1;
    }
}

// A tiling of a frame: tile (tx, ty) starts at (ty * T - off, tx * T - off).  Rounds may alternate between two (the
// watershed's levels: the tile borders of one round are tile centres of the next); the mark buffer a round reads is in
// that round's layout.
struct Tiling {
    int off;     // 0 or T / 2
    int nx, ny;  // tiles per frame in x and y
};

// ---- the tail.  The fixed points are driven WITHOUT the host: a fixed number of grid rounds is enqueued (a round that finds no mark
// costs a few microseconds), and whatever is still marked after them -- a few tiles of a few frames, if anything -- is
// finished by a tail kernel: one block per frame walks the frame's marked tiles round by round until a round marks
// nothing.  Rounds of one frame only depend on that frame's tiles, so the block's own barrier is the only synchronisation
// (stores and loads of one workgroup go through the same L1).  This is that block's loop for frame b; the tail kernels
// supply the tilings of even and odd rounds, counts(t) -- does marked tile t count (one that does not is never visited) --
// and visit(cur, nxt, tx, ty, din, dout): one tile of tiling cur, takes its mark in din down, marks tiles of nxt in dout.
// It gives up after max_rounds rounds (cannot happen for a monotone fixed point; never spin for ever): what the frame holds
// is then no fixed point and must not be used as one.  Returns, block-uniformly, the number of rounds it ran, or a negative
// value when it gave up; it writes no flag itself -- what giving up means is the caller's.
constexpr int TAIL_LIST = 1024;  // marked tiles a tail kernel lists per round (more: it walks every tile)

template <int THREADS, typename Counts, typename Visit>
__device__ __forceinline__ int tail_rounds(const int b, uint8_t *din, uint8_t *dout, const int first_round, const int max_rounds,
                                           const Tiling &t_even, const Tiling &t_odd, Counts &&counts, Visit &&visit)
{
    __shared__ int tail_list[TAIL_LIST];
    __shared__ int tail_count;
    for (int round = first_round;; ++round) {
        const Tiling cur = (round & 1) ? t_odd : t_even, nxt = (round & 1) ? t_even : t_odd;
        const int ntiles = cur.nx * cur.ny;
        const uint8_t *marks = din + (int64_t)b * ntiles;
        // the round's work list: the marked tiles, gathered in parallel (walking ALL tiles and letting each look at its own
        // mark costs a dependent global load per tile -- 256 round trips per round for a handful of marked tiles)
        __syncthreads();  // (a block that walks a frame list: the frame before has read tail_count)
        if (threadIdx.x == 0) tail_count = 0;
        __syncthreads();
        for (int t = threadIdx.x; t < ntiles; t += THREADS)
            if (marks[t] != 0 && counts(t)) {
                const int k = atomicAdd(&tail_count, 1);
                if (k < TAIL_LIST) tail_list[k] = t;
            }
        __syncthreads();
        const int marked = tail_count;
        if (marked == 0) return round - first_round;
        if (round - first_round >= max_rounds) return -1;
        const int walk = marked <= TAIL_LIST ? marked : ntiles;  // (a list that overflowed: every tile, each checks its mark)
        for (int k = 0; k < walk; ++k) {
            const int t = marked <= TAIL_LIST ? tail_list[k] : k;
            visit(cur, nxt, t % cur.nx, t / cur.nx, din, dout);
            __syncthreads();  // the tile's stores (keys, marks) before the next tile loads its halo / the next round scans
        }
        uint8_t *tmp = din; din = dout; dout = tmp;
    }
}

}  // namespace pcseg
