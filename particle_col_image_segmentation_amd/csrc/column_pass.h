// The vertical pass of the separable transforms, stated once: edt.hip (squared distance transform, disk dilation,
// fill_particle) and voronoi.hip (nearest-label transform) both measure, per column, how far a row is from the nearest
// TARGET above and below it, and search along the row afterwards.
//
// CONVENTION.  The image is reduced to one bit per pixel, 32 rows of a column per word, (B, nch, W).  A set bit is a
// target, the pixel distances are measured TO: a zero pixel for the distance transform and its thresholds, a site for the
// nearest-label transform.  Bits of rows at or beyond H are 0 -- the bit kernels mask them with col_valid(), so no reader
// has to.  Two uint16 carries per word join the words of a column: up = distance from the word's first row to the nearest
// target in the words above it, dn = from its last row to the nearest target in the words below it, COL_NONE if there is
// none (rows are below 2^15, check_shape, so a real carry never reaches it).  any[b] = 1 if frame b has a target at all.
#pragma once
#include "common.h"

namespace pcseg {

constexpr int COL_ROWS = 32;            // rows per bit word
constexpr unsigned COL_NONE = 0xFFFFu;  // carry / distance: no target that way in this column
constexpr int COL_STAGE_TRIPS = 4;      // column words a thread fetches as one batch when it stages a row block

// the rows of a word that lie inside the frame, as a mask (rows = min(COL_ROWS, H - first row of the word))
__device__ __forceinline__ unsigned col_valid(int rows) { return rows >= 32 ? 0xFFFFFFFFu : ((1u << rows) - 1u); }

struct ColWs {
    unsigned *bits;
    uint16_t *up, *dn;
    int *any;
    int nch;
};

inline ColWs col_carve(Carver &cv, int B, int H, int W)
{
    ColWs ws;
    ws.nch = (H + COL_ROWS - 1) / COL_ROWS;
    const size_t words = (size_t)B * ws.nch * W;
    ws.bits = cv.take<unsigned>(words);
    ws.up = cv.take<uint16_t>(words);
    ws.dn = cv.take<uint16_t>(words);
    ws.any = cv.take<int>(B);
    return ws;
}

// up, dn and any from the bit words (the one carry kernel, edt.hip).  Zeroes nothing: any[] is cleared by the caller
int col_carry_launch(const ColWs &ws, int B, int H, int W, hipStream_t s);

// row j (0 .. 31) of a word with `rows` rows: du = distance to the nearest target at or above it in the column, dd = to the
// nearest one below it; COL_NONE where there is none
struct ColDist {
    unsigned du, dd;
};
__device__ __forceinline__ ColDist col_nearest(unsigned word, int j, unsigned up, unsigned dn, int rows)
{
    const unsigned le_mask = j == 31 ? 0xFFFFFFFFu : ((2u << j) - 1u);
    const unsigned le = word & le_mask, gt = word & ~le_mask;  // targets in rows <= j (the pixel's own among them), in rows > j
    ColDist d;
    d.du = le ? (unsigned)(j - (31 - __clz(le))) : (up == COL_NONE ? COL_NONE : up + j);
    d.dd = gt ? (unsigned)((__ffs(gt) - 1) - j) : (dn == COL_NONE ? COL_NONE : dn + (rows - 1 - j));
    return d;
}

// A block of 256 threads stages the RB rows from r0 of frame b: f(j, c, du, dd) for every row j < min(RB, H - r0) and column
// c < W.  The column words of COL_STAGE_TRIPS trips (W <= 1024: all of them) are fetched as one batch with their carries,
// then turned into distances: the loads of a batch are in flight together.  RB divides COL_ROWS: the rows lie in one word
template <int RB, typename F>
__device__ __forceinline__ void col_stage_rows(const unsigned *__restrict__ bits, const uint16_t *__restrict__ up,
                                               const uint16_t *__restrict__ dn, int b, int r0, int H, int W, int nch, F f)
{
    static_assert(COL_ROWS % RB == 0, "a block's rows lie in one bit word");
    const int ch = r0 / COL_ROWS, j0 = r0 % COL_ROWS;
    const int rows_in_word = min(COL_ROWS, H - ch * COL_ROWS);
    const int nrows = min(RB, H - r0);
    const int64_t wbase = ((int64_t)b * nch + ch) * W;
    for (int cbase = 0; cbase < W; cbase += 256 * COL_STAGE_TRIPS) {
        unsigned wordv[COL_STAGE_TRIPS], uv[COL_STAGE_TRIPS], dv[COL_STAGE_TRIPS];
#pragma unroll
        for (int t = 0; t < COL_STAGE_TRIPS; ++t) {
            const int c = min(cbase + (int)threadIdx.x + 256 * t, W - 1);
            wordv[t] = bits[wbase + c];
            uv[t] = up[wbase + c];
            dv[t] = dn[wbase + c];
        }
#pragma unroll
        for (int t = 0; t < COL_STAGE_TRIPS; ++t) {
            const int c = cbase + (int)threadIdx.x + 256 * t;
            if (c < W) {
#pragma unroll
                for (int j = 0; j < RB; ++j)
                    if (j < nrows) {
                        const ColDist d = col_nearest(wordv[t], j0 + j, uv[t], dv[t], rows_in_word);
                        f(j, c, d.du, d.dd);
                    }
            }
        }
    }
}

}  // namespace pcseg
