// Launch order of the exact-f32 grid forward's tiles from the last pass's K counts (profiles/fwd_balance_notes.md), shared by
// the kernels (mlp_kernel.h, mlp_balance.hip) and by the host program under tests/fwd_balance_host/.
//
// The ORDER launch evaluates the rows of sdfr_grid_tile_order 64 at a time: CHUNK c of the order is its entries [64 c, 64 c + 64), one
// 4x4x4 block of the grid where the density is a multiple of 4.  Since the per-tile K compaction a tile's time follows the K extent its
// compacted products walk (measured: correlation 0.9994), the 1000 tiles of the headline's launch are 3.9 per CU, and the hardware hands
// workgroups out in blockIdx order: whatever is heavy and late makes the tail.  So the forward reports each tile's COST, and a small kernel
// behind it ranks the chunks heaviest first for the NEXT launch of the same state.  The prior is one step old; a stale or meaningless one costs
// time, never a bit -- a row's arithmetic depends on the rows that share its tile, and chunks stay whole.
//
// Cost of a tile: the K extent the compacted products walked, summed over the compacted layers -- per layer the tile's surviving operand
// features padded as the k list pads them (kc_slots.h: sdfr_kc_padded).  Integers in steps of 16; a launch of several crops adds the crops'
// costs of a chunk (integer adds: the sum does not depend on the order of the workgroups).
//
// State of one order (device memory, int32 words; sdfr_mlp_balance_bytes):
//   cost [T]           T = sdfr_tb_chunks(order_rows): what the forward launches since the last ranking added
//   last [T]           the costs the last ranking read (kept for the caller to look at; nothing reads them back)
//   at   [T]           the chunk of the static order at each place of order[]: the tile at launch place p reports to cost[at[p]]
//   ctl  [4]           [0]: workgroups of the running ranking that have read the costs (the last one zeroes them, and this word)
//   order[order_rows]  the order the next launch uses: always written by sdfr_mlp_balance_init or by the ranking, from `fixed` alone
//   fixed[order_rows]  the caller's static order
// The rule: full chunks go by (cost descending, static index ascending); a partial last chunk (order_rows % 64 != 0) keeps the last place.
// Whatever the cost words hold -- negative, huge, anything -- the ranks of the full chunks are a permutation of [0, full): the comparison is a
// strict total order on (cost, index).  Rank by enumeration, T^2 integer comparisons: orders of more than SDFR_TB_MAX_CHUNKS chunks (tens of
// rounds on the device: no tail to speak of) are not ranked and keep the static order.
#pragma once
#include <stdint.h>
#include "kc_slots.h"
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDFR_TB_HD __host__ __device__ __forceinline__
#else
#define SDFR_TB_HD inline
#endif

constexpr int SDFR_TB_CHUNK = 64;               // entries of a chunk = rows of a tile of the ORDER kernels
constexpr int SDFR_TB_MAX_CHUNKS = 4096;        // largest order that is ranked (every workgroup of the ranking holds all costs in LDS)
constexpr int SDFR_TB_CTL = 4;                  // control words of the state

SDFR_TB_HD int64_t sdfr_tb_chunks(int64_t order_rows) { return (order_rows + SDFR_TB_CHUNK - 1) / SDFR_TB_CHUNK; }
SDFR_TB_HD int64_t sdfr_tb_full_chunks(int64_t order_rows) { return order_rows / SDFR_TB_CHUNK; }
SDFR_TB_HD bool sdfr_tb_ranked(int64_t order_rows) { return sdfr_tb_chunks(order_rows) <= SDFR_TB_MAX_CHUNKS; }
// the place in the order at which a tile of the launch starts, in chunks: the one its first slot lies in (order_rows a multiple of 64:
// tile % chunks, for every crop); the chunk of the static order that sits there is at[place]
// With several crops and order_rows % 64 != 0 the tiles of the crops behind the first straddle chunks (and crops): such a tile's whole cost
// goes to the chunk of its first slot, and a moved order no longer keeps its rows together -- the costs are approximate there, the bits are not
// (32-bit arithmetic: a launch has fewer than 2^31 rows, so 64 tile < 2^32 and order_rows < 2^31)
SDFR_TB_HD int sdfr_tb_place_of_tile(int64_t tile, int64_t order_rows) {
    return (int)((uint32_t)tile * (uint32_t)SDFR_TB_CHUNK % (uint32_t)order_rows / (uint32_t)SDFR_TB_CHUNK);
}
// what one compacted layer adds to its tile's cost: `survivors` operand features, padded as the k list is
SDFR_TB_HD int sdfr_tb_layer_cost(int survivors) { return sdfr_kc_padded(survivors); }

// state layout, int32 words
SDFR_TB_HD int64_t sdfr_tb_cost_word(int64_t order_rows) { (void)order_rows; return 0; }
SDFR_TB_HD int64_t sdfr_tb_last_word(int64_t order_rows) { return sdfr_tb_chunks(order_rows); }
SDFR_TB_HD int64_t sdfr_tb_at_word(int64_t order_rows) { return 2 * sdfr_tb_chunks(order_rows); }
SDFR_TB_HD int64_t sdfr_tb_ctl_word(int64_t order_rows) { return 3 * sdfr_tb_chunks(order_rows); }
SDFR_TB_HD int64_t sdfr_tb_order_word(int64_t order_rows) { return 3 * sdfr_tb_chunks(order_rows) + SDFR_TB_CTL; }
SDFR_TB_HD int64_t sdfr_tb_fixed_word(int64_t order_rows) { return sdfr_tb_order_word(order_rows) + order_rows; }
SDFR_TB_HD int64_t sdfr_tb_state_words(int64_t order_rows) { return sdfr_tb_order_word(order_rows) + 2 * order_rows; }
// the cost word a tile at `place` adds to: at[place] when that names a chunk, the place itself otherwise (a state nobody initialised)
SDFR_TB_HD int sdfr_tb_cost_index(int at_place, int place, int64_t order_rows) {
    return (uint32_t)at_place < (uint32_t)sdfr_tb_chunks(order_rows) ? at_place : place;
}

// place of full chunk i in the next launch: the chunks in front of it in (cost descending, static index ascending).  The count over the
// chunks j = first, first + step, ...: the device sums the 64 parts of a wave's lanes (first = lane, step = 64), the host takes it whole
SDFR_TB_HD int sdfr_tb_rank_part(const int32_t* cost, int full, int i, int first, int step) {
    const int32_t ci = cost[i];
    int r = 0;
    for (int j = first; j < full; j += step) {
        const int32_t cj = cost[j];
        r += (cj > ci || (cj == ci && j < i)) ? 1 : 0;
    }
    return r;
}
SDFR_TB_HD int sdfr_tb_rank(const int32_t* cost, int full, int i) { return sdfr_tb_rank_part(cost, full, i, 0, 1); }
// entry e of the next order, given the rank of the chunk it belongs to in the static order
SDFR_TB_HD int64_t sdfr_tb_dest(int64_t chunk, int rank, int e, int64_t full) {
    return (chunk < full ? (int64_t)rank : chunk) * SDFR_TB_CHUNK + e;
}

// The whole rule on the host: next[] and at[] from cost[] and fixed[] (tests; the device kernel runs the same functions, a chunk per wave)
inline void sdfr_tb_next_order_host(const int32_t* cost, const int32_t* fixed, int32_t* next, int32_t* at, int64_t order_rows) {
    const int64_t T = sdfr_tb_chunks(order_rows), full = sdfr_tb_full_chunks(order_rows);
    for (int64_t c = 0; c < T; ++c) {
        const int rank = (c < full && sdfr_tb_ranked(order_rows)) ? sdfr_tb_rank(cost, (int)full, (int)c) : (int)c;
        const int64_t n = c < full ? SDFR_TB_CHUNK : order_rows - full * SDFR_TB_CHUNK;
        at[rank] = (int32_t)c;
        for (int e = 0; e < n; ++e) next[sdfr_tb_dest(c, rank, e, full)] = fixed[c * SDFR_TB_CHUNK + e];
    }
}
