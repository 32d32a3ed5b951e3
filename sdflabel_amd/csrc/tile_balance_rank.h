// The ranking of tile_balance.h as the work of ONE workgroup of NT threads, shared by the kernel that only ranks (mlp_balance.hip) and by the
// launch that ranks behind the band selection (band_rank.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include "tile_balance.h"

constexpr int TB_NT = 256;                             // threads of the kernel that only ranks; a wave ranks and moves one chunk

static inline int sdfr_tb_rank_blocks(int64_t order_rows, int nt) { return (int)((sdfr_tb_chunks(order_rows) + nt / 64 - 1) / (nt / 64)); }

// Workgroup `blk` of `nblk` = sdfr_tb_rank_blocks(order_rows, NT), wave w owns chunk c = (NT / 64) blk + w.  Every workgroup copies the
// T <= SDFR_TB_MAX_CHUNKS costs the forward launches added into LDS; a wave ranks its chunk by (cost descending, static index ascending) --
// each lane counts a 64th of the chunks in front, the wave adds the counts -- keeps the cost in last[], enters at[rank] = c and moves the
// chunk's 64 entries of fixed[] to place rank of order[]; a partial last chunk keeps the last place.  Every entry of order[] and at[] is
// written on every call, order[] from fixed[]: whatever the cost words held, the result is the static order with whole chunks moved.  The
// costs are zeroed by the workgroup that is the last to have read them (ctl[0] counts the readers and goes back to 0 with them): nobody waits.
template <int NT>
__device__ __forceinline__ void sdfr_tb_rank_block(int32_t* __restrict__ state, int64_t order_rows, int blk, int nblk) {
    __shared__ int32_t cost[SDFR_TB_MAX_CHUNKS];
    __shared__ int last_reader;
    const int T = (int)sdfr_tb_chunks(order_rows), full = (int)sdfr_tb_full_chunks(order_rows);
    int32_t* g_cost = state + sdfr_tb_cost_word(order_rows);
    int32_t* g_last = state + sdfr_tb_last_word(order_rows);
    int32_t* g_at = state + sdfr_tb_at_word(order_rows);
    int32_t* ctl = state + sdfr_tb_ctl_word(order_rows);
    int32_t* order = state + sdfr_tb_order_word(order_rows);
    const int32_t* fixed = state + sdfr_tb_fixed_word(order_rows);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blk * (NT / 64) + wave;
    const int64_t i = (int64_t)c * SDFR_TB_CHUNK + lane;
    const bool moves = c < T && i < order_rows;
    const int32_t entry = moves ? fixed[i] : 0;        // (requested in front of the costs: one round trip to memory for both)
    for (int k = tid; k < T; k += NT) cost[k] = g_cost[k];
    __syncthreads();                                   // this workgroup's reads of the costs are complete: their values are in LDS
    if (c < T) {
        int r = c;
        if (c < full) {
            r = sdfr_tb_rank_part(cost, full, c, lane, 64);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) r += __shfl_xor(r, d, 64);
        }
        if (lane == 0) {
            g_last[c] = cost[c];
            g_at[r] = c;
        }
        if (moves) order[sdfr_tb_dest(c, r, lane, full)] = entry;
    }
    if (tid == 0) last_reader = atomicAdd(ctl, 1) == nblk - 1 ? 1 : 0;
    __syncthreads();
    if (last_reader) {                                 // every workgroup has the costs in LDS: nobody reads the words again
        for (int k = tid; k < T; k += NT) g_cost[k] = 0;
        if (tid == 0) ctl[0] = 0;
    }
}
