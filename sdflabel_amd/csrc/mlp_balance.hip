// Next launch order of the exact-f32 grid forward's tiles (tile_balance.h): the state's set-up and the ranking that runs behind every
// balanced forward.  Both are kernels -- no memset or copy node, so that every entry point may be captured into a graph (sdfr_common.h).
#include <hip/hip_runtime.h>
#include "sdfr_common.h"
#include "tile_balance.h"

constexpr int TB_NT = 256, TB_WAVES = TB_NT / 64;      // a wave ranks and moves one chunk

// order[] = fixed[] = the caller's order; cost[] = last[] = ctl[] = 0; at[] = the identity
__global__ __launch_bounds__(256) void sdfr_tile_balance_init_kernel(int32_t* __restrict__ state, const int32_t* __restrict__ order, int64_t order_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t T = sdfr_tb_chunks(order_rows);
    if (i < 3 * T + SDFR_TB_CTL) state[i] = (i < 2 * T || i >= 3 * T) ? 0 : (int32_t)(i - 2 * T);
    if (i < order_rows) {
        const int32_t o = order[i];
        state[sdfr_tb_order_word(order_rows) + i] = o;
        state[sdfr_tb_fixed_word(order_rows) + i] = o;
    }
}

// ceil(T / 4) workgroups, wave w of workgroup b owns chunk c = 4 b + w.  Every workgroup copies the T <= SDFR_TB_MAX_CHUNKS costs the
// forward launches added into LDS; a wave ranks its chunk by (cost descending, static index ascending) -- each lane counts a 64th of the
// chunks in front, the wave adds the counts -- keeps the cost in last[], enters at[rank] = c and moves the chunk's 64 entries of fixed[] to
// place rank of order[]; a partial last chunk keeps the last place.  Every entry of order[] and at[] is written on every call, order[] from
// fixed[]: whatever the cost words held, the result is the static order with whole chunks moved.  The costs are zeroed by the workgroup
// that is the last to have read them (ctl[0] counts the readers and goes back to 0 with them).
__global__ __launch_bounds__(TB_NT) void sdfr_tile_balance_kernel(int32_t* __restrict__ state, int64_t order_rows) {
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
    const int c = (int)blockIdx.x * TB_WAVES + wave;
    const int64_t i = (int64_t)c * SDFR_TB_CHUNK + lane;
    const bool moves = c < T && i < order_rows;
    const int32_t entry = moves ? fixed[i] : 0;        // (requested in front of the costs: one round trip to memory for both)
    for (int k = tid; k < T; k += TB_NT) cost[k] = g_cost[k];
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
    if (tid == 0) last_reader = atomicAdd(ctl, 1) == (int)gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (last_reader) {                                 // every workgroup has the costs in LDS: nobody reads the words again
        for (int k = tid; k < T; k += TB_NT) g_cost[k] = 0;
        if (tid == 0) ctl[0] = 0;
    }
}

void sdfr_launch_tile_balance_init(int32_t* state, const int32_t* order, int64_t order_rows, hipStream_t s) {
    const int64_t head = 3 * sdfr_tb_chunks(order_rows) + SDFR_TB_CTL, n = order_rows > head ? order_rows : head;
    hipLaunchKernelGGL(sdfr_tile_balance_init_kernel, dim3(sdfr_cdiv(n, 256)), dim3(256), 0, s, state, order, order_rows);
}

void sdfr_launch_tile_balance(int32_t* state, int64_t order_rows, hipStream_t s) {
    hipLaunchKernelGGL(sdfr_tile_balance_kernel, dim3(sdfr_cdiv(sdfr_tb_chunks(order_rows), TB_WAVES)), dim3(TB_NT), 0, s, state, order_rows);
}
