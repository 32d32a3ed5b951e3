// Next launch order of the exact-f32 grid forward's tiles (tile_balance.h): the state's set-up and the ranking that runs behind every
// balanced forward.  Both are kernels -- no memset or copy node, so that every entry point may be captured into a graph (sdfr_common.h).
#include <hip/hip_runtime.h>
#include "sdfr_common.h"
#include "tile_balance_rank.h"

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

// ceil(T / 4) workgroups of sdfr_tb_rank_block (tile_balance_rank.h).  sdfr_band_select_rank runs the same workgroups behind its selection.
__global__ __launch_bounds__(TB_NT) void sdfr_tile_balance_kernel(int32_t* __restrict__ state, int64_t order_rows) {
    sdfr_tb_rank_block<TB_NT>(state, order_rows, (int)blockIdx.x, (int)gridDim.x);
}

void sdfr_launch_tile_balance_init(int32_t* state, const int32_t* order, int64_t order_rows, hipStream_t s) {
    const int64_t head = 3 * sdfr_tb_chunks(order_rows) + SDFR_TB_CTL, n = order_rows > head ? order_rows : head;
    hipLaunchKernelGGL(sdfr_tile_balance_init_kernel, dim3(sdfr_cdiv(n, 256)), dim3(256), 0, s, state, order, order_rows);
}

void sdfr_launch_tile_balance(int32_t* state, int64_t order_rows, hipStream_t s) {
    hipLaunchKernelGGL(sdfr_tile_balance_kernel, dim3(sdfr_tb_rank_blocks(order_rows, TB_NT)), dim3(TB_NT), 0, s, state, order_rows);
}
