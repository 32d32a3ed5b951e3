// Band selection and tile ranking in ONE launch behind the balanced grid forward (gfx950; include/sdfr.h: sdfr_band_select_rank).
//
// Between the end of a one-crop grid forward and the band's Jacobian the GPU is nearly empty: the ranking (mlp_balance.hip), the band count
// and the band scatter (surface.hip) are three dependent launches of a few microseconds each for microseconds of work.  Here the first
// workgroups select and the remaining ones rank; the two halves share nothing, and no workgroup waits for another.
//
// Selection: workgroup (crop b, block k) owns the rows [k R, k R + R) of the crop, R = SDFR_BR_ROWS.  The two-kernel form takes the block's
// offset from per-block counts of a first launch; this one counts the band rows of its crop IN FRONT OF ITS OWN ROWS straight from sdf with
// 16-byte loads -- redundant reads, at most the crop's G floats from L2 for the last block, instead of a launch.  The scatter is
// sdfr_band_scatter_kernel's: ascending grid order, idx / slot / cnt, cap, thr_extra, skip and the sticky `over` bit.
// Compiled with -ffp-contract=off like surface.hip (thr + thr_extra[b] is the only arithmetic).
#include "sdfr_common.h"
#include "tile_balance_rank.h"

constexpr int SDFR_BR_NT = 1024, SDFR_BR_WAVES = SDFR_BR_NT / 64;      // threads = rows of a selection workgroup; a ranking workgroup: 16 chunks
constexpr int SDFR_BR_ROWS = SDFR_BR_NT;
constexpr int SDFR_BR_FLY = 8;                                         // 16-byte loads a thread of the count has in flight

__device__ __forceinline__ int sdfr_br_in(float v, float thr) { return fabsf(v) < thr ? 1 : 0; }

// grid: nsel selection workgroups (B crops x nblk blocks, a crop's LAST block first: it has the longest count), then nrank ranking workgroups.
// G == 0: nsel == 1, the workgroup zeroes cnt[].
__global__ __launch_bounds__(SDFR_BR_NT) void sdfr_band_rank_kernel(const float* __restrict__ sdf, int64_t G, int B, float thr,
                                                                  const float* __restrict__ thr_extra, const int32_t* __restrict__ skip,
                                                                  int32_t* __restrict__ idx, int cap, int32_t* __restrict__ cnt,
                                                                  int32_t* __restrict__ slot, int32_t* __restrict__ over, int over_bit, int nblk,
                                                                  int nsel, int32_t* __restrict__ state, int64_t order_rows, int nrank) {
    const int bid = (int)blockIdx.x;
    if (bid >= nsel) {
        sdfr_tb_rank_block<SDFR_BR_NT>(state, order_rows, bid - nsel, nrank);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (G == 0) {
        for (int b = tid; b < B; b += SDFR_BR_NT) cnt[b] = 0;     // (every crop, flagged or not, as sdfr_band_select_ex does)
        return;
    }
    const int b = bid / nblk, blk = nblk - 1 - bid % nblk;
    if (skip && skip[b]) return;                             // this crop keeps its previous selection
    if (thr_extra) thr += thr_extra[b];
    const float* __restrict__ p = sdf + (int64_t)b * G;
    const int64_t r0 = (int64_t)blk * SDFR_BR_ROWS;          // rows in front of this block's (r0 < G)
    // the block's own row first: its load flies while the rows in front are counted
    const int64_t g = r0 + tid;
    const bool in = g < G && sdfr_br_in(p[g], thr);
    // band rows in [0, r0): scalar loads up to the first 16-byte boundary of the crop's rows, 16-byte loads behind it -- SDFR_BR_FLY of them
    // requested before the first is counted, so the 64 000 rows in front of a 40^3 grid's last block are one round trip to memory -- and
    // scalar loads for the up to three rows left in front of r0
    int front = 0;
    int64_t head = (int64_t)((4u - (uint32_t)((uintptr_t)p >> 2)) & 3u);
    if (head > r0) head = r0;
    if (tid < head) front += sdfr_br_in(p[tid], thr);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
    const int nv = (int)((r0 - head) >> 2);                  // (G < 2^31 rows: idx holds them as int32)
    for (int i0 = 0; i0 < nv; i0 += SDFR_BR_NT * SDFR_BR_FLY) {
        float4 q[SDFR_BR_FLY];
#pragma unroll
        for (int u = 0; u < SDFR_BR_FLY; ++u) {
            const int i = i0 + u * SDFR_BR_NT + tid;
            q[u] = p4[i < nv ? i : nv - 1];                  // (beyond the end: the last vector again, not counted)
        }
#pragma unroll
        for (int u = 0; u < SDFR_BR_FLY; ++u) {
            const int c = sdfr_br_in(q[u].x, thr) + sdfr_br_in(q[u].y, thr) + sdfr_br_in(q[u].z, thr) + sdfr_br_in(q[u].w, thr);
            front += i0 + u * SDFR_BR_NT + tid < nv ? c : 0;
        }
    }
    const int64_t tail = head + 4 * (int64_t)nv;
    if (tail + tid < r0) front += sdfr_br_in(p[tail + tid], thr);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) front += __shfl_xor(front, d, 64);
    __shared__ int wfront[SDFR_BR_WAVES];
    __shared__ int wc[SDFR_BR_WAVES];
    const unsigned long long bal = __ballot(in);
    if (lane == 0) {
        wc[wv] = __popcll(bal);
        wfront[wv] = front;
    }
    __syncthreads();
    int base = 0, woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SDFR_BR_WAVES; ++w) {
        const int c = wc[w];
        base += wfront[w];
        woff += w < wv ? c : 0;
        tot += c;
    }
    const int rank = base + woff + __popcll(bal & ((1ull << lane) - 1ull));
    if (g < G) {
        int sl = -1;
        if (in && rank < cap) {
            idx[(int64_t)b * cap + rank] = (int32_t)g;
            sl = rank;
        }
        if (slot) slot[(int64_t)b * G + g] = sl;
    }
    if (blk == nblk - 1 && tid == 0) {
        cnt[b] = base + tot;
        if (over && base + tot > cap) atomicOr(&over[b], over_bit);           // sticky, as in sdfr_band_scatter_kernel
    }
}

// Above this many rows (B G) the redundant count costs more than the launch it replaces: callers keep sdfr_mlp_forward_balanced +
// sdfr_band_select_ex there (profiles/chain_notes.md has the measurements).
#define SDFR_BAND_RANK_MAX_ROWS ((int64_t)256000)
extern "C" int64_t sdfr_band_select_rank_max_rows(void) { return SDFR_BAND_RANK_MAX_ROWS; }

extern "C" int sdfr_band_select_rank(const float* sdf, int64_t G, int B, float thr, const float* thr_extra, const int32_t* skip, int32_t* idx,
                                     int cap, int32_t* cnt, int32_t* slot, int32_t* over, int over_bit, void* balance_state, int64_t order_rows,
                                     void* stream) {
    SDFR_REQUIRE(sdf && idx && cnt, "sdfr_band_select_rank: NULL argument");
    SDFR_REQUIRE(G >= 0 && B >= 0 && cap >= 0, "sdfr_band_select_rank: negative size");
    SDFR_REQUIRE(!balance_state || (order_rows > 0 && order_rows < (int64_t)1 << 31), "sdfr_band_select_rank: order_rows=%lld out of range",
                 (long long)order_rows);
    const int64_t nblk = G > 0 ? (G + SDFR_BR_ROWS - 1) / SDFR_BR_ROWS : 1;
    const int64_t nsel = B == 0 ? 0 : (G > 0 ? nblk * B : 1);
    // (orders of more than SDFR_TB_MAX_CHUNKS chunks are not ranked: sdfr_mlp_forward_balanced_deferred launches them in the static order)
    const int nrank = balance_state && sdfr_tb_ranked(order_rows) ? sdfr_tb_rank_blocks(order_rows, SDFR_BR_NT) : 0;
    SDFR_REQUIRE(nsel + nrank < (int64_t)1 << 31, "sdfr_band_select_rank: G=%lld rows of B=%d crops exceed one launch", (long long)G, B);
    if (nsel + nrank == 0) return SDFR_OK;
    hipLaunchKernelGGL(sdfr_band_rank_kernel, dim3((unsigned)(nsel + nrank)), dim3(SDFR_BR_NT), 0, (hipStream_t)stream, sdf, G, B, thr, thr_extra, skip,
                       idx, cap, cnt, slot, over, over_bit, (int)nblk, (int)nsel, (int32_t*)balance_state, order_rows, nrank);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
