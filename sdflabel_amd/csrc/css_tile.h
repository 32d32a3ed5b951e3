// The logits tile of the CSS head (gfx950), stated once for css_head.hip (inference) and css_train.hip (losses and backward).
//
// A workgroup of 4 waves works on 128 consecutive pixels of one crop; a wave owns 32 pixels and all 256 classes of one colour head: 8
// accumulator tiles of v_mfma_f32_32x32x2_f32, A = the head's weights from the LDS image W^T [k][class], B = the features straight from
// global memory (NCHW: a k-row of 32 pixels is one 128-byte line).  k runs 0 ... 63 in order from a zero accumulator for every class and
// every pixel and the bias is added last: an fmaf chain, bit for bit.  Pixel p's logits sit in lanes p and p + 32 (lane half h), 128
// registers each, so every reduction over the classes is over a lane's registers in a fixed order plus one exchange with lane ^ 32.
// The training gradients are right only if css_loss_fwd_kernel sees the logits sdfr_css_head_kernel computes: both call css_logits_tile.
#pragma once
#include "sdfr_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CSS_K 64                   // input channels of the head
#define CSS_N 256                  // classes per colour head
#define CSS_LD (CSS_N + 1)         // row pitch in dwords of the LDS image W^T [k][class] (257: the transposing store is conflict free)
#define CSS_TILE 128               // pixels per workgroup pass: 4 waves x 32

// row of accumulator register r in lane half h (C/D map of the 32x32 MFMA), and the class of register r of tile t
#define CSS_ROW(r, h) (((r) & 3) + 8 * ((r) >> 2) + 4 * (h))
#define CSS_CLASS(t, r, h) (32 * (t) + CSS_ROW(r, h))

// NC classes' weights w [NC][64], transposed into the LDS image wT [k][class] at pitch NC + 1, and their bias: thread reads
// w[c][4 q ... 4 q + 3] (coalesced), writes wT[4 q + i][c].  256 threads; the caller synchronises.
template <int NC>
__device__ __forceinline__ void css_stage_weights(const float* w, const float* bias, float* wT, float* bs, int tid) {
    const float4* W4 = reinterpret_cast<const float4*>(w);
    for (int i = tid; i < NC * CSS_K / 4; i += 256) {
        const float4 v = W4[i];
        const int c = i >> 4, k = (i & 15) * 4;
        wT[(k + 0) * (NC + 1) + c] = v.x;
        wT[(k + 1) * (NC + 1) + c] = v.y;
        wT[(k + 2) * (NC + 1) + c] = v.z;
        wT[(k + 3) * (NC + 1) + c] = v.w;
    }
    if (tid < NC) bs[tid] = bias[tid];
}

// where a lane stands in a tile.  Tiles never cross a crop, so a pixel's tile, wave and lane depend on its index inside the crop only.
struct CssLane {
    int b, pix, p;                 // crop, pixel of the crop, the pixel to read: a dead lane reads pixel 0 and stores nothing
    bool live;                     // pix < HW
    bool wave_past_crop;           // wave-uniform: all 32 pixels of the wave are past the crop.  Not for control flow around a barrier.
};
__device__ __forceinline__ CssLane css_tile_lane(int64_t tile, int tiles_per_crop, int HW, int wave, int col) {
    CssLane L;
    const int first = (int)(tile % tiles_per_crop) * CSS_TILE + wave * 32;
    L.b = (int)(tile / tiles_per_crop);
    L.pix = first + col;
    L.live = L.pix < HW;
    L.wave_past_crop = first >= HW;
    L.p = L.live ? L.pix : 0;
    return L;
}

// the B operands of the first 8 MFMA steps, xh = x + ((int64_t)b * 64 + h) * HW + p: step s takes x[b][2 s + h][p].  Apart from the logits,
// so that a caller can put independent work between the loads and their use.
__device__ __forceinline__ void css_prefetch8(const float* xh, int HW, bool live, float (&xb)[8]) {
#pragma unroll
    for (int s = 0; s < 8; ++s) xb[s] = live ? xh[(int64_t)(2 * s) * HW] : 0.f;
}

// the logits of the lane's pixel: acc[t][r] = z[CSS_CLASS(t, r, h)], k in order, every group's 8 operands fetched a group ahead of their
// use (xb: css_prefetch8), bias last.  Returns the pixel's maximum over the 256 classes.
__device__ __forceinline__ float css_logits_tile(const float* wT, const float* bs, const float* xh, int HW, bool live, int col, int h,
                                                 float (&xb)[8], f32x16 (&acc)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const float* wa = wT + h * CSS_LD + col;
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
        float xn[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) xn[s] = (live && g < 3) ? xh[(int64_t)(2 * (8 * (g + 1) + s)) * HW] : 0.f;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
#pragma unroll
            for (int t = 0; t < 8; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[2 * (8 * g + s) * CSS_LD + 32 * t], xb[s], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) xb[s] = xn[s];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[t][r] = acc[t][r] + bs[CSS_CLASS(t, r, h)];
            mx = fmaxf(mx, acc[t][r]);
        }
    return fmaxf(mx, __shfl_xor(mx, 32));
}

// a pixel's sum over both lane halves: half 0's term first, then half 1's, whichever half the lane is in
template <typename T>
__device__ __forceinline__ T css_pair_sum(T s, int h) {
    const T o = __shfl_xor(s, 32);
    return h ? o + s : s + o;
}

// 256 threads sum NA arrays red[a][256] in LDS to red[a][0] on a fixed tree (n = 128, 64, ... 1): the same order whatever the launch.
// The caller has stored its terms; the sums are visible to every thread on return.
template <int NA, typename T>
__device__ __forceinline__ void css_tree_sum256(T* red, int tid) {
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if (tid < n)
            for (int a = 0; a < NA; ++a) red[a * 256 + tid] += red[a * 256 + tid + n];
        __syncthreads();
    }
}

// the launch dereferences the caller's pointers from the stream of the CURRENT device: refuse a call whose data lives elsewhere, as the decoder
// launches do for their weight images
static inline int css_device_check(const void* p, const char* what) {
    int cur = -1;
    SDFR_HIP_CHECK(hipGetDevice(&cur));
    hipPointerAttribute_t at;
    SDFR_HIP_CHECK(hipPointerGetAttributes(&at, p));
    SDFR_REQUIRE(at.device == cur, "%s: the tensors live on device %d but the current device (the launch stream's) is %d", what, at.device, cur);
    return SDFR_OK;
}
