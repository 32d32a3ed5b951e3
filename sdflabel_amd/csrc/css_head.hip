// The output head of the CSS network on the device (gfx950): networks/resnet_css.py:194-196 and :203-249 of the reference.
//
// sdfr_css_head    three 1x1 convolutions 64 -> 256 (out_u / out_v / out_w) and one 64 -> 2 (out_mask) with everything the reference derives from
//                  them per pixel: log_softmax, softmax(100 .), the expected colour sum_k k p_k, the soft mask, the arg-max mask and the masked
//                  product.  A 64 -> 768 GEMM with a per-pixel reduction epilogue: nothing 256 channels wide is written unless the caller asks
//                  for the log-probabilities.
//                    - Logits: css_logits_tile of css_tile.h (exact-f32 MFMA, k in order, bias last; a wave owns 32 pixels and all 256
//                      classes, pixel p's logits sit in lanes p and p + 32), the function the training kernels of css_train.hip call too.
//                      Every reduction is over a lane's registers in a fixed order plus one exchange with lane ^ 32.
//                    - softmax(100 log_softmax(u)) == softmax(100 u): the colour path never forms the log-softmax.  The maximum is subtracted
//                      first, exp runs in float32 (expf), the two sums accumulate in float64 (k e is exact there) in class order.
//                      A class whose 100 (logit - max) is below -104 in all 64 lanes is skipped: expf returns exactly 0 there.
//                    - Every head's workgroups compute the two mask logits of their own pixels (fmaf chain over k, bias last); head 0 writes them.
//                    - No atomics; a pixel's result depends on its own 4 x 64 features and the weights only: not on B, the tile or the launch.
// sdfr_css_latent  out_lat (1x1 conv 256 -> 3) on x4, the mean over the pixels and the projection onto the unit sphere; one workgroup per crop.
// Compiled with -ffp-contract=off: the fused operations are the explicit fmaf / MFMA chains only.
#include "css_tile.h"

#define CH_SKIP (-104.0f)          // expf(x) == 0 for x < -103.98 (below half the smallest subnormal)
#define CH_HARD 100.0f             // sm_hardness of the reference

struct CssHeadArgs {
    const float* x[3];             // x_u, x_v, x_w [B][64][HW]
    const float* xm;               // x_mask
    const float* w[3];             // [256][64]
    const float* b[3];             // [256]
    const float* wm;               // [2][64]
    const float* bm;               // [2]
    float* uvw_sm;                 // [B][3][HW]
    float* uvw_sm_masked;          // [B][3][HW]
    float* mask;                   // [B][2][HW]
    float* mask_sm;                // [B][1][HW]
    float* lp[3];                  // u, v, w [B][256][HW] or NULL
    int HW, tiles_per_crop;
    int64_t n_tiles;               // B * tiles_per_crop
};

__global__ __launch_bounds__(256, 2) void sdfr_css_head_kernel(CssHeadArgs A) {
    extern __shared__ float smem[];
    float* wT = smem;                              // [64][CSS_LD]
    float* bs = smem + CSS_K * CSS_LD;             // [256] bias, then [128] mask weights, [2] mask bias
    float* wms = bs + CSS_N;
    const int head = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, h = lane >> 5;

    css_stage_weights<CSS_N>(A.w[head], A.b[head], wT, bs, tid);
    if (tid < 2 * CSS_K) wms[tid] = A.wm[tid];
    if (tid < 2) wms[2 * CSS_K + tid] = A.bm[tid];
    __syncthreads();

    const int HW = A.HW;
    for (int64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const CssLane L = css_tile_lane(tile, A.tiles_per_crop, HW, wave, col);
        if (L.wave_past_crop) continue;
        const int b = L.b, pix = L.pix, p = L.p;
        const bool live = L.live;

        // ---- B operands: x[b][2 s + h][pix], one register per MFMA step, fetched 8 steps ahead of their use: before the mask chain
        const float* xh = A.x[head] + ((int64_t)b * CSS_K + h) * HW + p;
        float xb[8];
        css_prefetch8(xh, HW, live, xb);

        // ---- the mask logit of row h for this pixel (both halves of the wave work: row 0 in lanes 0-31, row 1 in lanes 32-63)
        float mh = 0.f;
        {
            const float* xm = A.xm + (int64_t)b * CSS_K * HW + p;
            const float* wr = wms + h * CSS_K;
#pragma unroll 16
            for (int k = 0; k < CSS_K; ++k) mh = fmaf(wr[k], xm[(int64_t)k * HW], mh);
            mh = mh + wms[2 * CSS_K + h];
        }
        const float mo = __shfl_xor(mh, 32);
        const float m0 = h ? mo : mh, m1 = h ? mh : mo;

        // ---- logits: 8 tiles of 32 classes x 32 pixels, k in order, bias last, and the per-pixel maximum
        f32x16 acc[8];
        const float mx = css_logits_tile(wT, bs, xh, HW, live, col, h, xb, acc);

        // ---- expected colour: sum k e / sum e, e = exp(100 (logit - max)); float64 sums, classes in register order, half 0 before half 1
        double se = 0.0, sk = 0.0;
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = CH_HARD * (acc[t][r] - mx);
                if (__builtin_amdgcn_ballot_w64(a >= CH_SKIP) != 0ull) {
                    const double e = (double)expf(a);
                    se += e;
                    sk = fma((double)CSS_CLASS(t, r, 0), e, sk);          // the half's 4 h is added once below
                }
            }
        sk = fma((double)(4 * h), se, sk);
        const double S = css_pair_sum(se, h), N = css_pair_sum(sk, h);
        const float colour = (float)(N / S);

        // ---- mask: raw logits, softmax(100 .)[1], arg-max (a tie is class 0)
        const float mm = fmaxf(m0, m1);
        const float e0 = expf(CH_HARD * (m0 - mm)), e1 = expf(CH_HARD * (m1 - mm));
        const float msm = e1 / (e0 + e1);
        const float fg = m1 > m0 ? 1.f : 0.f;

        if (live && h == 0) {
            const int64_t o = ((int64_t)b * 3 + head) * HW + pix;
            A.uvw_sm[o] = colour;
            A.uvw_sm_masked[o] = colour * fg;
            if (head == 0) {
                A.mask[((int64_t)b * 2) * HW + pix] = m0;
                A.mask[((int64_t)b * 2 + 1) * HW + pix] = m1;
                A.mask_sm[(int64_t)b * HW + pix] = msm;
            }
        }

        // ---- optional log-probabilities: logit - max - log(sum exp(logit - max))
        float* lp = A.lp[head];
        if (lp != nullptr) {
            double s1 = 0.0;
#pragma unroll
            for (int t = 0; t < 8; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) s1 += (double)expf(acc[t][r] - mx);
            const float lse = (float)log(css_pair_sum(s1, h));
            if (live) {
                float* d = lp + ((int64_t)b * CSS_N + 4 * h) * HW + pix;
#pragma unroll
                for (int t = 0; t < 8; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) d[(int64_t)CSS_CLASS(t, r, 0) * HW] = (acc[t][r] - mx) - lse;
            }
        }
    }
}

// ---- latent head ---------------------------------------------------------------------------------------------------------------------------
#define CL_K 256
__global__ __launch_bounds__(256) void sdfr_css_latent_kernel(const float* __restrict__ x4, const float* __restrict__ w, const float* __restrict__ bias,
                                                              int hw, float* __restrict__ out) {
    __shared__ float ws[3 * CL_K];
    __shared__ float red[3][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < 3 * CL_K; i += 256) ws[i] = w[i];
    __syncthreads();
    // thread t: the 1x1 conv of pixels t, t + 256, ... (k in order, bias last), summed in that order
    float s[3] = {0.f, 0.f, 0.f};
    const float* xb = x4 + (int64_t)b * CL_K * hw;
    for (int p = tid; p < hw; p += 256) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll 8
        for (int k = 0; k < CL_K; ++k) {
            const float v = xb[(int64_t)k * hw + p];
            a0 = fmaf(ws[k], v, a0);
            a1 = fmaf(ws[CL_K + k], v, a1);
            a2 = fmaf(ws[2 * CL_K + k], v, a2);
        }
        s[0] += a0 + bias[0];
        s[1] += a1 + bias[1];
        s[2] += a2 + bias[2];
    }
    for (int c = 0; c < 3; ++c) red[c][tid] = s[c];
    css_tree_sum256<3>(&red[0][0], tid);
    if (tid == 0) {
        const float v0 = red[0][0] / (float)hw, v1 = red[1][0] / (float)hw, v2 = red[2][0] / (float)hw;
        const float len = sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
        const float f = 1.0f / (len + 1e-8f);
        out[3 * b] = v0 * f;
        out[3 * b + 1] = v1 * f;
        out[3 * b + 2] = v2 * f;
    }
}

extern "C" int sdfr_css_head(const float* x_u, const float* x_v, const float* x_w, const float* x_mask, int B, int C, int H, int W,
                             const float* w_u, const float* b_u, const float* w_v, const float* b_v, const float* w_w, const float* b_w,
                             const float* w_mask, const float* b_mask, float* uvw_sm, float* uvw_sm_masked, float* mask, float* mask_sm,
                             float* u, float* v, float* w, void* stream) {
    SDFR_REQUIRE(B >= 0 && H >= 0 && W >= 0, "sdfr_css_head: negative size");
    SDFR_REQUIRE(C == CSS_K, "sdfr_css_head: the head takes %d feature channels (got %d)", CSS_K, C);
    SDFR_REQUIRE((int64_t)H * W < (1ll << 30), "sdfr_css_head: H * W = %lld is beyond 2^30", (long long)H * W);
    if (B == 0 || H == 0 || W == 0) return SDFR_OK;
    SDFR_REQUIRE(x_u && x_v && x_w && x_mask && w_u && b_u && w_v && b_v && w_w && b_w && w_mask && b_mask, "sdfr_css_head: NULL input");
    SDFR_REQUIRE(uvw_sm && uvw_sm_masked && mask && mask_sm, "sdfr_css_head: NULL output");
    SDFR_REQUIRE((u != nullptr) == (v != nullptr) && (u != nullptr) == (w != nullptr), "sdfr_css_head: u, v, w are given together or not at all");
    if (int rc = css_device_check(x_u, "sdfr_css_head")) return rc;
    CssHeadArgs A;
    A.x[0] = x_u; A.x[1] = x_v; A.x[2] = x_w; A.xm = x_mask;
    A.w[0] = w_u; A.w[1] = w_v; A.w[2] = w_w; A.b[0] = b_u; A.b[1] = b_v; A.b[2] = b_w;
    A.wm = w_mask; A.bm = b_mask;
    A.uvw_sm = uvw_sm; A.uvw_sm_masked = uvw_sm_masked; A.mask = mask; A.mask_sm = mask_sm;
    A.lp[0] = u; A.lp[1] = v; A.lp[2] = w;
    A.HW = H * W;
    A.tiles_per_crop = sdfr_cdiv(A.HW, CSS_TILE);
    A.n_tiles = (int64_t)B * A.tiles_per_crop;
    // two workgroups fit a CU (64 KB of LDS each); three heads share the device, so each gets a third of the slots and walks its tiles
    int dev = 0, cus = 0;
    SDFR_HIP_CHECK(hipGetDevice(&dev));
    SDFR_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    int64_t gx = (int64_t)(cus > 0 ? cus : 256) * 2 / 3;
    if (gx < 1) gx = 1;
    if (gx > A.n_tiles) gx = A.n_tiles;
    const size_t lds = (size_t)(CSS_K * CSS_LD + CSS_N + 2 * CSS_K + 2) * sizeof(float);
    // (more than 64 KB of dynamic LDS needs the attribute; it belongs to the current device's image of the kernel, so it is set at every call)
    SDFR_HIP_CHECK(hipFuncSetAttribute((const void*)sdfr_css_head_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(sdfr_css_head_kernel, dim3((unsigned)gx, 3), dim3(256), lds, (hipStream_t)stream, A);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_css_latent(const float* x4, int B, int C, int h, int w, const float* w_lat, const float* b_lat, float* latent, void* stream) {
    SDFR_REQUIRE(B >= 0 && h >= 0 && w >= 0, "sdfr_css_latent: negative size");
    SDFR_REQUIRE(C == CL_K, "sdfr_css_latent: out_lat takes %d feature channels (got %d)", CL_K, C);
    SDFR_REQUIRE((int64_t)h * w < (1ll << 22), "sdfr_css_latent: h * w = %lld is beyond 2^22", (long long)h * w);
    if (B == 0 || h == 0 || w == 0) return SDFR_OK;
    SDFR_REQUIRE(x4 && w_lat && b_lat && latent, "sdfr_css_latent: NULL argument");
    if (int rc = css_device_check(x4, "sdfr_css_latent")) return rc;
    hipLaunchKernelGGL(sdfr_css_latent_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x4, w_lat, b_lat, h * w, latent);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
