// Training the CSS network's output head on the device (gfx950): the losses of pipelines/train_css.py:71-80 of the reference and their
// gradients for unit upstream gradient, without anything 256 channels wide in global memory.
//
// With N = B H W, m the ground-truth mask, t = uvw_gt * m and z = W x + b (per colour head):
//   loss = (1/N) [ sum_{m=1} (logsumexp(z) - z[t]) + (N - n_fg) ln 256 ]        dloss/dz = m (softmax(z) - onehot(t)) / N
//   loss_mask = 2 CE(z_mask, m),  dloss/dz_mask = 2 (softmax(z_mask) - onehot(m)) / N
//   loss_latent = mean((lat - gt)^2), lat = v / (|v| + 1e-8) with the length DETACHED as in the reference: dlat/dv = 1 / (|v| + 1e-8)
//
// sdfr_css_head_loss   four launches on one stream:
//   css_loss_fwd_kernel   css_logits_tile of css_tile.h, the function sdfr_css_head_kernel calls (a wave owns 32 pixels x 256 classes, 8
//                         accumulator tiles of v_mfma_f32_32x32x2_f32, k in order, bias last, the per-pixel maximum): the inference path's
//                         logits by construction.  Then log-sum-exp and target logit (compare against the class number of each register),
//                         g = m (exp(z - lse) - onehot) / N over the accumulators, then
//                         dX[k][pix] = sum_c W[c][k] g[c][pix]: accumulator register r of tile t IS the B operand (its two k-slots are the
//                         classes of lane halves 0 and 1), the A operand W[class][32 mt + col] comes from the same LDS image W^T [k][class] the
//                         logits read (css_stage_weights): at pitch 257 the 32 lanes of a ds_read_b32 group hit 32 banks.  The per-pixel lse
//                         (4 bytes per pixel and head) goes to the workspace; loss sums are float64 per workgroup.
//   css_loss_dw_kernel    dW[c][k] = sum_pix g[c][pix] x[k][pix] needs the pixels in the reduction slot: a second pass recomputes the logits
//                         TRANSPOSED (css_logits_tile's MFMA with A and B swapped: the same products in the same order) from the stored lse,
//                         so that a lane owns a class and its registers are pixels; that register is the A operand of the dW MFMA, the B operand
//                         x[k][pix] comes from an LDS copy of the wave's 64 x 32 feature tile.  A workgroup owns half the classes (128
//                         accumulator registers per wave), walks its tiles, sums its four waves in order and writes ONE partial dW / db.
//   css_loss_mask_kernel  the 64 -> 2 mask head on fmaf chains, a thread per pixel; its dW through an LDS copy of the tile.
//   css_loss_reduce_kernel sums the workgroups' partials in workgroup order.
// The partials' size depends on the (fixed) grid only.  No atomics: every output has the same bits in every run.
// sdfr_css_latent_loss  one workgroup per crop, then a reduction over the crops in order.
// Compiled with -ffp-contract=off: the fused operations are the explicit fmaf / MFMA chains only.
#include "css_tile.h"

#define CT_NH (CSS_N / 2)           // classes of a dW workgroup; its LDS image W^T [k][class] has pitch CT_NH + 1
#define CT_LDH (CT_NH + 1)
#define CT_XP 33                   // pitch of a wave's feature tile [k][32 pixels] in LDS
#define CT_GX 80                   // workgroups per colour head (fixed: the partials' size and the summation order do not depend on the device)
#define CT_MTILE 256               // pixels per pass of the mask kernel
#define CT_MLD (CT_MTILE + 1)      // pitch of its feature tile [k][256 pixels] in LDS
#define CT_MGX 128                 // workgroups of the mask kernel
#define CT_LN256 5.5451774444795624753

// workspace layout (bytes): doubles first
//   double part_loss[3][CT_GX][2]   (sum over foreground pixels of lse - z[t], number of foreground pixels)
//   double part_lossm[CT_MGX]
//   float  part_dw[3][CT_GX][2][128][64], part_db[3][CT_GX][256], part_dwm[CT_MGX][128], part_dbm[CT_MGX][2]
//   float  lse[3][N]
#define CT_WS_DOUBLES (3 * CT_GX * 2 + CT_MGX)
#define CT_WS_FLOATS ((int64_t)3 * CT_GX * CSS_N * CSS_K + 3 * CT_GX * CSS_N + CT_MGX * 2 * CSS_K + CT_MGX * 2)
#define CT_WS_FIXED ((int64_t)CT_WS_DOUBLES * 8 + CT_WS_FLOATS * 4)
static_assert(CT_WS_FIXED == SDFR_CSS_LOSS_WS_FIXED, "include/sdfr.h publishes the size of this layout: change both together");

struct CssLossArgs {
    const float* x[3];             // x_u, x_v, x_w [B][64][HW]
    const float* w[3];             // [256][64]
    const float* b[3];             // [256]
    const uint8_t* uvw;            // [B][3][HW]
    const uint8_t* mask;           // [B][HW]
    float* dx[3];                  // [B][64][HW]
    float* lse;                    // [3][N]
    double* part_loss;             // [3][gridDim.x][2]
    float* part_dw;                // [3][gridDim.x][2][128][64]
    float* part_db;                // [3][gridDim.x][256]
    int HW, tiles_per_crop;
    int64_t n_tiles, N;
    float invN;
};

__global__ __launch_bounds__(256, 2) void css_loss_fwd_kernel(CssLossArgs A) {
    extern __shared__ __align__(16) float smem[];
    float* wT = smem;                              // [64][CSS_LD]
    float* bs = smem + CSS_K * CSS_LD;             // [256] bias
    const int head = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, h = lane >> 5;
    css_stage_weights<CSS_N>(A.w[head], A.b[head], wT, bs, tid);
    __syncthreads();

    const int HW = A.HW;
    double lsum = 0.0, nfg = 0.0;
    for (int64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const CssLane L = css_tile_lane(tile, A.tiles_per_crop, HW, wave, col);
        if (L.wave_past_crop) continue;
        const int b = L.b, pix = L.pix, p = L.p;
        const bool live = L.live;

        const float* xh = A.x[head] + ((int64_t)b * CSS_K + h) * HW + p;
        float xb[8];
        css_prefetch8(xh, HW, live, xb);
        const bool m = live && A.mask[(int64_t)b * HW + p] != 0;
        const int tg = m ? (int)A.uvw[((int64_t)b * 3 + head) * HW + p] : 0;

        // ---- logits: the function of the inference path (8 tiles of 32 classes x 32 pixels, k in order, bias last) and the maximum
        f32x16 acc[8];
        const float mx = css_logits_tile(wT, bs, xh, HW, live, col, h, xb, acc);

        // ---- log-sum-exp (float64 sum, classes in register order, half 0 before half 1) and the target logit
        double s1 = 0.0;
        float zt = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s1 += (double)expf(acc[t][r] - mx);
                zt = (CSS_CLASS(t, r, h) == tg) ? acc[t][r] : zt;
            }
        const float lse = mx + (float)log(css_pair_sum(s1, h));
        const float zt_o = __shfl_xor(zt, 32);
        const float ztf = (((tg >> 2) & 1) == h) ? zt : zt_o;
        if (m && h == 0) {
            lsum += (double)lse - (double)ztf;
            nfg += 1.0;
        }
        if (live && h == 0) A.lse[(int64_t)head * A.N + (int64_t)b * HW + pix] = lse;

        // ---- g = m (softmax - onehot) / N over the accumulators; exactly 0 at background pixels
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pr = expf(acc[t][r] - lse);
                const float oh = (CSS_CLASS(t, r, h) == tg) ? 1.f : 0.f;
                acc[t][r] = m ? (pr - oh) * A.invN : 0.f;
            }

        // ---- dX[k][pix] = sum_c W[c][k] g[c][pix]: B = the accumulator register, A = W[class of (t, r, half)][32 mt + col]
        f32x16 dxa[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dxa[mt][r] = 0.f;
        const float* wd = wT + col * CSS_LD + 4 * h;
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    dxa[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wd[32 * mt * CSS_LD + CSS_CLASS(t, r, 0)], acc[t][r], dxa[mt], 0, 0, 0);
            }
        if (live) {
            float* d = A.dx[head] + ((int64_t)b * CSS_K + 4 * h) * HW + pix;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) d[(int64_t)(32 * mt + CSS_ROW(r, 0)) * HW] = dxa[mt][r];
        }
    }

    // ---- the workgroup's loss sums: a fixed tree
    __syncthreads();
    double* red = reinterpret_cast<double*>(smem);
    red[tid] = lsum;
    red[256 + tid] = nfg;
    css_tree_sum256<2>(red, tid);
    if (tid == 0) {
        double* o = A.part_loss + ((int64_t)head * gridDim.x + blockIdx.x) * 2;
        o[0] = red[0];
        o[1] = red[256];
    }
}

// dW / db of half the classes of one colour head: blockIdx = (workgroup, head, class half)
__global__ __launch_bounds__(256, 2) void css_loss_dw_kernel(CssLossArgs A) {
    extern __shared__ __align__(16) float smem[];
    float* wT = smem;                              // [64][CT_LDH]: W^T of the workgroup's 128 classes
    float* bs = wT + CSS_K * CT_LDH;               // [128]
    float* xs = bs + 128;                          // [4 waves][64][CT_XP]
    float* pl = xs + 4 * CSS_K * CT_XP;            // [4][32] lse, then [4][32] scale, then [4][32] target (int)
    float* ps = pl + 128;
    int* pt = reinterpret_cast<int*>(ps + 128);
    const int head = blockIdx.y, zh = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, h = lane >> 5;
    css_stage_weights<CT_NH>(A.w[head] + zh * CT_NH * CSS_K, A.b[head] + zh * CT_NH, wT, bs, tid);      // (the loop's first barrier follows)
    const int HW = A.HW;
    f32x16 dw[4][2];
    float dbacc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        dbacc[t] = 0.f;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dw[t][nt][r] = 0.f;
    }
    float* xsw = xs + wave * CSS_K * CT_XP;
    for (int64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {                 // the same trips for every wave: barriers inside
        const CssLane L = css_tile_lane(tile, A.tiles_per_crop, HW, wave, col);            // (no early-out on L.wave_past_crop: barriers)
        const int b = L.b, p = L.p;
        const bool live = L.live;
        __syncthreads();                                                                   // the previous tile's LDS reads are done
        {
            const float* xh = A.x[head] + ((int64_t)b * CSS_K + h) * HW + p;
#pragma unroll 8
            for (int s = 0; s < 32; ++s) xsw[(2 * s + h) * CT_XP + col] = live ? xh[(int64_t)(2 * s) * HW] : 0.f;
            if (h == 0) {
                const bool m = live && A.mask[(int64_t)b * HW + p] != 0;
                pl[wave * 32 + col] = live ? A.lse[(int64_t)head * A.N + (int64_t)b * HW + p] : 0.f;
                ps[wave * 32 + col] = m ? A.invN : 0.f;
                pt[wave * 32 + col] = m ? (int)A.uvw[((int64_t)b * 3 + head) * HW + p] : -1;
            }
        }
        __syncthreads();
        const float* plw = pl + wave * 32 + 4 * h;                                         // per-pixel data of register r: index CSS_ROW(r, 0)
        const float* psw = ps + wave * 32 + 4 * h;
        const int* ptw = pt + wave * 32 + 4 * h;
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) any = any || psw[CSS_ROW(r, 0)] != 0.f;
        if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue;                            // no foreground pixel in the wave's 32: g is all zero
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            // transposed logits: rows = pixels, columns = the lane's class; the forward's products in the forward's order
            f32x16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = 0.f;
#pragma unroll 8
            for (int s = 0; s < 32; ++s)
                z = __builtin_amdgcn_mfma_f32_32x32x2f32(xsw[(2 * s + h) * CT_XP + col], wT[(2 * s + h) * CT_LDH + 32 * t + col], z, 0, 0, 0);
            const float bias = bs[32 * t + col];
            const int cls = zh * 128 + 32 * t + col;
            float dbs = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pr = expf((z[r] + bias) - plw[CSS_ROW(r, 0)]);
                const float g = (pr - (ptw[CSS_ROW(r, 0)] == cls ? 1.f : 0.f)) * psw[CSS_ROW(r, 0)];
                z[r] = g;
                dbs += g;
            }
            dbacc[t] += css_pair_sum(dbs, h);
            // dW[class][k] += sum over the 32 pixels: A = g (lane = class, slots = pixels ROW(r, 0 / 1)), B = x[32 nt + col][that pixel]
#pragma unroll
            for (int r = 0; r < 16; ++r) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    dw[t][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(z[r], xsw[(32 * nt + col) * CT_XP + CSS_ROW(r, h)], dw[t][nt], 0, 0, 0);
            }
        }
    }

    // ---- the four waves in order, through LDS (32 KB a wave: the weights and tiles are no longer needed)
    for (int w = 1; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) smem[((t * 2 + nt) * 16 + r) * 64 + lane] = dw[t][nt][r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) dw[t][nt][r] += smem[((t * 2 + nt) * 16 + r) * 64 + lane];
        }
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) smem[wave * 128 + 32 * t + col] = dbacc[t];
    }
    __syncthreads();
    const int64_t blk = (int64_t)head * gridDim.x + blockIdx.x;
    if (wave == 0) {
        float* o = A.part_dw + (blk * 2 + zh) * 128 * CSS_K;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[(32 * t + CSS_ROW(r, h)) * CSS_K + 32 * nt + col] = dw[t][nt][r];
    }
    if (tid < 128) A.part_db[blk * CSS_N + zh * 128 + tid] = ((smem[tid] + smem[128 + tid]) + smem[256 + tid]) + smem[384 + tid];
}

// ---- mask head: 64 -> 2 on fmaf chains, a thread per pixel ------------------------------------------------------------------------------------
struct CssMaskLossArgs {
    const float* xm;               // [B][64][HW]
    const float* wm;               // [2][64]
    const float* bm;               // [2]
    const uint8_t* mask;           // [B][HW]
    float* dxm;                    // [B][64][HW]
    double* part_loss;             // [gridDim.x]
    float* part_dw;                // [gridDim.x][128]
    float* part_db;                // [gridDim.x][2]
    int HW, tiles_per_crop;
    int64_t n_tiles;
    float invN;
};

__global__ __launch_bounds__(256) void css_loss_mask_kernel(CssMaskLossArgs A) {
    extern __shared__ __align__(16) float smem[];
    float* xs = smem;                              // [64][CT_MLD]: the tile's features, [k][pixel]
    float* gs = xs + CSS_K * CT_MLD;               // [2][256]: the tile's logit gradients
    float* ws = gs + 2 * CT_MTILE;                 // [128] weights, [2] bias
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 2 * CSS_K) ws[tid] = A.wm[tid];
    if (tid < 2) ws[2 * CSS_K + tid] = A.bm[tid];
    __syncthreads();
    const int HW = A.HW;
    const int half = tid >> 7, c = (tid >> 6) & 1, k = tid & 63;       // the dW role of the thread: pixels 128 half ... + 127 of the tile
    double lsum = 0.0;
    float dwa = 0.f, dba = 0.f;
    for (int64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const int b = (int)(tile / A.tiles_per_crop);
        const int pix = (int)(tile % A.tiles_per_crop) * CT_MTILE + tid;
        const bool live = pix < HW;
        const int p = live ? pix : 0;
        __syncthreads();
        const float* xm = A.xm + (int64_t)b * CSS_K * HW + p;
        float m0 = 0.f, m1 = 0.f;
#pragma unroll 16
        for (int j = 0; j < CSS_K; ++j) {
            const float v = live ? xm[(int64_t)j * HW] : 0.f;
            xs[j * CT_MLD + tid] = v;
            m0 = fmaf(ws[j], v, m0);
            m1 = fmaf(ws[CSS_K + j], v, m1);
        }
        m0 = m0 + ws[2 * CSS_K];
        m1 = m1 + ws[2 * CSS_K + 1];
        const bool fg = live && A.mask[(int64_t)b * HW + p] != 0;
        const float mm = fmaxf(m0, m1);
        const float e0 = expf(m0 - mm), e1 = expf(m1 - mm), S = e0 + e1;
        if (live) lsum += ((double)mm + (double)logf(S)) - (double)(fg ? m1 : m0);
        const float sc = live ? 2.f * A.invN : 0.f;
        const float g0 = (e0 / S - (fg ? 0.f : 1.f)) * sc, g1 = (e1 / S - (fg ? 1.f : 0.f)) * sc;
        gs[tid] = g0;
        gs[CT_MTILE + tid] = g1;
        if (live) {
            float* d = A.dxm + (int64_t)b * CSS_K * HW + pix;
#pragma unroll 16
            for (int j = 0; j < CSS_K; ++j) d[(int64_t)j * HW] = fmaf(ws[CSS_K + j], g1, ws[j] * g0);
        }
        __syncthreads();
        const float* gp = gs + c * CT_MTILE + half * 128;
        const float* xp = xs + k * CT_MLD + half * 128;
#pragma unroll 16
        for (int i = 0; i < 128; ++i) dwa = fmaf(gp[i], xp[i], dwa);
        if (wave < 2) {                                                // db of class `wave`: four strided terms, then a fixed shuffle tree
            const float* gw = gs + wave * CT_MTILE;
            float v = ((gw[lane] + gw[64 + lane]) + gw[128 + lane]) + gw[192 + lane];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            dba += v;
        }
    }
    __syncthreads();
    double* red = reinterpret_cast<double*>(smem);                      // [256] doubles, then the dW halves behind them
    float* dwh = smem + 512;
    red[tid] = lsum;
    dwh[tid] = dwa;
    css_tree_sum256<1>(red, tid);
    if (tid == 0) A.part_loss[blockIdx.x] = red[0];
    if (tid < 128) A.part_dw[(int64_t)blockIdx.x * 128 + tid] = dwh[tid] + dwh[128 + tid];
    if (wave < 2 && lane == 0) A.part_db[(int64_t)blockIdx.x * 2 + wave] = dba;
}

struct CssReduceArgs {
    const double* part_loss;       // [3][gx][2]
    const double* part_lossm;      // [gm]
    const float* part_dw;          // [3][gx][256][64] (as [2][128][64] halves)
    const float* part_db;          // [3][gx][256]
    const float* part_dwm;         // [gm][128]
    const float* part_dbm;         // [gm][2]
    float* dw[3];
    float* db[3];
    float* dwm;
    float* dbm;
    float* loss;                   // [4]
    int gx, gm;
    int64_t N;
};

#define CT_RED_DW (3 * CSS_N * CSS_K)
#define CT_RED_DB (3 * CSS_N)
#define CT_RED_TOTAL (CT_RED_DW + CT_RED_DB + 2 * CSS_K + 2 + 4)

__global__ __launch_bounds__(256) void css_loss_reduce_kernel(CssReduceArgs A) {
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e < CT_RED_DW) {
        const int head = e / (CSS_N * CSS_K), i = e % (CSS_N * CSS_K);
        const float* p = A.part_dw + (int64_t)head * A.gx * CSS_N * CSS_K + i;
        float s = 0.f;
        for (int g = 0; g < A.gx; ++g) s += p[(int64_t)g * CSS_N * CSS_K];
        A.dw[head][i] = s;
        return;
    }
    e -= CT_RED_DW;
    if (e < CT_RED_DB) {
        const int head = e / CSS_N, i = e % CSS_N;
        const float* p = A.part_db + (int64_t)head * A.gx * CSS_N + i;
        float s = 0.f;
        for (int g = 0; g < A.gx; ++g) s += p[(int64_t)g * CSS_N];
        A.db[head][i] = s;
        return;
    }
    e -= CT_RED_DB;
    if (e < 2 * CSS_K) {
        float s = 0.f;
        for (int g = 0; g < A.gm; ++g) s += A.part_dwm[(int64_t)g * 128 + e];
        A.dwm[e] = s;
        return;
    }
    e -= 2 * CSS_K;
    if (e < 2) {
        float s = 0.f;
        for (int g = 0; g < A.gm; ++g) s += A.part_dbm[(int64_t)g * 2 + e];
        A.dbm[e] = s;
        return;
    }
    e -= 2;
    if (e < 3) {
        double s = 0.0, n = 0.0;
        for (int g = 0; g < A.gx; ++g) {
            s += A.part_loss[((int64_t)e * A.gx + g) * 2];
            n += A.part_loss[((int64_t)e * A.gx + g) * 2 + 1];
        }
        A.loss[e] = (float)((s + ((double)A.N - n) * CT_LN256) / (double)A.N);
    } else if (e == 3) {
        double s = 0.0;
        for (int g = 0; g < A.gm; ++g) s += A.part_lossm[g];
        A.loss[3] = (float)(2.0 * s / (double)A.N);
    }
}

// ---- latent head --------------------------------------------------------------------------------------------------------------------------------
#define CTL_K 256
#define CTL_PART (3 * CTL_K + 3)   // floats per crop: dv (x) xbar, dv

__global__ __launch_bounds__(256) void css_latent_loss_kernel(const float* __restrict__ x4, const float* __restrict__ w, const float* __restrict__ bias,
                                                              const float* __restrict__ gt, int hw, int B, float* __restrict__ dx4,
                                                              float* __restrict__ part, double* __restrict__ part_loss) {
    __shared__ float xbar[CTL_K];
    __shared__ float gcs[CTL_K];
    __shared__ float vs[3];
    __shared__ float dvs[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    {
        const float* xr = x4 + ((int64_t)b * CTL_K + tid) * hw;
        float s = 0.f;
        for (int p = 0; p < hw; ++p) s += xr[p];
        xbar[tid] = s / (float)hw;
    }
    __syncthreads();
    if (tid < 3) {
        float a = 0.f;
        for (int k = 0; k < CTL_K; ++k) a = fmaf(w[tid * CTL_K + k], xbar[k], a);
        vs[tid] = a + bias[tid];
    }
    __syncthreads();
    if (tid == 0) {
        const float v0 = vs[0], v1 = vs[1], v2 = vs[2];
        const float len = sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
        const float f = 1.0f / (len + 1e-8f);                          // the length is a constant of the backward, as in the reference
        const float d0 = v0 * f - gt[3 * b], d1 = v1 * f - gt[3 * b + 1], d2 = v2 * f - gt[3 * b + 2];
        part_loss[b] = ((double)d0 * d0 + (double)d1 * d1) + (double)d2 * d2;
        const float sc = 2.0f / (3.0f * (float)B);
        dvs[0] = d0 * sc * f;
        dvs[1] = d1 * sc * f;
        dvs[2] = d2 * sc * f;
    }
    __syncthreads();
    const float dv0 = dvs[0], dv1 = dvs[1], dv2 = dvs[2];
    gcs[tid] = fmaf(w[2 * CTL_K + tid], dv2, fmaf(w[CTL_K + tid], dv1, w[tid] * dv0)) / (float)hw;
    float* o = part + (int64_t)b * CTL_PART;
    o[tid] = dv0 * xbar[tid];
    o[CTL_K + tid] = dv1 * xbar[tid];
    o[2 * CTL_K + tid] = dv2 * xbar[tid];
    if (tid < 3) o[3 * CTL_K + tid] = dvs[tid];
    __syncthreads();
    float* d = dx4 + (int64_t)b * CTL_K * hw;
    for (int64_t i = tid; i < (int64_t)CTL_K * hw; i += 256) d[i] = gcs[i / hw];
}

__global__ __launch_bounds__(256) void css_latent_reduce_kernel(const float* __restrict__ part, const double* __restrict__ part_loss, int B,
                                                                float* __restrict__ dw, float* __restrict__ db, float* __restrict__ loss) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < CTL_PART) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += part[(int64_t)b * CTL_PART + e];
        if (e < 3 * CTL_K) dw[e] = s;
        else db[e - 3 * CTL_K] = s;
    } else if (e == CTL_PART) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += part_loss[b];
        loss[0] = (float)(s / (3.0 * (double)B));
    }
}

extern "C" int sdfr_css_head_loss(const float* x_u, const float* x_v, const float* x_w, const float* x_mask, int B, int C, int H, int W,
                                  const float* w_u, const float* b_u, const float* w_v, const float* b_v, const float* w_w, const float* b_w,
                                  const float* w_mask, const float* b_mask, const uint8_t* uvw_gt, const uint8_t* mask_gt, float* loss,
                                  float* dx_u, float* dx_v, float* dx_w, float* dx_mask, float* dw_u, float* db_u, float* dw_v, float* db_v,
                                  float* dw_w, float* db_w, float* dw_mask, float* db_mask, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    SDFR_REQUIRE(B >= 0 && H >= 0 && W >= 0, "sdfr_css_head_loss: negative size");
    SDFR_REQUIRE(C == CSS_K, "sdfr_css_head_loss: the head takes %d feature channels (got %d)", CSS_K, C);
    SDFR_REQUIRE((int64_t)H * W < (1ll << 30), "sdfr_css_head_loss: H * W = %lld is beyond 2^30", (long long)H * W);
    if (B == 0 || H == 0 || W == 0) return SDFR_OK;
    SDFR_REQUIRE(x_u && x_v && x_w && x_mask && w_u && b_u && w_v && b_v && w_w && b_w && w_mask && b_mask && uvw_gt && mask_gt,
                 "sdfr_css_head_loss: NULL input");
    SDFR_REQUIRE(loss && dx_u && dx_v && dx_w && dx_mask && dw_u && db_u && dw_v && db_v && dw_w && db_w && dw_mask && db_mask,
                 "sdfr_css_head_loss: NULL output");
    const int HW = H * W;
    const int64_t N = (int64_t)B * HW;
    const int64_t need = CT_WS_FIXED + 3 * N * 4;
    SDFR_REQUIRE(workspace != nullptr && workspace_bytes >= need, "sdfr_css_head_loss: the workspace needs %lld bytes (%lld + 12 per pixel), got %lld",
                 (long long)need, (long long)CT_WS_FIXED, (long long)(workspace ? workspace_bytes : 0));
    if (int rc = css_device_check(x_u, "sdfr_css_head_loss")) return rc;

    double* wd = reinterpret_cast<double*>(workspace);
    double* part_loss = wd;
    double* part_lossm = wd + 3 * CT_GX * 2;
    float* wf = reinterpret_cast<float*>(wd + CT_WS_DOUBLES);
    float* part_dw = wf;
    float* part_db = part_dw + (int64_t)3 * CT_GX * CSS_N * CSS_K;
    float* part_dwm = part_db + 3 * CT_GX * CSS_N;
    float* part_dbm = part_dwm + CT_MGX * 2 * CSS_K;
    float* lse = part_dbm + CT_MGX * 2;

    CssLossArgs A;
    A.x[0] = x_u; A.x[1] = x_v; A.x[2] = x_w;
    A.w[0] = w_u; A.w[1] = w_v; A.w[2] = w_w; A.b[0] = b_u; A.b[1] = b_v; A.b[2] = b_w;
    A.uvw = uvw_gt; A.mask = mask_gt;
    A.dx[0] = dx_u; A.dx[1] = dx_v; A.dx[2] = dx_w;
    A.lse = lse; A.part_loss = part_loss; A.part_dw = part_dw; A.part_db = part_db;
    A.HW = HW;
    A.tiles_per_crop = sdfr_cdiv(HW, CSS_TILE);
    A.n_tiles = (int64_t)B * A.tiles_per_crop;
    A.N = N;
    A.invN = (float)(1.0 / (double)N);
    const int gx = (int)(A.n_tiles < CT_GX ? A.n_tiles : CT_GX);

    CssMaskLossArgs M;
    M.xm = x_mask; M.wm = w_mask; M.bm = b_mask; M.mask = mask_gt; M.dxm = dx_mask;
    M.part_loss = part_lossm; M.part_dw = part_dwm; M.part_db = part_dbm;
    M.HW = HW;
    M.tiles_per_crop = sdfr_cdiv(HW, CT_MTILE);
    M.n_tiles = (int64_t)B * M.tiles_per_crop;
    M.invN = A.invN;
    const int gm = (int)(M.n_tiles < CT_MGX ? M.n_tiles : CT_MGX);

    const size_t lds_fwd = (size_t)(CSS_K * CSS_LD + CSS_N) * sizeof(float);
    const size_t lds_dw = (size_t)(CSS_K * CT_LDH + 128 + 4 * CSS_K * CT_XP + 3 * 128) * sizeof(float);
    const size_t lds_mask = (size_t)(CSS_K * CT_MLD + 2 * CT_MTILE + 2 * CSS_K + 2) * sizeof(float);
    // (more than 64 KB of dynamic LDS needs the attribute; it belongs to the current device's image of the kernel, so it is set at every call)
    SDFR_HIP_CHECK(hipFuncSetAttribute((const void*)css_loss_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fwd));
    SDFR_HIP_CHECK(hipFuncSetAttribute((const void*)css_loss_dw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dw));
    SDFR_HIP_CHECK(hipFuncSetAttribute((const void*)css_loss_mask_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_mask));
    hipLaunchKernelGGL(css_loss_fwd_kernel, dim3((unsigned)gx, 3), dim3(256), lds_fwd, (hipStream_t)stream, A);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(css_loss_dw_kernel, dim3((unsigned)gx, 3, 2), dim3(256), lds_dw, (hipStream_t)stream, A);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(css_loss_mask_kernel, dim3((unsigned)gm), dim3(256), lds_mask, (hipStream_t)stream, M);
    SDFR_LAUNCH_CHECK();
    CssReduceArgs R;
    R.part_loss = part_loss; R.part_lossm = part_lossm; R.part_dw = part_dw; R.part_db = part_db; R.part_dwm = part_dwm; R.part_dbm = part_dbm;
    R.dw[0] = dw_u; R.dw[1] = dw_v; R.dw[2] = dw_w; R.db[0] = db_u; R.db[1] = db_v; R.db[2] = db_w;
    R.dwm = dw_mask; R.dbm = db_mask; R.loss = loss;
    R.gx = gx; R.gm = gm; R.N = N;
    hipLaunchKernelGGL(css_loss_reduce_kernel, dim3((unsigned)sdfr_cdiv(CT_RED_TOTAL, 256)), dim3(256), 0, (hipStream_t)stream, R);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_css_latent_loss(const float* x4, int B, int C, int h, int w, const float* w_lat, const float* b_lat, const float* latent_gt,
                                    float* loss, float* dx4, float* dw_lat, float* db_lat, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    SDFR_REQUIRE(B >= 0 && h >= 0 && w >= 0, "sdfr_css_latent_loss: negative size");
    SDFR_REQUIRE(C == CTL_K, "sdfr_css_latent_loss: out_lat takes %d feature channels (got %d)", CTL_K, C);
    SDFR_REQUIRE((int64_t)h * w < (1ll << 22), "sdfr_css_latent_loss: h * w = %lld is beyond 2^22", (long long)h * w);
    if (B == 0 || h == 0 || w == 0) return SDFR_OK;
    SDFR_REQUIRE(x4 && w_lat && b_lat && latent_gt && loss && dx4 && dw_lat && db_lat, "sdfr_css_latent_loss: NULL argument");
    const int64_t need = (int64_t)B * (8 + CTL_PART * 4);
    SDFR_REQUIRE(workspace != nullptr && workspace_bytes >= need, "sdfr_css_latent_loss: the workspace needs %lld bytes (%d per crop), got %lld",
                 (long long)need, 8 + CTL_PART * 4, (long long)(workspace ? workspace_bytes : 0));
    if (int rc = css_device_check(x4, "sdfr_css_latent_loss")) return rc;
    double* part_loss = reinterpret_cast<double*>(workspace);
    float* part = reinterpret_cast<float*>(part_loss + B);
    hipLaunchKernelGGL(css_latent_loss_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x4, w_lat, b_lat, latent_gt, h * w, B, dx4, part,
                       part_loss);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(css_latent_reduce_kernel, dim3((unsigned)sdfr_cdiv(CTL_PART + 1, 256)), dim3(256), 0, (hipStream_t)stream, part, part_loss, B,
                       dw_lat, db_lat, loss);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
