// Frame labelling on the device (gfx950): depth-crop reprojection and segmented point extents.
//
// sdfr_reproject replaces utils/refinement.py:360-410 (torch branch) for B ragged crops: the pixels with depth != 0 (torch.nonzero, :378), in
// row-major order, optionally only those with some colour channel > 0 (:404-408), as points = (Kinv [x, y, 1]) depth (:381-382) and colours.
// The compaction keeps the pixel order (the RANSAC draws index rows of the result): per-256-pixel block counts, then block offset + ballot rank,
// as the band selection of surface.hip does.
// sdfr_point_extents is the min / max of p' = A (s p) + t (and of its pinhole projection) over ragged point lists, one list per annotation:
// the box of the initial pose's projection and the cloud's lowest y (pipelines/refine_css.py:181-189), and the label's dimensions
// (utils/refinement.py:541-545).
// Compiled with -ffp-contract=off: every multiply / add rounds separately, like the reference's ATen and numpy ops.
#include <hip/hip_fp16.h>
#include "sdfr_common.h"

// crop b's pixel p is kept?  meta[b] = (W, H, first pixel of the crop in depth, colour layout: 1 = (3, H, W), 0 = (H, W, 3))
__device__ __forceinline__ bool rp_keep(const float* __restrict__ depth, const float* __restrict__ color, const int32_t* __restrict__ m, int p,
                                        int filter, float* d_out, float c_out[3]) {
    const int npix = m[0] * m[1];
    if (p >= npix) return false;
    const int64_t off = m[2];
    const float d = depth[off + p];
    if (!(d != 0.f)) return false;                       // torch.nonzero: NaN counts as non-zero
    const float* c = color + 3 * off;
    if (m[3]) { c_out[0] = c[p]; c_out[1] = c[(int64_t)npix + p]; c_out[2] = c[2 * (int64_t)npix + p]; }
    else      { c_out[0] = c[3 * (int64_t)p]; c_out[1] = c[3 * (int64_t)p + 1]; c_out[2] = c[3 * (int64_t)p + 2]; }
    *d_out = d;
    return !filter || c_out[0] > 0.f || c_out[1] > 0.f || c_out[2] > 0.f;
}

__global__ __launch_bounds__(256) void sdfr_reproject_count_kernel(const float* __restrict__ depth, const float* __restrict__ color,
                                                                  const int32_t* __restrict__ meta, int filter,
                                                                  int32_t* __restrict__ blockcnt) {
    const int b = blockIdx.y;
    float d, c[3];
    const bool in = rp_keep(depth, color, meta + 4 * b, blockIdx.x * 256 + threadIdx.x, filter, &d, c);
    const unsigned long long bal = __ballot(in);
    __shared__ int wc[4];
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) blockcnt[(int64_t)b * gridDim.x + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

__global__ __launch_bounds__(256) void sdfr_reproject_scatter_kernel(const float* __restrict__ depth, const float* __restrict__ color,
                                                                    const int32_t* __restrict__ meta, const float* __restrict__ kinv,
                                                                    int filter, const int32_t* __restrict__ blockcnt, int cap,
                                                                    float* __restrict__ points, float* __restrict__ colors,
                                                                    int32_t* __restrict__ cnt, int32_t* __restrict__ over, int over_bit) {
    const int b = blockIdx.y, nblk = gridDim.x, tid = threadIdx.x;
    const int32_t* m = meta + 4 * b;
    __shared__ int part[256];
    __shared__ int wc[4];
    int s = 0;
    for (int i = tid; i < (int)blockIdx.x; i += 256) s += blockcnt[(int64_t)b * nblk + i];
    part[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) part[tid] += part[tid + st];
        __syncthreads();
    }
    const int base = part[0];
    const int p = blockIdx.x * 256 + tid;
    float d = 0.f, c[3] = {0.f, 0.f, 0.f};
    const bool in = rp_keep(depth, color, m, p, filter, &d, c);
    const unsigned long long bal = __ballot(in);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wc[wv] = __popcll(bal);
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wv; ++w) woff += wc[w];
    const int rank = base + woff + __popcll(bal & ((1ull << lane) - 1ull));
    if (in && rank < cap) {
        const float x = (float)(p % m[0]), y = (float)(p / m[0]);
        const float* k = kinv + 9 * b;
        const int64_t e = 3 * ((int64_t)b * cap + rank);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            points[e + r] = (k[3 * r] * x + k[3 * r + 1] * y + k[3 * r + 2]) * d;      // (Kinv @ [x, y, 1]) * depth
            colors[e + r] = c[r];
        }
    }
    if (blockIdx.x == nblk - 1 && tid == 0) {
        const int total = base + wc[0] + wc[1] + wc[2] + wc[3];
        cnt[b] = total;                                                                // the TRUE count (callers compare against cap)
        if (over && total > cap) atomicOr(&over[b], over_bit);
    }
}

extern "C" int sdfr_reproject(const float* depth, const float* color, const int32_t* meta, const float* kinv, int B, int max_pix, int filter,
                              int cap, float* points, float* colors, int32_t* cnt, int32_t* scratch, int32_t* over, int over_bit, void* stream) {
    SDFR_REQUIRE(B >= 0 && max_pix >= 0 && cap >= 0, "sdfr_reproject: negative size");
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(meta && kinv && cnt && scratch, "sdfr_reproject: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    if (max_pix == 0) { SDFR_HIP_CHECK(sdfr_zero_async(cnt, sizeof(int32_t) * B, s)); return SDFR_OK; }
    SDFR_REQUIRE(depth && color, "sdfr_reproject: NULL image");
    SDFR_REQUIRE(cap == 0 || (points && colors), "sdfr_reproject: NULL output");
    dim3 grid(sdfr_cdiv(max_pix, 256), B);
    hipLaunchKernelGGL(sdfr_reproject_count_kernel, grid, dim3(256), 0, s, depth, color, meta, filter, scratch);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_reproject_scatter_kernel, grid, dim3(256), 0, s, depth, color, meta, kinv, filter, scratch, cap, points, colors, cnt,
                       over, over_bit);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// ---- segmented extents -------------------------------------------------------------------------------------------------------------------
// One workgroup per segment.  Minima and maxima do not depend on the order of the comparisons, so any launch shape returns the same bits.
#define SDFR_EXT_THREADS 1024
#define SDFR_EXT_VALUES 10       // xmin xmax ymin ymax zmin zmax umin umax vmin vmax

__global__ __launch_bounds__(SDFR_EXT_THREADS) void sdfr_point_extents_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                                             const int32_t* __restrict__ cnt, int cap,
                                                                             const float* __restrict__ A, const float* __restrict__ sc,
                                                                             const float* __restrict__ t, const float* __restrict__ K, int flags,
                                                                             float* __restrict__ ext, int32_t* __restrict__ n_out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = sdfr_count(cnt, b, cap);
    const float* p = pts + 3 * (off ? off[b] : (int64_t)b * cap);
    float a[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tr[3] = {0.f, 0.f, 0.f}, s = 1.f;
    if (A) for (int i = 0; i < 9; ++i) a[i] = A[9 * b + i];
    if (t) for (int i = 0; i < 3; ++i) tr[i] = t[3 * b + i];
    if (sc) s = sc[b];
    const bool half = flags & 1;
    if (half) s = __half2float(__float2half(s));
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
    if (K) { fx = K[9 * b]; cx = K[9 * b + 2]; fy = K[9 * b + 4]; cy = K[9 * b + 5]; }
    const float inf = __builtin_huge_valf();
    float lo[5] = {inf, inf, inf, inf, inf}, hi[5] = {-inf, -inf, -inf, -inf, -inf};
    for (int i = tid; i < n; i += SDFR_EXT_THREADS) {
        float q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v = p[3 * (int64_t)i + k];
            if (half) v = __half2float(__float2half(__half2float(__float2half(v)) * s));     // a float16 cloud times a float16 scale, in float16
            else v = v * s;
            q[k] = v;
        }
        float w[5];
#pragma unroll
        for (int r = 0; r < 3; ++r) w[r] = ((a[3 * r] * q[0] + a[3 * r + 1] * q[1]) + a[3 * r + 2] * q[2]) + tr[r];
        w[3] = fx * (w[0] / w[2]) + cx;                                                       // pinhole, no distortion
        w[4] = fy * (w[1] / w[2]) + cy;
#pragma unroll
        for (int k = 0; k < 5; ++k) { lo[k] = fminf(lo[k], w[k]); hi[k] = fmaxf(hi[k], w[k]); }
    }
    __shared__ float red[SDFR_EXT_THREADS / 64][SDFR_EXT_VALUES];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], o, 64));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o, 64));
        }
        if ((tid & 63) == 0) { red[tid >> 6][2 * k] = lo[k]; red[tid >> 6][2 * k + 1] = hi[k]; }
    }
    __syncthreads();
    const int nv = K ? SDFR_EXT_VALUES : 6;
    if (tid < nv) {
        float v = red[0][tid];
        for (int w = 1; w < SDFR_EXT_THREADS / 64; ++w) v = (tid & 1) ? fmaxf(v, red[w][tid]) : fminf(v, red[w][tid]);
        ext[(int64_t)b * SDFR_EXT_VALUES + tid] = n > 0 ? v : __builtin_nanf("");            // an empty list has no extreme
    } else if (tid < SDFR_EXT_VALUES) {
        ext[(int64_t)b * SDFR_EXT_VALUES + tid] = __builtin_nanf("");
    }
    if (tid == 0) n_out[b] = n;
}

extern "C" int sdfr_point_extents(const float* pts, const int64_t* off, const int32_t* cnt, int cap, int B, const float* A, const float* scale,
                                  const float* t, const float* K, int flags, float* ext, int32_t* n_out, void* stream) {
    SDFR_REQUIRE(B >= 0 && cap >= 0, "sdfr_point_extents: negative size");
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(ext && n_out, "sdfr_point_extents: NULL output");
    SDFR_REQUIRE(pts || cap == 0, "sdfr_point_extents: NULL points");
    SDFR_REQUIRE(cnt || !off, "sdfr_point_extents: lists given by offsets need their counts");
    SDFR_REQUIRE((flags & ~1) == 0, "sdfr_point_extents: unknown flag");
    hipLaunchKernelGGL(sdfr_point_extents_kernel, dim3(B), dim3(SDFR_EXT_THREADS), 0, (hipStream_t)stream, pts, off, cnt, cap, A, scale, t, K,
                       flags, ext, n_out);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
