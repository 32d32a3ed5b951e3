// Verification of refined autolabels ("Verification"): an exact rasteriser of camera-frame triangle meshes into the label's
// window, the counts behind the projective test, and the lidar points in the decoder's band behind the geometric test.  The per-triangle,
// per-pixel and per-point arithmetic is verify_cells.h; this file holds the launches.
//
//   sdfr_mesh_raster          B ragged meshes, each into its own window: an init launch, 64-bit keys by an integer atomic minimum, then a resolve launch
//                             to mask / depth / winning triangle.  A lane takes a triangle; a triangle whose pixel box holds more than
//                             VERIFY_SMALL pixels is left to the whole wave afterwards, 64 pixels at a time.
//   sdfr_verify_mask_counts   per mesh: covered area, tight box of the covered pixels, label area and intersection (one workgroup per mesh,
//                             integer sums in a fixed tree)
//   sdfr_verify_point_rows    the decoder's input rows latent || x of camera-frame points taken to the lattice frame of their annotation
//   sdfr_verify_band_counts   per annotation: points, points inside the cube, points in the band (one workgroup per annotation)
//
// The only atomics are integer minimum / or: the same bits on every run, whatever the schedule, and a mesh's output does not depend on the
// batch around it.  Compiled with -ffp-contract=off (build.sh).
#include "sdfr_common.h"
#include "verify_cells.h"

#define VERIFY_SMALL 32          // pixel boxes up to this many pixels are walked by the triangle's own lane

namespace {

// set up global triangle g of the ragged batch for its mesh's window; returns the status and the mesh; flags are raised here
__device__ __forceinline__ int verify_load_tri(const RasterArgs& a, int64_t g, VerifyTri* T, int* mesh, int32_t* local, int32_t* flags) {
    const int b = verify_owner(a.toff, a.B, g);
    *mesh = b;
    *local = (int32_t)(g - a.toff[b]);
    const int64_t v0 = a.voff[b], nv = a.voff[b + 1] - v0;
    const int32_t f[3] = {a.faces[3 * g], a.faces[3 * g + 1], a.faces[3 * g + 2]};
    const int32_t* w = a.windows + 4 * b;
    const bool idx_ok = v0 >= 0 && a.voff[b + 1] <= a.V && verify_face_ok(f, nv);
    if (!idx_ok || !verify_window_ok(w, a.poff + b, a.P, a.W, a.H)) {
        atomicOr(&flags[b], VERIFY_FLAG_INVALID);
        return VERIFY_TRI_SKIP;
    }
    const int st = verify_tri_setup(a.vertices + 3 * (v0 + f[0]), a.vertices + 3 * (v0 + f[1]), a.vertices + 3 * (v0 + f[2]), a.K, a.z_min, w[0], w[1],
                                    w[2], w[3], T);
    if (st == VERIFY_TRI_BEHIND) atomicOr(&flags[b], VERIFY_FLAG_BEHIND);
    return st;
}

__device__ __forceinline__ void verify_put(const RasterArgs& a, int b, const VerifyTri& T, int x, int y, int32_t local,
                                           unsigned long long* keys) {
    const uint64_t key = verify_pixel_key(&T, x, y, (uint32_t)local);
    if (key == VERIFY_NO_KEY) return;
    // (x, y) is inside the window (verify_tri_setup clamped the box) and the window's pixels are poff[b] .. poff[b + 1] (verify_window_ok)
    atomicMin(&keys[verify_window_pixel(a.windows + 4 * b, a.poff[b], x, y)], (unsigned long long)key);
}

// keys to "no cover", flags to 0 (a kernel, not a memset: every entry point may be captured into a graph, sdfr_common.h)
__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_mesh_raster_init_kernel(unsigned long long* __restrict__ keys, int64_t P,
                                                                             int32_t* __restrict__ flags, int B) {
    const int64_t i = (int64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i < P) keys[i] = VERIFY_NO_KEY;
    if (i < B) flags[i] = 0;
}

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_mesh_raster_kernel(RasterArgs a, unsigned long long* __restrict__ keys,
                                                                        int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    const int64_t base = g - lane;                                       // the wave's first triangle
    VerifyTri T;
    int b = 0;
    int32_t local = 0;
    bool big = false;
    if (g < a.T && verify_load_tri(a, g, &T, &b, &local, flags) == VERIFY_TRI_OK) {
        const int bw = T.x1 - T.x0 + 1, bh = T.y1 - T.y0 + 1;
        const int64_t n = (int64_t)bw * bh;                              // at most the window: below 2^31
        if (n <= VERIFY_SMALL) {
            for (int i = 0; i < (int)n; ++i) verify_put(a, b, T, T.x0 + i % bw, T.y0 + i / bw, local, keys);
        } else {
            big = true;
        }
    }
    // the large boxes of this wave, one after the other, 64 pixels at a time.  Every lane sets the triangle up again itself: the flags it
    // would raise are raised already, and a triangle that reached this point has status OK.
    unsigned long long todo = __ballot(big);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        VerifyTri L;
        int lb = 0;
        int32_t ll = 0;
        if (verify_load_tri(a, base + leader, &L, &lb, &ll, flags) != VERIFY_TRI_OK) continue;      // (cannot happen; uniform over the wave)
        const int bw = L.x1 - L.x0 + 1, bh = L.y1 - L.y0 + 1;
        const int n = bw * bh;
        for (int i = lane; i < n; i += 64) verify_put(a, lb, L, L.x0 + i % bw, L.y0 + i / bw, ll, keys);
    }
}

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_mesh_resolve_kernel(const unsigned long long* __restrict__ keys, int64_t P,
                                                                         uint8_t* __restrict__ mask, float* __restrict__ depth,
                                                                         int32_t* __restrict__ tri) {
    const int64_t i = (int64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= P) return;
    verify_resolve((uint64_t)keys[i], &mask[i], &depth[i], &tri[i]);
}

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_verify_mask_counts_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ label,
                                                                               RasterArgs a, int32_t* __restrict__ out) {
    __shared__ int sh[VERIFY_BLOCK];
    const int b = blockIdx.x;
    int32_t* o = out + 8 * b;
    const int32_t* w = a.windows + 4 * b;
    if (!verify_window_ok(w, a.poff + b, a.P, a.W, a.H)) {   // uniform over the workgroup
        if (threadIdx.x < 8) o[threadIdx.x] = threadIdx.x == 7 ? VERIFY_FLAG_INVALID : 0;
        return;
    }
    const int l = w[0], t = w[1], ww = w[2] - w[0];
    const int n = ww * (w[3] - w[1]);
    const uint8_t* m = mask + a.poff[b];
    const uint8_t* lab = label ? label + a.poff[b] : nullptr;
    int area = 0, la = 0, inter = 0, x0 = INT32_MAX, y0 = INT32_MAX, x1 = -1, y1 = -1;
    for (int i = threadIdx.x; i < n; i += VERIFY_BLOCK) {
        const bool c = m[i] != 0, g = lab && lab[i] != 0;
        area += c, la += g, inter += c && g;
        if (c) {
            const int x = l + i % ww, y = t + i / ww;
            x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1, y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1;
        }
    }
    area = verify_block_reduce<0>(area, sh);
    la = verify_block_reduce<0>(la, sh);
    inter = verify_block_reduce<0>(inter, sh);
    x0 = verify_block_reduce<1>(x0, sh);
    y0 = verify_block_reduce<1>(y0, sh);
    x1 = verify_block_reduce<2>(x1, sh);
    y1 = verify_block_reduce<2>(y1, sh);
    if (threadIdx.x == 0) {
        o[0] = area;
        o[1] = area ? x0 : 0, o[2] = area ? y0 : 0, o[3] = area ? x1 + 1 : 0, o[4] = area ? y1 + 1 : 0;
        o[5] = la, o[6] = inter, o[7] = 0;
    }
}

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_verify_point_rows_kernel(const float* __restrict__ points, const int64_t* __restrict__ ptoff,
                                                                              int B, const float* __restrict__ pose,
                                                                              const float* __restrict__ latents, int L, int64_t row0,
                                                                              int64_t total, float* __restrict__ rows,
                                                                              uint8_t* __restrict__ in_cube) {
    const int64_t e = (int64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (e >= total) return;
    const int NI = L + 3;
    const int64_t r = e / NI, g = row0 + r;
    const int c = (int)(e - r * NI);
    const int b = verify_owner(ptoff, B, g);
    if (c < L) {
        rows[e] = latents[(int64_t)b * L + c];
        return;
    }
    float x[3];
    const uint8_t in = verify_point_x(points + 3 * g, pose + VERIFY_POSE * b, x);
    rows[e] = x[c - L];
    if (c == L) in_cube[g] = in;
}

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_verify_band_counts_kernel(const float* __restrict__ sdf, const uint8_t* __restrict__ in_cube,
                                                                               const int64_t* __restrict__ ptoff, const float* __restrict__ pose,
                                                                               float band, int64_t N, int32_t* __restrict__ counts) {
    __shared__ int sh[VERIFY_BLOCK];
    const int b = blockIdx.x;
    int64_t p0 = ptoff[b], p1 = ptoff[b + 1];
    if (p0 < 0 || p1 > N || p1 < p0) p0 = p1 = 0;             // offsets outside the arrays: nothing is read
    const float scale = pose[VERIFY_POSE * b + 5];
    int cube = 0, bnd = 0;
    for (int64_t i = p0 + threadIdx.x; i < p1; i += VERIFY_BLOCK) {
        const uint8_t in = in_cube[i];
        cube += in != 0;
        bnd += verify_in_band(sdf[i], in, scale, band);
    }
    cube = verify_block_reduce<0>(cube, sh);
    bnd = verify_block_reduce<0>(bnd, sh);
    if (threadIdx.x == 0) {
        counts[3 * b] = (int32_t)(p1 - p0);
        counts[3 * b + 1] = cube;
        counts[3 * b + 2] = bnd;
    }
}

}  // namespace

extern "C" int sdfr_mesh_raster(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const int64_t* voff, const int64_t* toff,
                                const int32_t* windows, const int64_t* poff, int64_t P, int B, int W, int H, const double* K, float z_min,
                                void* keys, uint8_t* mask, float* depth, int32_t* triangle, int32_t* flags, void* stream) {
    SDFR_REQUIRE(B >= 0 && W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31), "sdfr_mesh_raster: B = %d, image %d x %d", B, W, H);
    SDFR_REQUIRE(V >= 0 && T >= 0 && P >= 0 && T < ((int64_t)1 << 31) && V < ((int64_t)1 << 31) && P <= (int64_t)B * W * H,
                 "sdfr_mesh_raster: V = %lld, T = %lld, P = %lld out of range (P <= B W H)", (long long)V, (long long)T, (long long)P);
    SDFR_REQUIRE(K && K[0] == K[0] && K[1] == K[1] && K[2] == K[2] && K[3] == K[3], "sdfr_mesh_raster: the intrinsics are NULL or NaN");
    SDFR_REQUIRE(z_min >= 0.0f, "sdfr_mesh_raster: z_min must not be negative");
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(voff && toff && windows && poff && flags, "sdfr_mesh_raster: NULL pointer");
    SDFR_REQUIRE((V == 0 || vertices) && (T == 0 || faces), "sdfr_mesh_raster: NULL mesh");
    SDFR_REQUIRE(P == 0 || (keys && mask && depth && triangle), "sdfr_mesh_raster: NULL output");
    const RasterArgs a = raster_args(vertices, V, faces, T, voff, toff, windows, poff, P, B, W, H, K, z_min);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_init = P > B ? P : B;
    hipLaunchKernelGGL(sdfr_mesh_raster_init_kernel, dim3((unsigned)((n_init + VERIFY_BLOCK - 1) / VERIFY_BLOCK)), dim3(VERIFY_BLOCK), 0, s,
                       (unsigned long long*)keys, P, flags, B);
    SDFR_LAUNCH_CHECK();
    if (T > 0) {
        hipLaunchKernelGGL(sdfr_mesh_raster_kernel, dim3((unsigned)((T + VERIFY_BLOCK - 1) / VERIFY_BLOCK)), dim3(VERIFY_BLOCK), 0, s, a,
                           (unsigned long long*)keys, flags);
        SDFR_LAUNCH_CHECK();
    }
    if (P > 0) {
        hipLaunchKernelGGL(sdfr_mesh_resolve_kernel, dim3((unsigned)((P + VERIFY_BLOCK - 1) / VERIFY_BLOCK)), dim3(VERIFY_BLOCK), 0, s,
                           (const unsigned long long*)keys, P, mask, depth, triangle);
        SDFR_LAUNCH_CHECK();
    }
    return SDFR_OK;
}

extern "C" int sdfr_verify_mask_counts(const uint8_t* mask, const uint8_t* label_mask, const int32_t* windows, const int64_t* poff, int64_t P,
                                       int B, int W, int H, int32_t* counts, void* stream) {
    SDFR_REQUIRE(B >= 0 && W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31), "sdfr_verify_mask_counts: B = %d, image %d x %d", B, W, H);
    SDFR_REQUIRE(P >= 0 && P <= (int64_t)B * W * H, "sdfr_verify_mask_counts: P = %lld out of range (P <= B W H)", (long long)P);
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(windows && poff && counts && (P == 0 || mask), "sdfr_verify_mask_counts: NULL pointer");
    const RasterArgs a = raster_args(nullptr, 0, nullptr, 0, nullptr, nullptr, windows, poff, P, B, W, H, nullptr, 0.0f);
    hipLaunchKernelGGL(sdfr_verify_mask_counts_kernel, dim3((unsigned)B), dim3(VERIFY_BLOCK), 0, (hipStream_t)stream, mask, label_mask, a, counts);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_verify_point_rows(const float* points, int64_t N, const int64_t* ptoff, int B, const float* pose, const float* latents, int L,
                                      int64_t row0, int64_t nrows, float* rows, uint8_t* in_cube, void* stream) {
    SDFR_REQUIRE(B >= 1 && N >= 0 && L >= 0 && L <= 4096, "sdfr_verify_point_rows: B = %d, N = %lld, latent size %d", B, (long long)N, L);
    SDFR_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= N, "sdfr_verify_point_rows: rows %lld + %lld outside the %lld points",
                 (long long)row0, (long long)nrows, (long long)N);
    if (nrows == 0) return SDFR_OK;
    SDFR_REQUIRE(points && ptoff && pose && (L == 0 || latents) && rows && in_cube, "sdfr_verify_point_rows: NULL pointer");
    const int64_t total = nrows * (L + 3);
    SDFR_REQUIRE((total + VERIFY_BLOCK - 1) / VERIFY_BLOCK < ((int64_t)1 << 31), "sdfr_verify_point_rows: chunk too large");
    hipLaunchKernelGGL(sdfr_verify_point_rows_kernel, dim3((unsigned)((total + VERIFY_BLOCK - 1) / VERIFY_BLOCK)), dim3(VERIFY_BLOCK), 0,
                       (hipStream_t)stream, points, ptoff, B, pose, latents, L, row0, total, rows, in_cube);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_verify_band_counts(const float* sdf, const uint8_t* in_cube, int64_t N, const int64_t* ptoff, int B, const float* pose,
                                       float band, int32_t* counts, void* stream) {
    SDFR_REQUIRE(B >= 0 && N >= 0, "sdfr_verify_band_counts: B = %d, N = %lld", B, (long long)N);
    SDFR_REQUIRE(band == band, "sdfr_verify_band_counts: the band is NaN");
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(ptoff && pose && counts && (N == 0 || (sdf && in_cube)), "sdfr_verify_band_counts: NULL pointer");
    hipLaunchKernelGGL(sdfr_verify_band_counts_kernel, dim3((unsigned)B), dim3(VERIFY_BLOCK), 0, (hipStream_t)stream, sdf, in_cube, ptoff, pose,
                       band, N, counts);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
