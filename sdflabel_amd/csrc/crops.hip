// Export of CSS training crops from rasterised autolabels ("Training crops").  The per-pixel arithmetic is crop_cells.h; this
// file holds the launches.
//
//   sdfr_crop_owner     per window pixel of a frame's rasters (sdfr_mesh_raster's packed mask / depth): which annotation is nearest there.
//                       One thread per window pixel, a loop over the B windows.  AN OCCLUDER IS SEEN ONLY INSIDE ITS OWN WINDOW: what an
//                       annotation's mesh would cover outside the window it was rendered into does not exist for the others.
//   sdfr_crop_export    per annotation a half-open box inside its window: the NOCS bytes of the winning triangle's interpolated vertex
//                       attributes where the annotation is visible, zeros elsewhere, and the colour crop as RGB bytes.  An init launch (flag
//                       words), one thread per box pixel, then a launch that zeroes the pixels of annotations whose flag says invalid.
//   sdfr_crop_counts    per annotation: box pixels, covered, visible, flag word (one workgroup per annotation, integer sums in a fixed tree)
//
// No float atomics (the only atomic is an integer or on the flag words), no host synchronisation: the same bits on every run, and with
// occlusion off an annotation's bytes do not depend on the batch around it.  Compiled with -ffp-contract=off (build.sh).
#include "sdfr_common.h"
#include "crop_cells.h"

namespace {

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_crop_owner_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ depth,
                                                                     const int32_t* __restrict__ windows, const int64_t* __restrict__ poff,
                                                                     int64_t P, int B, int W, int H, int32_t* __restrict__ owner) {
    const int64_t i = (int64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (i >= P) return;
    const int b = verify_owner(poff, B, i);
    const int32_t* w = windows + 4 * b;
    if (!verify_window_ok(w, poff + b, P, W, H) || i < poff[b] || i >= poff[b + 1]) {        // the pixel belongs to no usable window
        owner[i] = -1;
        return;
    }
    const int64_t local = i - poff[b];
    const int ww = w[2] - w[0];                                                            // > 0: the window holds pixel i
    owner[i] = crop_owner_pixel(mask, depth, windows, poff, P, B, W, H, b, i, w[0] + (int)(local % ww), w[1] + (int)(local / ww));
}

// flag words: 0, or VERIFY_FLAG_INVALID for an annotation whose window, box and offsets do not fit (a kernel, not a memset: every entry
// point may be captured into a graph, sdfr_common.h)
__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_crop_init_kernel(CropArgs a, int32_t* __restrict__ flags) {
    const int b = blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (b < a.B) flags[b] = crop_anno_ok(&a, b) ? 0 : VERIFY_FLAG_INVALID;
}

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_crop_export_kernel(CropArgs a, const int32_t* __restrict__ triangle,
                                                                      const int32_t* __restrict__ owner, const float* __restrict__ colors,
                                                                      uint8_t* __restrict__ uvw, uint8_t* __restrict__ rgb,
                                                                      int32_t* __restrict__ flags) {
    const int64_t g = (int64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (g >= a.Q) return;
    uint8_t out[3];
    int b;
    int64_t at;
    const int raise = crop_export_pixel(&a, triangle, owner, g, out, &b, &at);
    if (raise) atomicOr(&flags[b], raise);                                                  // b is a usable annotation whenever a flag is raised
    uvw[3 * g] = out[0], uvw[3 * g + 1] = out[1], uvw[3 * g + 2] = out[2];
    if (rgb) {                                                                              // BGR in, RGB out; zeros for a pixel of no usable annotation
        for (int k = 0; k < 3; ++k) rgb[3 * g + k] = b >= 0 ? crop_rgb_byte(colors[3 * g + (2 - k)]) : (uint8_t)0;
    }
}

// after the export: the pixels of an annotation whose flag word says invalid are zeroed (a bad triangle index is found by one pixel only)
__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_crop_scrub_kernel(CropArgs a, const int32_t* __restrict__ flags, uint8_t* __restrict__ uvw,
                                                                     uint8_t* __restrict__ rgb) {
    const int64_t g = (int64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (g >= a.Q) return;
    const int b = verify_owner(a.qoff, a.B, g);
    if (!(flags[b] & VERIFY_FLAG_INVALID)) return;
    uvw[3 * g] = uvw[3 * g + 1] = uvw[3 * g + 2] = 0;
    if (rgb) rgb[3 * g] = rgb[3 * g + 1] = rgb[3 * g + 2] = 0;
}

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_crop_counts_kernel(CropArgs a, const uint8_t* __restrict__ mask, const int32_t* __restrict__ owner,
                                                                      const int32_t* __restrict__ flags, int32_t* __restrict__ counts) {
    __shared__ int sh[VERIFY_BLOCK];
    const int b = blockIdx.x;
    int32_t* o = counts + CROP_COUNTS * b;
    const bool fits = verify_window_ok(a.windows + 4 * b, a.poff + b, a.P, a.W, a.H) && crop_box_ok(a.boxes + 4 * b, a.windows + 4 * b, a.qoff + b, a.Q);
    const int32_t word = (flags ? flags[b] : 0) | (fits ? 0 : VERIFY_FLAG_INVALID);
    if (word & VERIFY_FLAG_INVALID) {                        // uniform over the workgroup
        if (threadIdx.x < CROP_COUNTS) o[threadIdx.x] = threadIdx.x == CROP_COUNTS - 1 ? word : 0;
        return;
    }
    const int32_t* w = a.windows + 4 * b;
    const int32_t* box = a.boxes + 4 * b;
    const int bw = box[2] - box[0];
    const int n = bw * (box[3] - box[1]);                    // at most the image: below 2^31
    int covered = 0, visible = 0;
    for (int i = threadIdx.x; i < n; i += VERIFY_BLOCK) {
        const int x = box[0] + i % bw, y = box[1] + i / bw;
        const int64_t at = verify_window_pixel(w, a.poff[b], x, y);
        const bool c = mask[at] != 0;
        covered += c;
        visible += c && (!owner || owner[at] == b);
    }
    covered = verify_block_reduce<0>(covered, sh);
    visible = verify_block_reduce<0>(visible, sh);
    if (threadIdx.x == 0) o[0] = n, o[1] = covered, o[2] = visible, o[3] = word;
}

unsigned crop_blocks(int64_t n) { return (unsigned)((n + VERIFY_BLOCK - 1) / VERIFY_BLOCK); }

}  // namespace

extern "C" int sdfr_crop_owner(const uint8_t* mask, const float* depth, const int32_t* windows, const int64_t* poff, int64_t P, int B, int W, int H,
                               int32_t* owner, void* stream) {
    SDFR_REQUIRE(B >= 0 && W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31), "sdfr_crop_owner: B = %d, image %d x %d", B, W, H);
    SDFR_REQUIRE(P >= 0 && P <= (int64_t)B * W * H, "sdfr_crop_owner: P = %lld out of range (P <= B W H)", (long long)P);
    if (B == 0 || P == 0) return SDFR_OK;
    SDFR_REQUIRE(mask && depth && windows && poff && owner, "sdfr_crop_owner: NULL pointer");
    hipLaunchKernelGGL(sdfr_crop_owner_kernel, dim3(crop_blocks(P)), dim3(VERIFY_BLOCK), 0, (hipStream_t)stream, mask, depth, windows, poff, P, B, W, H,
                       owner);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_crop_export(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const float* attributes, const int64_t* voff,
                                const int64_t* toff, const int32_t* windows, const int64_t* poff, int64_t P, const int32_t* triangle,
                                const int32_t* owner, const int32_t* boxes, const int64_t* qoff, int64_t Q, const float* colors, int B, int W, int H,
                                const double* K, float z_min, uint8_t* uvw, uint8_t* rgb, int32_t* flags, void* stream) {
    SDFR_REQUIRE(B >= 0 && W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31), "sdfr_crop_export: B = %d, image %d x %d", B, W, H);
    SDFR_REQUIRE(V >= 0 && T >= 0 && P >= 0 && Q >= 0 && T < ((int64_t)1 << 31) && V < ((int64_t)1 << 31) && P <= (int64_t)B * W * H && Q <= P,
                 "sdfr_crop_export: V = %lld, T = %lld, P = %lld, Q = %lld out of range (Q <= P <= B W H)", (long long)V, (long long)T, (long long)P,
                 (long long)Q);
    SDFR_REQUIRE(K && K[0] == K[0] && K[1] == K[1] && K[2] == K[2] && K[3] == K[3], "sdfr_crop_export: the intrinsics are NULL or NaN");
    SDFR_REQUIRE(z_min >= 0.0f, "sdfr_crop_export: z_min must not be negative");
    SDFR_REQUIRE((rgb == nullptr) == (colors == nullptr), "sdfr_crop_export: colors and rgb go together");
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(voff && toff && windows && poff && boxes && qoff && flags, "sdfr_crop_export: NULL pointer");
    SDFR_REQUIRE((V == 0 || (vertices && attributes)) && (T == 0 || faces), "sdfr_crop_export: NULL mesh");
    SDFR_REQUIRE((P == 0 || triangle) && (Q == 0 || uvw), "sdfr_crop_export: NULL triangle image or output");
    const CropArgs a = {raster_args(vertices, V, faces, T, voff, toff, windows, poff, P, B, W, H, K, z_min), attributes, boxes, qoff, Q};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sdfr_crop_init_kernel, dim3(crop_blocks(B)), dim3(VERIFY_BLOCK), 0, s, a, flags);
    SDFR_LAUNCH_CHECK();
    if (Q > 0) {
        hipLaunchKernelGGL(sdfr_crop_export_kernel, dim3(crop_blocks(Q)), dim3(VERIFY_BLOCK), 0, s, a, triangle, owner, colors, uvw, rgb, flags);
        SDFR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sdfr_crop_scrub_kernel, dim3(crop_blocks(Q)), dim3(VERIFY_BLOCK), 0, s, a, (const int32_t*)flags, uvw, rgb);
        SDFR_LAUNCH_CHECK();
    }
    return SDFR_OK;
}

extern "C" int sdfr_crop_counts(const uint8_t* mask, const int32_t* owner, const int32_t* windows, const int64_t* poff, int64_t P,
                                const int32_t* boxes, const int64_t* qoff, int64_t Q, const int32_t* flags, int B, int W, int H, int32_t* counts,
                                void* stream) {
    SDFR_REQUIRE(B >= 0 && W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31), "sdfr_crop_counts: B = %d, image %d x %d", B, W, H);
    SDFR_REQUIRE(P >= 0 && Q >= 0 && P <= (int64_t)B * W * H && Q <= P, "sdfr_crop_counts: P = %lld, Q = %lld out of range (Q <= P <= B W H)",
                 (long long)P, (long long)Q);
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(windows && poff && boxes && qoff && counts && (P == 0 || mask), "sdfr_crop_counts: NULL pointer");
    const CropArgs a = {raster_args(nullptr, 0, nullptr, 0, nullptr, nullptr, windows, poff, P, B, W, H, nullptr, 0.0f), nullptr, boxes, qoff, Q};
    hipLaunchKernelGGL(sdfr_crop_counts_kernel, dim3((unsigned)B), dim3(VERIFY_BLOCK), 0, (hipStream_t)stream, a, mask, owner, flags, counts);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
