// Synthetic bootstrap crops: colour images of posed shapes rendered from the shape prior ("Synthetic crops").  The per-pixel
// arithmetic is synth_cells.h; this file holds the launches.
//
//   sdfr_synth_owner    sdfr_crop_owner with a scene table: several scenes -- different images that share K and the image size -- in one
//                       launch, and an annotation is occluded by the annotations of its own scene only.  One thread per window pixel.
//   sdfr_synth_shade    per annotation a half-open box inside its window: the RGB bytes of the owner's winning triangle shaded with its
//                       interpolated vertex normal, the scene's background elsewhere.  An init launch (flag words), one thread per box pixel,
//                       then a launch that zeroes the pixels of annotations whose flag says invalid -- the launches of sdfr_crop_export.
//
// No float atomics (the only atomic is an integer or on the flag words), no host synchronisation: the same bits on every run, and a crop's
// bytes depend on its own scene only.  Compiled with -ffp-contract=off (build.sh).
#include "sdfr_common.h"
#include "synth_cells.h"

namespace {

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_synth_owner_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ depth,
                                                                      const int32_t* __restrict__ windows, const int64_t* __restrict__ poff,
                                                                      int64_t P, const int32_t* __restrict__ scene, int B, int W, int H,
                                                                      int32_t* __restrict__ owner) {
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
    owner[i] = synth_owner_pixel(mask, depth, windows, poff, P, scene, B, W, H, b, i, w[0] + (int)(local % ww), w[1] + (int)(local / ww));
}

// flag words: 0, or VERIFY_FLAG_INVALID for an annotation whose window, box, offsets and scene do not fit (a kernel, not a memset: every
// entry point may be captured into a graph, sdfr_common.h)
__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_synth_init_kernel(SynthArgs a, int32_t* __restrict__ flags) {
    const int b = blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (b < a.B) flags[b] = synth_anno_ok(&a, b) ? 0 : VERIFY_FLAG_INVALID;
}

__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_synth_shade_kernel(SynthArgs a, const int32_t* __restrict__ triangle,
                                                                      const int32_t* __restrict__ owner, uint8_t* __restrict__ rgb,
                                                                      int32_t* __restrict__ flags) {
    const int64_t g = (int64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (g >= a.Q) return;
    uint8_t out[3];
    int b;
    const int raise = synth_shade_pixel(&a, triangle, owner, g, out, &b);
    if (raise) atomicOr(&flags[b], raise);                                                  // b is a usable annotation whenever a flag is raised
    rgb[3 * g] = out[0], rgb[3 * g + 1] = out[1], rgb[3 * g + 2] = out[2];
}

// after the shading: the pixels of an annotation whose flag word says invalid are zeroed (a bad triangle index is found by one pixel only)
__global__ __launch_bounds__(VERIFY_BLOCK) void sdfr_synth_scrub_kernel(SynthArgs a, const int32_t* __restrict__ flags, uint8_t* __restrict__ rgb) {
    const int64_t g = (int64_t)blockIdx.x * VERIFY_BLOCK + threadIdx.x;
    if (g >= a.Q) return;
    const int b = verify_owner(a.qoff, a.B, g);
    if (!(flags[b] & VERIFY_FLAG_INVALID)) return;
    rgb[3 * g] = rgb[3 * g + 1] = rgb[3 * g + 2] = 0;
}

unsigned synth_blocks(int64_t n) { return (unsigned)((n + VERIFY_BLOCK - 1) / VERIFY_BLOCK); }

}  // namespace

extern "C" int sdfr_synth_owner(const uint8_t* mask, const float* depth, const int32_t* windows, const int64_t* poff, int64_t P, const int32_t* scene,
                                int B, int W, int H, int32_t* owner, void* stream) {
    SDFR_REQUIRE(B >= 0 && W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31), "sdfr_synth_owner: B = %d, image %d x %d", B, W, H);
    SDFR_REQUIRE(P >= 0 && P <= (int64_t)B * W * H, "sdfr_synth_owner: P = %lld out of range (P <= B W H)", (long long)P);
    if (B == 0 || P == 0) return SDFR_OK;
    SDFR_REQUIRE(mask && depth && windows && poff && owner, "sdfr_synth_owner: NULL pointer");
    hipLaunchKernelGGL(sdfr_synth_owner_kernel, dim3(synth_blocks(P)), dim3(VERIFY_BLOCK), 0, (hipStream_t)stream, mask, depth, windows, poff, P, scene, B,
                       W, H, owner);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_synth_shade(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const float* normals, const int64_t* voff,
                                const int64_t* toff, const int32_t* windows, const int64_t* poff, int64_t P, const int32_t* triangle,
                                const int32_t* owner, const int32_t* scene, const int32_t* boxes, const int64_t* qoff, int64_t Q, const double* paint,
                                const double* light, int S, const int32_t* bg_index, const uint8_t* bg, int NBG, const int32_t* ramp, int B, int W,
                                int H, const double* K, float z_min, uint8_t* rgb, int32_t* flags, void* stream) {
    SDFR_REQUIRE(B >= 0 && W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31), "sdfr_synth_shade: B = %d, image %d x %d", B, W, H);
    SDFR_REQUIRE(V >= 0 && T >= 0 && P >= 0 && Q >= 0 && T < ((int64_t)1 << 31) && V < ((int64_t)1 << 31) && P <= (int64_t)B * W * H && Q <= P,
                 "sdfr_synth_shade: V = %lld, T = %lld, P = %lld, Q = %lld out of range (Q <= P <= B W H)", (long long)V, (long long)T, (long long)P,
                 (long long)Q);
    SDFR_REQUIRE(K && K[0] == K[0] && K[1] == K[1] && K[2] == K[2] && K[3] == K[3], "sdfr_synth_shade: the intrinsics are NULL or NaN");
    SDFR_REQUIRE(z_min >= 0.0f, "sdfr_synth_shade: z_min must not be negative");
    SDFR_REQUIRE(S >= 0 && NBG >= 0 && (NBG == 0 || (bg && bg_index)), "sdfr_synth_shade: S = %d scenes, %d background images without the images or their index table", S, NBG);
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(S >= 1, "sdfr_synth_shade: annotations without a scene (S = 0)");
    SDFR_REQUIRE(voff && toff && windows && poff && boxes && qoff && flags && paint && light && ramp, "sdfr_synth_shade: NULL pointer");
    SDFR_REQUIRE((V == 0 || (vertices && normals)) && (T == 0 || faces), "sdfr_synth_shade: NULL mesh");
    SDFR_REQUIRE((P == 0 || (triangle && owner)) && (Q == 0 || rgb), "sdfr_synth_shade: NULL triangle image, owner image or output");
    SynthArgs a;
    static_cast<CropArgs&>(a) = {raster_args(vertices, V, faces, T, voff, toff, windows, poff, P, B, W, H, K, z_min), nullptr, boxes, qoff, Q};
    a.normals = normals, a.scene = scene, a.paint = paint, a.light = light, a.bg_index = NBG ? bg_index : nullptr, a.bg = bg, a.ramp = ramp;
    a.S = S, a.NBG = NBG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sdfr_synth_init_kernel, dim3(synth_blocks(B)), dim3(VERIFY_BLOCK), 0, s, a, flags);
    SDFR_LAUNCH_CHECK();
    if (Q > 0) {
        hipLaunchKernelGGL(sdfr_synth_shade_kernel, dim3(synth_blocks(Q)), dim3(VERIFY_BLOCK), 0, s, a, triangle, owner, rgb, flags);
        SDFR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sdfr_synth_scrub_kernel, dim3(synth_blocks(Q)), dim3(VERIFY_BLOCK), 0, s, a, (const int32_t*)flags, rgb);
        SDFR_LAUNCH_CHECK();
    }
    return SDFR_OK;
}
