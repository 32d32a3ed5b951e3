// Decoder forward on the grid, float32, padded hidden width 512 -- the dominant kernel of the whole path, compiled alone.
// Geometry macros (tools/ab_build.sh A/B builds): SDFR_FWD_FT feature tiles per wave, SDFR_FWD_NW waves (FT*NW = 16), SDFR_FWD_NP point
// tiles (32 points each) per workgroup, weight-fragment ring SDFR_FWD_PF, activation-fragment ring SDFR_FWD_PFB.
#include "mlp_kernel.h"
#include <stdlib.h>
#ifndef SDFR_FWD_PF
#define SDFR_FWD_PF 2
#endif
#ifndef SDFR_FWD_PFB
#define SDFR_FWD_PFB 2
#endif
#ifndef SDFR_FWD_FT
#define SDFR_FWD_FT 2
#define SDFR_FWD_NW 8
#define SDFR_FWD_NP 2
#endif
#ifndef SDFR_FWD_TILE_DEFAULT
#define SDFR_FWD_TILE_DEFAULT 64      // measured (profiles/fwd32_tiles_notes.md): the 32-row geometry is the slower one, the weight gathers bind it
#endif
int sdfr_fwd_f32_512_np() { return SDFR_FWD_NP; }
void sdfr_launch_fwd_f32_512(const MlpParams& P, int64_t n, bool save_masks, hipStream_t s) {
    static_assert(SDFR_FWD_FT * SDFR_FWD_NW == 16, "padded width 512 = 32 * FT * NW");
    // one instantiation serves both cases: without a mask buffer the mask-saving kernel skips its stores (measured 1.78 ms against 1.93 ms
    // of a separate no-mask instantiation -- the compiler's schedule for that one is simply worse)
    (void)save_masks;
    // per-tile K compaction (mlp_kernel.h, KC) is on by default; SDFR_FWD_COMPACT=0 in the environment, read at every launch, runs the full
    // K chain instead (same bits: A/B timing and the parity tests)
    MlpParams Q = P;
    const char* e = getenv("SDFR_FWD_COMPACT");
    if (e && e[0] == '0') Q.kcompact = 0;
    // Two tile geometries, same bits per row (sdf and mask words): the 64-row tiles with one workgroup per CU (the default),
    // and 32-row tiles, 64 KiB of operand, TWO workgroups resident per CU -- one tile's K loop runs under the other's epilogue and barriers
    // (mlp_kernel.h, KC2).  SDFR_FWD_TILE=64 / 32 in the environment, read at every launch, selects one (A/B timing and the parity tests).
    int tile = SDFR_FWD_TILE_DEFAULT;
    const char* t = getenv("SDFR_FWD_TILE");
    if (t && t[0] == '6' && t[1] == '4' && !t[2]) tile = 64;
    else if (t && t[0] == '3' && t[1] == '2' && !t[2]) tile = 32;
    if (tile == 32) {
        hipLaunchKernelGGL((sdfr_mlp_kernel<float, 32, 2, 1, 8, 2, 1, 2>), dim3(sdfr_cdiv(n, 32)), dim3(512), 0, s, Q);
        return;
    }
    const int grid = sdfr_cdiv(n, 32 * SDFR_FWD_NP);
    hipLaunchKernelGGL((sdfr_mlp_kernel<float, 32, SDFR_FWD_FT, SDFR_FWD_NP, SDFR_FWD_NW, SDFR_FWD_PF, 1, SDFR_FWD_PFB>), dim3(grid),
                       dim3(64 * SDFR_FWD_NW), 0, s, Q);
}
