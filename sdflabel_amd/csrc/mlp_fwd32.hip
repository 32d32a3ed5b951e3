// Decoder forward on the grid, float32, padded hidden width 512 -- the dominant kernel of the whole path, compiled alone.
// Geometry macros (tools/ab_variant.sh A/B builds): SDFR_FWD_FT feature tiles per wave, SDFR_FWD_NW waves (FT*NW = 16), SDFR_FWD_NP point
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
int sdfr_fwd_f32_512_np() { return SDFR_FWD_NP; }
// What the environment selects, read at every launch (A/B timing and the parity tests).
//   SDFR_FWD_COMPACT=0   the full K chain instead of the per-tile K compaction (mlp_kernel.h, KC), which is on by default; same bits
//                        (=2: see fwd_env)
static void fwd_env(MlpParams& Q) {
    const char* e = getenv("SDFR_FWD_COMPACT");
    if (e && e[0] == '0') Q.kcompact = 0;
    // (=2, tests only: the compaction even where the decoder's finite check declined it -- right only while every non-finite weight sits in
    // a k row that no survivor and no pad entry names; tests/test_gpu_kc_dense.py shows with it that the row of a dead feature is never read)
    else if (e && e[0] == '2' && Q.Wk) Q.kcompact = 1;
    //   SDFR_KC_TAIL=0       the compacted products run their whole padded extent instead of stopping behind the last chain step that holds
    //                        a survivor (kc_slots.h, sdfr_kc_steps); same bits
    const char* t = getenv("SDFR_KC_TAIL");
    if (t && t[0] == '0') Q.kc_tail = 0;
}
void sdfr_launch_fwd_f32_512(const MlpParams& P, int64_t n, bool save_masks, hipStream_t s) {
    static_assert(SDFR_FWD_FT * SDFR_FWD_NW == 16, "padded width 512 = 32 * FT * NW");
    // one instantiation serves both cases: without a mask buffer the mask-saving kernel skips its stores (measured 1.78 ms against 1.93 ms
    // of a separate no-mask instantiation -- the compiler's schedule for that one is simply worse)
    (void)save_masks;
    MlpParams Q = P;
    fwd_env(Q);
    const int grid = sdfr_cdiv(n, 32 * SDFR_FWD_NP);
    hipLaunchKernelGGL((sdfr_mlp_kernel<float, 32, SDFR_FWD_FT, SDFR_FWD_NP, SDFR_FWD_NW, SDFR_FWD_PF, 1, SDFR_FWD_PFB>), dim3(grid),
                       dim3(64 * SDFR_FWD_NW), 0, s, Q);
}
// The same kernel with the rows of a tile chosen by the caller (mlp_kernel.h, ORDER): slot j evaluates row (j / G) G + order[j % G] and
// stores value and masks at that row.  The switch above applies.  The geometry macros do not: the ordered variant exists for the shipped
// 64-row tiles.
void sdfr_launch_fwd_f32_512_ordered(const MlpParams& P, int64_t n, const int32_t* order, int64_t order_rows, hipStream_t s) {
    MlpParams Q = P;
    Q.gather_idx = order;
    Q.gather_rows = order_rows;
    fwd_env(Q);
    hipLaunchKernelGGL((sdfr_mlp_kernel<float, 32, 2, 2, 8, 2, 1, 2, false, 4>), dim3(sdfr_cdiv(n, 64)), dim3(512), 0, s, Q);
}
