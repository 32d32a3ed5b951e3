// Slot arithmetic of the band Jacobian's K compaction (16-row float32 mask-fed kernel, mlp_kernel.h KCJ), shared by the kernel
// and by the host emulation under tests/kcj_host/.
//
// The operand of a transposed product is g (.) mask: exactly +0 wherever the ReLU mask of the layer is 0.  A feature whose mask bit is 0 in
// all 16 rows of the tile contributes fma(+-0, acc) == acc to every accumulator (acc starts at +0 and can never become -0), so the product
// may skip it.  A wave owns 128 consecutive k of the operand it writes (feature tiles f = 0..7 of 16).  The full chain of the 16-row kernels
// visits k = 16 t + 4 g + s in the order (tile t, component s, lane group g); inside the wave that is position c = 4 q + g with q = 4 f + i,
// the lane's accumulator register (feature fbase + 16 f + 4 g + i).  The wave's survivors are the set bits of four words, w[g] bit q.
// With `off` survivors in the waves in front, the survivor of rank r sits at chain position pos = off + r of the compacted operand: k tile
// pos / 16, component (pos % 16) / 4, lane group pos % 4 -- the place at which the full chain would visit a feature there.  The operand
// keeps its layout act[k / 4][point][k % 4]; the k list (one int4 per k tile and lane group: the four components' rows in the k-major
// weight image) says which weights a slot meets.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDFR_KCJ_HD __host__ __device__ __forceinline__
#else
#define SDFR_KCJ_HD inline
#endif

constexpr int SDFR_KCJ_PT = 16;          // points of a tile
constexpr int SDFR_KCJ_KT = 16;          // k per k tile (4 lane groups x 4 components)
constexpr int SDFR_KCJ_RING = 4;         // weight fragment stages of the product loop = k tiles per trip

SDFR_KCJ_HD int sdfr_kcj_popc(uint32_t x) { return __builtin_popcount(x); }
SDFR_KCJ_HD int sdfr_kcj_count(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    return sdfr_kcj_popc(w0) + sdfr_kcj_popc(w1) + sdfr_kcj_popc(w2) + sdfr_kcj_popc(w3);
}
// survivors of the wave in front of chain position 4 q + g (q < 32, g < 4)
SDFR_KCJ_HD int sdfr_kcj_rank(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int q, int g) {
    const uint32_t below = (uint32_t)((1ull << q) - 1ull);
    int r = sdfr_kcj_popc(w0 & below) + sdfr_kcj_popc(w1 & below) + sdfr_kcj_popc(w2 & below) + sdfr_kcj_popc(w3 & below);
    if (g > 0) r += (int)((w0 >> q) & 1u);
    if (g > 1) r += (int)((w1 >> q) & 1u);
    if (g > 2) r += (int)((w2 >> q) & 1u);
    return r;
}
// feature (offset in the wave's block of 128) of register q of lane group g
SDFR_KCJ_HD int sdfr_kcj_feature(int q, int g) { return (q >> 2) * 16 + 4 * g + (q & 3); }
// chain position -> 16-byte vector of the operand (k tile, lane group) and component inside it
SDFR_KCJ_HD int sdfr_kcj_vec(int pos) { return (pos >> 4) * 4 + (pos & 3); }
SDFR_KCJ_HD int sdfr_kcj_comp(int pos) { return (pos & 15) >> 2; }
// ... -> float index of the operand act[vector][point][component], and int index of the k list [vector][component]
SDFR_KCJ_HD int sdfr_kcj_elem(int pos, int point) { return (sdfr_kcj_vec(pos) * SDFR_KCJ_PT + point) * 4 + sdfr_kcj_comp(pos); }
SDFR_KCJ_HD int sdfr_kcj_kidx(int pos) { return sdfr_kcj_vec(pos) * 4 + sdfr_kcj_comp(pos); }
// the layer's K extent: survivors padded with zero operand rows (k list entry 0) to whole trips of the product loop, at least one
SDFR_KCJ_HD int sdfr_kcj_padded(int tot) {
    const int trip = SDFR_KCJ_KT * SDFR_KCJ_RING;
    const int p = (tot + trip - 1) / trip * trip;
    return p < trip ? trip : p;
}
// the k tiles the product EXECUTES (gemm_kcj; host emulation: tests/kc_tail_host): ceil(tot / 16), at least one.  The operand, the k list
// and the ring's gathers keep the padded extent; the tiles behind the last live one would only add fma(+0, w, acc).  Whole trips run in the
// ring loop, the remaining 0 to 3 tiles behind its exit from the stages the ring has already filled: tail tile u sits in stage u.
SDFR_KCJ_HD int sdfr_kcj_tiles(int tot) { return tot <= SDFR_KCJ_KT ? 1 : (tot + SDFR_KCJ_KT - 1) / SDFR_KCJ_KT; }
SDFR_KCJ_HD int sdfr_kcj_padded_tiles(int tot) { return sdfr_kcj_padded(tot) / SDFR_KCJ_KT; }   // what the loop ran before the tail (SDFR_KC_TAIL=0)
SDFR_KCJ_HD int sdfr_kcj_trip_tiles(int tiles) { return tiles / SDFR_KCJ_RING * SDFR_KCJ_RING; }
SDFR_KCJ_HD int sdfr_kcj_tail_tiles(int tiles) { return tiles % SDFR_KCJ_RING; }
// padding: element e of the pad block (16 points per slot) -> chain position and point
SDFR_KCJ_HD int sdfr_kcj_pad_pos(int tot, int e) { return tot + e / SDFR_KCJ_PT; }
SDFR_KCJ_HD int sdfr_kcj_pad_point(int e) { return e % SDFR_KCJ_PT; }

// The k-major weight image: per layer and out-feature k one row of HP in-features; inside a wave's block of 128 in-features the eight values
// a lane feeds to its eight feature tiles (in-features fbase + 16 f + lp) are contiguous -- column fbase + 8 lp + f: two 16-byte loads per
// lane and component, 16 lanes of a lane group on 512 contiguous bytes.
SDFR_KCJ_HD int sdfr_kcj_col(int j) { return (j & ~127) | ((j & 15) << 3) | ((j >> 4) & 7); }

// The ring of the product loop: nkt k tiles, a multiple of SDFR_KCJ_RING.  In front of tile t's matrix instructions: the weights of tile
// t + RING - 1 are gathered into stage (t + RING - 1) % RING (their k-list words were read one tile earlier), the operand of tile t + 1 is
// read, and the k-list words of tile t + RING are read.  Tile indices beyond the last are clamped to it: the tail re-reads the last tile
// into registers nobody consumes, and the loop has no branch.
SDFR_KCJ_HD int sdfr_kcj_ring_clamp(int tile, int nkt) { return tile < nkt ? tile : nkt - 1; }
SDFR_KCJ_HD int sdfr_kcj_ring_gather_tile(int t, int nkt) { return sdfr_kcj_ring_clamp(t + SDFR_KCJ_RING - 1, nkt); }
SDFR_KCJ_HD int sdfr_kcj_ring_klist_tile(int t, int nkt) { return sdfr_kcj_ring_clamp(t + SDFR_KCJ_RING, nkt); }
SDFR_KCJ_HD int sdfr_kcj_ring_operand_tile(int t, int nkt) { return sdfr_kcj_ring_clamp(t + 1, nkt); }
