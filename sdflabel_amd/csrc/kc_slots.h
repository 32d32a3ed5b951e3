// Slot arithmetic of the KC epilogue (per-tile K compaction of the exact-f32 grid forward, mlp_kernel.h), shared by the kernel
// and by the host emulation under tests/kc_epilogue_host/.
//
// A wave owns 64 consecutive k of the layer it writes.  The full K chain visits them in the order c = 2 q + g (accumulator register
// q = 0..31, lane group g): the wave's survivors are the set bits of two words, w[g] bit q.  With `off` survivors in the waves in front, the
// survivor of rank r sits at chain position pos = off + r of the compacted operand: k tile pos / 8, and inside the tile 16-byte vector
// pos % 2 (the lane group that feeds it to the product), component (pos % 8) / 2.  The operand image is act[vector][point] (16 bytes each).
//
// A lane of lane group g holds register q's value at its points; it stores each survivor with 4-byte stores at sdfr_kc_slot(off + rank).
// (The 32-row kernel.  The 64-row kernels keep this rule for the k list and hold the values in the k-major image at the end of this file;
// its host emulation is tests/kc_kmajor_host/.)
#pragma once
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDFR_KC_HD __host__ __device__ __forceinline__
#else
#define SDFR_KC_HD inline
#endif

SDFR_KC_HD int sdfr_kc_popc(uint32_t x) { return __builtin_popcount(x); }
// chain position -> operand slot (float index inside a point's compacted row: vector slot / 4, component slot % 4)
SDFR_KC_HD int sdfr_kc_slot(int pos) { return (pos & ~7) | ((pos & 1) * 4) | ((pos & 7) >> 1); }
// survivors of the wave in front of chain position 2 q + g
SDFR_KC_HD int sdfr_kc_rank(uint32_t w0, uint32_t w1, int q, int g) {
    return sdfr_kc_popc(w0 & (uint32_t)((1ull << (q + g)) - 1ull)) + sdfr_kc_popc(w1 & (uint32_t)((1ull << q) - 1ull));
}
// the layer's K extent: survivors padded with zero activations (k list entry 0) to a multiple of two k tiles; the LAST wave pads
SDFR_KC_HD int sdfr_kc_padded(int tot) { return (tot + 15) & ~15; }
SDFR_KC_HD bool sdfr_kc_pads(int wave, int n_waves) { return wave == n_waves - 1; }

// The k-major image of the compacted operand (64-row tiles: two point tiles of 32).  The chain order, the ranks and the k list are the ones
// above; only the place where a survivor's values wait for the product differs.  The survivor at chain position pos owns ROW pos of the
// image, 64 dwords: point p 32 + lp at dword 2 lp + p, so the two points a lane holds of one feature are neighbours -- one 8-byte store per
// lane and survivor, 16 lanes cover 32 consecutive dwords.  The product's lane (lp, lg) reads, for k tile t and step ks, the same 8 bytes of
// row 8 t + 2 ks + lg: the position at which the full chain visits (tile, component, lane group).
SDFR_KC_HD int sdfr_kcm_dword(int pos, int point) { return pos * 64 + 2 * (point & 31) + (point >> 5); }
// first dword of the 8 bytes lane lp stores to / reads from row `row`
SDFR_KC_HD int sdfr_kcm_lane_dword(int row, int lp) { return row * 64 + 2 * lp; }
SDFR_KC_HD int sdfr_kcm_read_row(int t, int ks, int lg) { return 8 * t + 2 * ks + lg; }
// padding: rows [tot, padded) are one block of at most 15 x 256 bytes, zeroed by WAVE 0 with four 16-byte stores per lane at most: store i
// of lane `lane` covers 16-byte vector sdfr_kcm_pad_vec of the image when that lies below 16 padded; lane e < padded - tot enters pad k e
SDFR_KC_HD bool sdfr_kcm_pads(int wave) { return wave == 0; }
SDFR_KC_HD int sdfr_kcm_pad_vec(int tot, int i, int lane) { return tot * 16 + i * 64 + lane; }
constexpr int SDFR_KCM_PAD_STORES = 4;

// The ring of the compacted product loop (gemm_kc_body of the 64-row kernels; host emulation: tests/kc_ring_host).  A layer has nkt k tiles,
// an even number >= 2 (sdfr_kc_padded).  Tile t is consumed in four chain steps c = 4 t + ks, one per operand component ks, each a group of
// matrix instructions that reads component ks of the tile's weight fragments.  The fragments have TWO stages (tile t in stage t % 2), and a
// stage is refilled component by component: right behind chain step (t, ks) the gather of (t + 2, ks) is issued into the registers that step
// has just read, so that a gather has seven chain steps of lead (1.75 tiles of matrix work; the whole-tile ring gave it four) at no register
// more.  The k-list words a gather needs have two stages as well: stage t % 2 holds tile t + 2's words while tile t is consumed and reads
// tile t + 4's behind the tile's last gather; the operand (LDS) of tile t + 1 is read in front of tile t.  Tile indices beyond the last are
// clamped to it: the tail re-reads the last tile into registers nobody consumes, and the loop (two tiles per trip) has no branch.  Prologue:
// k list 0 and 1, all gathers of tiles 0 and 1, operand 0, then k list 2 and 3.
constexpr int SDFR_KC_RING_STAGES = 2, SDFR_KC_RING_LEAD = 2;      // fragment stages; a gather runs this many tiles ahead of its chain step
SDFR_KC_HD int sdfr_kc_ring_clamp(int tile, int nkt) { return tile < nkt ? tile : nkt - 1; }
constexpr int sdfr_kc_ring_stage(int t) { return t % SDFR_KC_RING_STAGES; }
// behind chain step (t, ks): the tile whose component ks is gathered into stage sdfr_kc_ring_stage(t), from k-list stage sdfr_kc_ring_stage(t)
SDFR_KC_HD int sdfr_kc_ring_gather_tile(int t, int nkt) { return sdfr_kc_ring_clamp(t + SDFR_KC_RING_LEAD, nkt); }
// behind tile t's last gather: the tile whose k-list words k-list stage sdfr_kc_ring_stage(t) reads
SDFR_KC_HD int sdfr_kc_ring_klist_tile(int t, int nkt) { return sdfr_kc_ring_clamp(t + 2 * SDFR_KC_RING_LEAD, nkt); }
// in front of tile t: the tile whose operand is read into operand stage sdfr_kc_ring_stage(t + 1)
SDFR_KC_HD int sdfr_kc_ring_operand_tile(int t, int nkt) { return sdfr_kc_ring_clamp(t + 1, nkt); }
