// Slot arithmetic of the KC epilogue (per-tile K compaction of the exact-f32 grid forward, mlp_kernel.h), shared by the kernel
// and by the host emulation under tests/kc_epilogue_host/.
//
// A wave owns 64 consecutive k of the layer it writes.  The full K chain visits them in the order c = 2 q + g (accumulator register
// q = 0..31, lane group g): the wave's survivors are the set bits of two words, w[g] bit q.  With `off` survivors in the waves in front, the
// survivor of rank r sits at chain position pos = off + r of the compacted operand: k tile pos / 8, and inside the tile 16-byte vector
// pos % 2 (the lane group that feeds it to the product), component (pos % 8) / 2.  The operand image is act[vector][point] (16 bytes each).
//
// A lane of lane group g holds register q's value at its points; it stores each survivor with 4-byte stores at sdfr_kc_slot(off + rank).
// (No kernel writes this compacted value image any more; tests/kc_epilogue_host still walks it.  Its slot, rank and padding rule remains
// the k list's: the kernels enter a survivor's k word at sdfr_kc_slot(off + rank) and hold the values of EVERY feature in the dense k-major
// image at the end of this file, whose host emulation is tests/kc_dense_host/.)
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
// the layer's K extent: survivors padded with zero activations to a multiple of two k tiles (the kernels: sdfr_kcd_pad_entry, entered by
// sdfr_kcm_pads' wave).  The compacted value image of tests/kc_epilogue_host: k list entry 0, zeros stored by the LAST wave
SDFR_KC_HD int sdfr_kc_padded(int tot) { return (tot + 15) & ~15; }
SDFR_KC_HD bool sdfr_kc_pads(int wave, int n_waves) { return wave == n_waves - 1; }
// the chain steps the product EXECUTES (gemm_kc_body, full-width waves; host emulation: tests/kc_tail_host): chain step ks of k tile t reads
// the positions 8 t + 2 ks and 8 t + 2 ks + 1 (component ks of both lane groups), so `tot` survivors are covered by ceil(tot / 2) steps.  The
// k list, its pad entries and the ring's gathers keep the padded extent; the steps behind the last live one would only add fma(+0, w, acc).
// Whole trips (SDFR_KC_TRIP_STEPS steps: two k tiles) run in the ring loop, the remaining 0 to 7 behind its exit from the two stages the
// ring has already filled: step i of the tail is component i % 4 of stage i / 4.
constexpr int SDFR_KC_TILE_STEPS = 4, SDFR_KC_TRIP_STEPS = 8;
SDFR_KC_HD int sdfr_kc_steps(int tot) { return (tot + 1) >> 1; }
SDFR_KC_HD int sdfr_kc_padded_steps(int tot) { return sdfr_kc_padded(tot) >> 1; }      // what the loop ran before the tail (SDFR_KC_TAIL=0)
SDFR_KC_HD int sdfr_kc_trip_tiles(int steps) { return steps / SDFR_KC_TRIP_STEPS * 2; }  // k tiles the ring loop consumes
SDFR_KC_HD int sdfr_kc_tail_steps(int steps) { return steps % SDFR_KC_TRIP_STEPS; }

// The k-major image of the compacted operand (64-row tiles: two point tiles of 32).  The chain order, the ranks and the k list are the ones
// above; only the place where a survivor's values wait for the product differs.  The survivor at chain position pos owns ROW pos of the
// image, 64 dwords: point p 32 + lp at dword 2 lp + p, so the two points a lane holds of one feature are neighbours -- one 8-byte store per
// lane and survivor, 16 lanes cover 32 consecutive dwords.  The product's lane (lp, lg) reads, for k tile t and step ks, the same 8 bytes of
// row 8 t + 2 ks + lg: the position at which the full chain visits (tile, component, lane group).
// (Of the sdfr_kcm_* functions the kernels still use sdfr_kcm_lane_dword and sdfr_kcm_pads alone: their operand is the dense image below.
// The others stay because tests/kc_kmajor_host and tests/kc_ring_host compile them; removing them is a later change that touches those
// tests.)
SDFR_KC_HD int sdfr_kcm_dword(int pos, int point) { return pos * 64 + 2 * (point & 31) + (point >> 5); }
// first dword of the 8 bytes lane lp stores to / reads from row `row`
SDFR_KC_HD int sdfr_kcm_lane_dword(int row, int lp) { return row * 64 + 2 * lp; }
SDFR_KC_HD int sdfr_kcm_read_row(int t, int ks, int lg) { return 8 * t + 2 * ks + lg; }
// padding: rows [tot, padded) are one block of at most 15 x 256 bytes, zeroed by WAVE 0 with four 16-byte stores per lane at most: store i
// of lane `lane` covers 16-byte vector sdfr_kcm_pad_vec of the image when that lies below 16 padded; lane e < padded - tot enters pad k e
SDFR_KC_HD bool sdfr_kcm_pads(int wave) { return wave == 0; }
SDFR_KC_HD int sdfr_kcm_pad_vec(int tot, int i, int lane) { return tot * 16 + i * 64 + lane; }
constexpr int SDFR_KCM_PAD_STORES = 4;

// The ring of the compacted product loop (gemm_kc_body, full-width waves; host emulation: tests/kc_ring_host).  A layer has nkt k tiles,
// an even number >= 2 (sdfr_kc_padded).  Tile t is consumed in four chain steps c = 4 t + ks, one per operand component ks, each a group of
// matrix instructions that reads component ks of the tile's weight fragments.  The fragments have TWO stages (tile t in stage t % 2), and a
// stage is refilled component by component: right behind chain step (t, ks) the gather of (t + 2, ks) is issued into the registers that step
// has just read, so that a gather has seven chain steps of lead (1.75 tiles of matrix work; the whole-tile ring gave it four) at no register
// more.  The k-list words a gather needs have two stages as well: stage t % 2 holds tile t + 2's words while tile t is consumed and reads
// tile t + 4's behind the tile's last gather; the operand (LDS) of tile t + 1 is read in front of tile t.  Tile indices beyond the last are
// clamped to it: the tail re-reads the last tile into registers nobody consumes, and the loop (two tiles per trip) has no branch.  Prologue:
// k list 0 and 1, all gathers of tiles 0 and 1, operand 0, then k list 2 and 3.  (The operand rule of this paragraph is the compacted
// image's, which tests/kc_ring_host walks; with the dense image at the end of this file the operand travels with the weights,
// sdfr_kcd_ring_operand_tile, and the prologue reads operand 0 and 1 with the gathers.)
constexpr int SDFR_KC_RING_STAGES = 2, SDFR_KC_RING_LEAD = 2;      // fragment stages; a gather runs this many tiles ahead of its chain step
SDFR_KC_HD int sdfr_kc_ring_clamp(int tile, int nkt) { return tile < nkt ? tile : nkt - 1; }
constexpr int sdfr_kc_ring_stage(int t) { return t % SDFR_KC_RING_STAGES; }
// behind chain step (t, ks): the tile whose component ks is gathered into stage sdfr_kc_ring_stage(t), from k-list stage sdfr_kc_ring_stage(t)
SDFR_KC_HD int sdfr_kc_ring_gather_tile(int t, int nkt) { return sdfr_kc_ring_clamp(t + SDFR_KC_RING_LEAD, nkt); }
// behind tile t's last gather: the tile whose k-list words k-list stage sdfr_kc_ring_stage(t) reads
SDFR_KC_HD int sdfr_kc_ring_klist_tile(int t, int nkt) { return sdfr_kc_ring_clamp(t + 2 * SDFR_KC_RING_LEAD, nkt); }
// in front of tile t: the tile whose operand is read into operand stage sdfr_kc_ring_stage(t + 1)
SDFR_KC_HD int sdfr_kc_ring_operand_tile(int t, int nkt) { return sdfr_kc_ring_clamp(t + 1, nkt); }

// The DENSE image the kernels use (host emulation: tests/kc_dense_host).  The product needs the LIST of survivors, not their values in
// consecutive rows: it walks the k list anyway to gather its weights.  So the epilogue writes EVERY feature j of the layer to its own row j
// of the k-major image (64 dwords, sdfr_kcm_lane_dword(j, lp) = the lane's 8 bytes; dead features store their zeros) -- 32 unconditional
// 8-byte stores per lane from one address register -- and the k list, whose places, order and padding are the rule at the top of this file,
// names rows: the entry of feature j is j * 256, the byte offset of row j in the image, and 8 times that is the byte offset of k row j in
// the layer's Wk image (512 floats per row), one VALU instruction for either address.  Pad entries name the ZERO ROW, row 512: 256 bytes
// behind the image that are zeroed once per workgroup, and a row of Wk that always exists and is finite (the next layer's row 0, or the
// zero row appended behind the last layer: sdfr_kcd_wk_floats).  A pad term is fma(0, w, acc) as before.
constexpr int SDFR_KCD_ROW_BYTES = 256, SDFR_KCD_ZERO_ROW = 512, SDFR_KCD_WK_ROW_FLOATS = 512;
// feature of register q (0..31), lane group g of wave `wave`: the row its values go to
SDFR_KC_HD int sdfr_kcd_feature(int wave, int q, int g) { return wave * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3); }
SDFR_KC_HD int sdfr_kcd_row(int feature) { return feature; }
// the part of a store's row that is the same for all 32 registers of a lane (the lane's address register) and the register's constant part
SDFR_KC_HD int sdfr_kcd_row_lane(int wave, int g) { return wave * 64 + 4 * g; }
SDFR_KC_HD int sdfr_kcd_row_reg(int q) { return (q >> 4) * 32 + ((q >> 2) & 3) * 8 + (q & 3); }
SDFR_KC_HD int sdfr_kcd_entry(int feature) { return sdfr_kcd_row(feature) * SDFR_KCD_ROW_BYTES; }
SDFR_KC_HD int sdfr_kcd_pad_entry() { return SDFR_KCD_ZERO_ROW * SDFR_KCD_ROW_BYTES; }
// byte offsets the product forms from a k-list entry: the lane's 8 bytes of the operand row, and the k row of the layer's Wk image
SDFR_KC_HD uint32_t sdfr_kcd_operand_byte(int entry, int lp) { return (uint32_t)entry + 8u * (uint32_t)lp; }
SDFR_KC_HD uint32_t sdfr_kcd_weight_byte(int entry) { return (uint32_t)entry * (uint32_t)(SDFR_KCD_WK_ROW_FLOATS * 4 / SDFR_KCD_ROW_BYTES); }
// floats of Wk a layer at float offset `layer_off` needs so that its pad row exists
SDFR_KC_HD int64_t sdfr_kcd_wk_floats(int64_t layer_off) { return layer_off + (int64_t)(SDFR_KCD_ZERO_ROW + 1) * SDFR_KCD_WK_ROW_FLOATS; }
// The operand's place in the ring (sdfr_kc_ring_*): it travels WITH the weights.  Behind chain step (t, ks) the operand of
// (sdfr_kc_ring_gather_tile(t), ks) is read into operand stage sdfr_kc_ring_stage(t), component ks, from the k word the gather uses.
SDFR_KC_HD int sdfr_kcd_ring_operand_tile(int t, int nkt) { return sdfr_kc_ring_gather_tile(t, nkt); }
