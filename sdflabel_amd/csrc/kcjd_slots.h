// Chain-order survivor words of the band Jacobian's K compaction (mlp_kernel.h KCJ, the stage between two products; kcj_slots.h has the slot
// rule itself), shared by the kernel and by the host emulation under tests/kcjd_host/.
//
// kcj_slots.h names a wave's survivors by four words, w[g] bit q (lane group g, accumulator register q), and a survivor's place by the
// number of survivors in front of chain position c = 4 q + g.  Counted from w[] that is a running count over q of four bit tests plus the
// lane groups in front -- wave-uniform scalar work in front of every one of a lane's 32 stores.  Here the same 128 bits are kept in CHAIN
// order: word j = c / 32, bit c % 32, i.e. c[j] bit 4 (q % 8) + g = w[g] bit 8 j + q % 8.  The survivors in front of a position are then the
// set bits of the words in front of its own (three wave-uniform sums per layer) plus one masked population count of its own word: a lane
// takes a register's position with a handful of vector instructions and no scalar chain.  The positions are those of sdfr_kcj_rank, bit for bit.
#pragma once
#include "kcj_slots.h"

// bits 0 .. 7 of `byte` to bits 0, 4, .. 28
SDFR_KCJ_HD uint32_t sdfr_kcjd_spread8(uint32_t byte) {
    uint32_t s = byte & 0xFFu;
    s = (s | (s << 12)) & 0x000F000Fu;
    s = (s | (s << 6)) & 0x03030303u;
    s = (s | (s << 3)) & 0x11111111u;
    return s;
}
// what lane group g adds to chain word j from its survivor word w
SDFR_KCJ_HD uint32_t sdfr_kcjd_group_part(uint32_t w, int j, int g) { return sdfr_kcjd_spread8(w >> (8 * j)) << g; }
// chain word j (0 .. 3) of the wave
SDFR_KCJ_HD uint32_t sdfr_kcjd_chain_word(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int j) {
    return sdfr_kcjd_group_part(w0, j, 0) | sdfr_kcjd_group_part(w1, j, 1) | sdfr_kcjd_group_part(w2, j, 2) | sdfr_kcjd_group_part(w3, j, 3);
}
// survivors of the wave in front of chain position 4 q + g, given `front` = the set bits of the chain words in front of word q / 8 and
// `word` = chain word q / 8 (what sdfr_kcj_rank returns)
SDFR_KCJ_HD int sdfr_kcjd_rank_in_word(uint32_t word, int front, int q, int g) {
    const int bit = 4 * (q & 7) + g;
    return front + sdfr_kcj_popc(word & ((1u << bit) - 1u));
}
SDFR_KCJ_HD int sdfr_kcjd_rank(const uint32_t c[4], int q, int g) {
    int front = 0;
    for (int j = 0; j < (q >> 3); ++j) front += sdfr_kcj_popc(c[j]);
    return sdfr_kcjd_rank_in_word(c[q >> 3], front, q, g);
}
// Where a lane stores a register that did NOT survive, so that the 32 stores of a stage need no predicate: a dead feature's operand is
// exactly +0 in all 16 rows (it is g (.) mask), and chain position min(tot, 511) either is the first padding slot, which holds +0 anyway
// (tot < padded), or lies behind the K extent the product walks (tot == padded < 512); with tot == 512 no register is dead.
SDFR_KCJ_HD int sdfr_kcjd_dead_pos(int tot) { return tot < 511 ? tot : 511; }
