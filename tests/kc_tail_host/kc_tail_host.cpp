// Host emulation of the compacted products with their tails (csrc/kc_slots.h: sdfr_kc_steps and the sdfr_kc_ring_* rule, mlp_kernel.h
// gemm_kc_body of the 64-row kernels; csrc/kcj_slots.h: sdfr_kcj_tiles and the sdfr_kcj_ring_* rule, mlp_kernel.h gemm_kcj): one wave's
// prologue, ring loop over the whole trips and tail, with the headers' own arithmetic, for every survivor total 0 .. 512 and with the tail
// on and off (off: the loop runs the whole padded extent, SDFR_KC_TAIL=0).  The k list is built as the epilogues build it -- the survivor at
// chain position pos < tot enters the word pos at its slot, the pad entries [tot, padded) enter PAD -- and is an array of EXACTLY the padded
// extent, as is the operand: an index beyond it is an error under the sanitizers.  What the emulated registers hold is a tag carried through
// the k list (the tile the words were read from) and the words themselves.  One record of eight int32 per consumed group of matrix
// instructions:
//     kernel (0 forward, 1 Jacobian), tail (0 / 1), tot, lane group, tile the loop is at, tile the fragment was gathered for,
//     component (Jacobian: tile the operand was read for), k word the lane group meets (Jacobian: component 0's)
// The forward consumes one chain step (tile, component) per record; the Jacobian a whole k tile, one record per lane group.  The program
// counts what it sees wrong itself ("bad"); tests/test_kc_tail_cpu.py checks the log against the rule restated there.
//   kc_tail_host out.bin
#include "kc_slots.h"
#include "kcj_slots.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace {
constexpr int PAD = -1, NONE = -2;
struct Log {
    std::vector<int32_t> rec;
    void add(int kernel, int tail, int tot, int lg, int at, int frag, int comp, int word) {
        const int32_t r[8] = {kernel, tail, tot, lg, at, frag, comp, word};
        rec.insert(rec.end(), r, r + 8);
    }
};

// ---- grid forward: k tiles of 8 (4 components x 2 lane groups), trips of two tiles, fragments refilled component by component
int forward(int tot, int tail, int lg, Log& log) {
    int bad = 0;
    const int padded = sdfr_kc_padded(tot), nkt = padded / 8;
    if (nkt <= 0) return 0;                                           // (the kernel: gemm_kc zeroes the accumulators, the body returns)
    std::vector<int> klist(padded);                                   // exact size
    for (int pos = 0; pos < padded; ++pos) klist[sdfr_kc_slot(pos)] = pos < tot ? pos : PAD;
    struct Words { int tile; int w[4]; };
    auto read_klist = [&](int tile) {                                 // the int4 of (tile, lane group)
        Words k;
        k.tile = tile;
        for (int c = 0; c < 4; ++c) k.w[c] = klist[(tile * 2 + lg) * 4 + c];
        return k;
    };
    Words ko[2];
    int frag_tile[2][4], frag_word[2][4];
    auto gather = [&](int s, int c) { frag_tile[s][c] = ko[s].tile; frag_word[s][c] = ko[s].w[c]; };
    auto step = [&](int at, int s, int c) {
        if (frag_tile[s][c] != at) ++bad;                             // the chain step reads the fragment gathered for its own tile
        log.add(0, tail, tot, lg, at, frag_tile[s][c], c, frag_word[s][c]);
        frag_tile[s][c] = NONE;                                       // consumed
    };
    ko[0] = read_klist(0);
    ko[1] = read_klist(sdfr_kc_ring_clamp(1, nkt));
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 4; ++c) gather(s, c);
    ko[0] = read_klist(sdfr_kc_ring_clamp(2, nkt));
    ko[1] = read_klist(sdfr_kc_ring_clamp(3, nkt));
    const int steps = tail ? sdfr_kc_steps(tot) : sdfr_kc_padded_steps(tot);
    const int ntrip = sdfr_kc_trip_tiles(steps);
    for (int t = 0; t < ntrip; t += SDFR_KC_RING_STAGES)
        for (int u = 0; u < SDFR_KC_RING_STAGES; ++u) {
            const int s = sdfr_kc_ring_stage(u);
            for (int c = 0; c < 4; ++c) {
                step(t + u, s, c);
                if (ko[s].tile != sdfr_kc_ring_gather_tile(t + u, nkt)) ++bad;
                gather(s, c);
            }
            ko[s] = read_klist(sdfr_kc_ring_klist_tile(t + u, nkt));
        }
    const int rem = sdfr_kc_tail_steps(steps);
    for (int i = 0; i < SDFR_KC_TRIP_STEPS - 1; ++i)
        if (rem > i) step(ntrip + i / SDFR_KC_TILE_STEPS, i / SDFR_KC_TILE_STEPS, i % SDFR_KC_TILE_STEPS);
    return bad;
}

// ---- band Jacobian: k tiles of 16 (4 components x 4 lane groups), trips of four tiles, whole-tile fragments three tiles ahead
int jacobian(int tot, int tail, int lg, Log& log) {
    int bad = 0;
    const int padded = sdfr_kcj_padded(tot), nkt = padded / SDFR_KCJ_KT;
    std::vector<int> klist(padded), operand(nkt * 4);                 // exact sizes; operand: one tag per 16-byte vector (tile, lane group)
    for (int pos = 0; pos < padded; ++pos) klist[sdfr_kcj_kidx(pos)] = pos < tot ? pos : PAD;
    for (int t = 0; t < nkt; ++t)
        for (int g = 0; g < 4; ++g) operand[t * 4 + g] = t;
    struct Words { int tile; int w[4]; };
    auto read_klist = [&](int tile) {
        Words k;
        k.tile = tile;
        for (int c = 0; c < 4; ++c) k.w[c] = klist[(tile * 4 + lg) * 4 + c];
        return k;
    };
    constexpr int R = SDFR_KCJ_RING;
    Words a[R];
    int b[2] = {NONE, NONE};
    for (int s = 0; s < R; ++s) a[s].tile = NONE;
    auto tile = [&](int at, int s, int bs) {
        if (a[s].tile != at || b[bs] != at) ++bad;                    // its own tile's weights and operand
        for (int c = 1; c < 4; ++c)
            if (a[s].w[c] != (16 * at + 4 * c + lg < tot ? 16 * at + 4 * c + lg : PAD)) ++bad;
        log.add(1, tail, tot, lg, at, a[s].tile, b[bs], a[s].w[0]);
        a[s].tile = NONE;
    };
    Words ko = read_klist(0);
    for (int u = 0; u < R - 1; ++u) {
        a[u] = ko;
        ko = read_klist(sdfr_kcj_ring_clamp(u + 1, nkt));
    }
    b[0] = operand[0 * 4 + lg];
    const int tiles = tail ? sdfr_kcj_tiles(tot) : sdfr_kcj_padded_tiles(tot);
    const int ntrip = sdfr_kcj_trip_tiles(tiles);
    for (int t = 0; t < ntrip; t += R)
        for (int u = 0; u < R; ++u) {
            if (ko.tile != sdfr_kcj_ring_gather_tile(t + u, nkt)) ++bad;
            a[(u + R - 1) % R] = ko;
            b[(u + 1) % 2] = operand[sdfr_kcj_ring_operand_tile(t + u, nkt) * 4 + lg];
            ko = read_klist(sdfr_kcj_ring_klist_tile(t + u, nkt));
            tile(t + u, u, u % 2);
        }
    const int rem = sdfr_kcj_tail_tiles(tiles);
    for (int u = 0; u < R - 1; ++u)
        if (rem > u) {
            if (u + 1 < R - 1) b[(u + 1) % 2] = operand[(ntrip + u + 1) * 4 + lg];
            tile(ntrip + u, u, u % 2);
        }
    return bad;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: kc_tail_host out.bin\n"); return 2; }
    Log log;
    int bad = 0, cases = 0;
    for (int tot = 0; tot <= 512; ++tot)
        for (int tail = 0; tail < 2; ++tail) {
            for (int lg = 0; lg < 2; ++lg) bad += forward(tot, tail, lg, log);
            for (int lg = 0; lg < 4; ++lg) bad += jacobian(tot, tail, lg, log);
            ++cases;
        }
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    const size_t n = std::fwrite(log.rec.data(), sizeof(int32_t), log.rec.size(), f);
    std::fclose(f);
    if (n != log.rec.size()) return 4;
    std::printf("cases %d bad %d\n", cases, bad);
    return bad ? 1 : 0;
}
