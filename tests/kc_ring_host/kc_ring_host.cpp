// Host emulation of the ring of the compacted product loop (csrc/kc_slots.h, the sdfr_kc_ring_* rule; mlp_kernel.h, gemm_kc_body of the
// 64-row kernels): one wave's loop, event by event, with the header's own arithmetic.  For every even tile count nkt = 2 .. 64 it walks the
// prologue and the loop as the kernel does and writes one record of six int32 per event,
//     nkt, kind, clock, stage, component, tile
// kind 0: k-list read of `tile` into k-list stage `stage`;  1: gather of (tile, component) into fragment stage `stage`, addressed by the
// words the k-list stage of the same number holds at that moment;  2: operand read of `tile` into operand stage `stage`;  3: the matrix
// instructions of chain step (tile, component) read fragment stage `stage` and the operand stage of the same number.
// clock = the chain step 4 t + component in front of / behind which the event happens (prologue events: the clock their place in the
// rule gives them, below zero).  `tile` of kinds 1 and 3 is what the emulated registers HOLD (a tag carried through the k list, the weight
// image and the operand), not what the rule says they should hold.  The k list, the weight image and the operand are arrays of exactly nkt
// tiles: an index beyond the last tile is an error under the sanitizers.  The program counts what it sees wrong itself ("bad"), and
// tests/test_kc_ring_cpu.py checks the event log against the rule restated there.
//   kc_ring_host out.bin
#include "kc_slots.h"

#include <cstdint>
#include <cstdio>
#include <vector>

namespace {
constexpr int NS = SDFR_KC_RING_STAGES, NC = 4;

struct Log {
    std::vector<int32_t> rec;
    void add(int nkt, int kind, int clock, int stage, int comp, int tile) {
        const int32_t r[6] = {nkt, kind, clock, stage, comp, tile};
        rec.insert(rec.end(), r, r + 6);
    }
};

int run(int nkt, Log& log) {
    int bad = 0;
    std::vector<int> klist(nkt), weights(nkt), operand(nkt);          // exact size; entry t carries the tag t
    for (int t = 0; t < nkt; ++t) klist[t] = weights[t] = operand[t] = t;
    int ko[NS], a[NS][NC], b[NS], consumed_a[NS][NC], consumed_b[NS];
    for (int s = 0; s < NS; ++s) {
        ko[s] = b[s] = -1;
        consumed_b[s] = 1;
        for (int c = 0; c < NC; ++c) { a[s][c] = -1; consumed_a[s][c] = 1; }
    }
    auto read_klist = [&](int clock, int stage, int tile) {
        ko[stage] = klist[tile];
        log.add(nkt, 0, clock, stage, 0, tile);
    };
    auto gather = [&](int clock, int stage, int comp) {
        if (ko[stage] < 0) { ++bad; return; }
        if (!consumed_a[stage][comp]) ++bad;                          // overwritten before its chain step read it
        a[stage][comp] = weights[ko[stage]];
        consumed_a[stage][comp] = 0;
        log.add(nkt, 1, clock, stage, comp, a[stage][comp]);
    };
    auto read_operand = [&](int clock, int stage, int tile) {
        if (!consumed_b[stage]) ++bad;
        b[stage] = operand[tile];
        consumed_b[stage] = 0;
        log.add(nkt, 2, clock, stage, 0, tile);
    };
    // prologue: k list 0 and 1, all gathers of tiles 0 and 1, operand 0, then k list 2 and 3
    read_klist(-2 * NC * SDFR_KC_RING_LEAD, sdfr_kc_ring_stage(0), 0);
    read_klist(-2 * NC * SDFR_KC_RING_LEAD, sdfr_kc_ring_stage(1), sdfr_kc_ring_clamp(1, nkt));
    for (int c = 0; c < NC; ++c) gather(c - NC * SDFR_KC_RING_LEAD, sdfr_kc_ring_stage(0), c);
    read_operand(-NC, sdfr_kc_ring_stage(0), 0);
    for (int c = 0; c < NC; ++c) gather(NC + c - NC * SDFR_KC_RING_LEAD, sdfr_kc_ring_stage(1), c);
    read_klist(-1, sdfr_kc_ring_stage(0), sdfr_kc_ring_clamp(2, nkt));
    read_klist(-1, sdfr_kc_ring_stage(1), sdfr_kc_ring_clamp(3, nkt));
    for (int t0 = 0; t0 < nkt; t0 += NS)
        for (int u = 0; u < NS; ++u) {
            const int t = t0 + u, s = sdfr_kc_ring_stage(t);
            read_operand(NC * t, sdfr_kc_ring_stage(t + 1), sdfr_kc_ring_operand_tile(t, nkt));
            for (int c = 0; c < NC; ++c) {
                if (a[s][c] != t || b[s] != t) ++bad;                 // the chain step reads its own tile, every tile in order
                log.add(nkt, 3, NC * t + c, s, c, a[s][c]);
                consumed_a[s][c] = 1;
                if (c == NC - 1) consumed_b[s] = 1;
                if (ko[s] != sdfr_kc_ring_gather_tile(t, nkt)) ++bad; // the k-list stage holds the words of the tile the rule names
                gather(NC * t + c, s, c);
            }
            read_klist(NC * t + NC - 1, s, sdfr_kc_ring_klist_tile(t, nkt));
        }
    return bad;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: kc_ring_host out.bin\n"); return 2; }
    Log log;
    int bad = 0, cases = 0;
    for (int nkt = 2; nkt <= 64; nkt += 2) { bad += run(nkt, log); ++cases; }
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    const size_t n = std::fwrite(log.rec.data(), sizeof(int32_t), log.rec.size(), f);
    std::fclose(f);
    if (n != log.rec.size()) return 4;
    std::printf("cases %d bad %d\n", cases, bad);
    return bad ? 1 : 0;
}
