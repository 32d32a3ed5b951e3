// Host emulation of one workgroup's KC epilogue (csrc/kc_slots.h; mlp_kernel.h, kc_store fed from the two survivor words): 8 waves x 64
// lanes, lane by lane, with the header's own rank and slot arithmetic.  Reads mask sets (8 x uint64 chain masks per case, bit c = 2 q + g of wave w), gives every
// accumulator register a tag of its own, and writes per case
//     int32 ok, tot, padded, klist[512]  (+ float image[512 * 64] with "dump")
// ok = 0 when a dword of the live region [0, padded) x 64 points was not written exactly once, when one outside was written, or when the
// image is not the one the rule defines (survivor at chain position pos -> slot (pos & ~7) | (pos & 1) * 4 | (pos & 7) >> 1 of its point,
// zeros up to the next multiple of 16), which is restated here without the header.
//   kc_epilogue_host masks.bin out.bin [dump]
#include "kc_slots.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
constexpr int NW = 8, HP = 512, PT = 64;

float tag(int wave, int c, int point) { return (float)((wave * 64 + c) * 64 + point + 1); }

struct Tile {
    std::vector<float> image = std::vector<float>(HP * PT);
    std::vector<int> writes = std::vector<int>(HP * PT);
    int klist[HP], kwrites[HP];
};

// dword of slot s (a point's compacted row) in the operand image act[vector][point][component]
int dword_of(int s, int point) { return ((s / 4) * PT + point) * 4 + (s % 4); }

bool run_case(const uint64_t* cm, Tile& T, int& tot, int& padded) {
    for (auto& v : T.image) v = -1.f;
    for (auto& v : T.writes) v = 0;
    for (int s = 0; s < HP; ++s) { T.klist[s] = -1; T.kwrites[s] = 0; }
    uint32_t w[NW][2];
    int cnt[NW];
    tot = 0;
    for (int wv = 0; wv < NW; ++wv) {
        w[wv][0] = w[wv][1] = 0u;
        for (int q = 0; q < 32; ++q)
            for (int g = 0; g < 2; ++g) w[wv][g] |= (uint32_t)((cm[wv] >> (2 * q + g)) & 1ull) << q;
        cnt[wv] = sdfr_kc_popc(w[wv][0]) + sdfr_kc_popc(w[wv][1]);         // kc_cnt[wave]
        tot += cnt[wv];
    }
    padded = sdfr_kc_padded(tot);
    static float acc[2][2][16][64];                                       // [f][p][r][lane], the kernel's accumulators of one wave
    for (int wv = NW - 1; wv >= 0; --wv) {                                // (any order: the waves' stores do not meet)
        int off = 0;
        for (int u = 0; u < wv; ++u) off += cnt[u];
        // lane (g, lp) holds feature (q, g) at points p 32 + lp
        for (int f = 0; f < 2; ++f)
            for (int p = 0; p < 2; ++p)
                for (int r = 0; r < 16; ++r)
                    for (int lane = 0; lane < 64; ++lane) acc[f][p][r][lane] = tag(wv, 2 * (f * 16 + r) + lane / 32, p * 32 + lane % 32);
        for (int lane = 0; lane < 64; ++lane) {
            const int lp = lane % 32, lg = lane / 32;
            for (int q = 0; q < 32; ++q) {
                const int below = sdfr_kc_rank(w[wv][0], w[wv][1], q, 0);                // as kc_store: wave-uniform part, then the lane group's
                const bool b0 = (w[wv][0] >> q) & 1u, b1 = (w[wv][1] >> q) & 1u;
                if (lg ? b1 : b0) {
                    const int s = sdfr_kc_slot(off + below + ((lg && b0) ? 1 : 0));
                    for (int p = 0; p < 2; ++p) {
                        const int d = dword_of(s, p * 32 + lp);
                        T.image[d] = acc[q / 16][p][q % 16][lane];
                        ++T.writes[d];
                    }
                }
            }
            // k list: lane (g, q) enters the feature of register q, lane group g
            const int q = lane % 32, g = lane / 32;
            if ((w[wv][g] >> q) & 1u) {
                const int j = wv * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3);
                const int s = sdfr_kc_slot(off + sdfr_kc_rank(w[wv][0], w[wv][1], q, g));
                T.klist[s] = j * HP;
                ++T.kwrites[s];
            }
        }
        if (sdfr_kc_pads(wv, NW))
            for (int e = 0; e < padded - tot; ++e) {
                const int s = sdfr_kc_slot(tot + e);
                for (int lane = 0; lane < PT; ++lane) { T.image[dword_of(s, lane)] = 0.f; ++T.writes[dword_of(s, lane)]; }
                T.klist[s] = 0;
                ++T.kwrites[s];
            }
    }
    // the rule, restated: walk the full chain, count the survivors
    bool ok = true;
    std::vector<float> want(HP * PT, -1.f);
    std::vector<int> wantk(HP, -1);
    int pos = 0;
    for (int wv = 0; wv < NW; ++wv)
        for (int c = 0; c < 64; ++c)
            if ((cm[wv] >> c) & 1ull) {
                const int s = (pos & ~7) | ((pos & 1) * 4) | ((pos & 7) >> 1);
                for (int pt = 0; pt < PT; ++pt) want[((s >> 2) * PT + pt) * 4 + (s & 3)] = tag(wv, c, pt);
                const int q = c >> 1, g = c & 1;
                wantk[s] = (wv * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3)) * HP;
                ++pos;
            }
    ok = ok && pos == tot;
    const int pad_to = (pos + 15) / 16 * 16;
    ok = ok && pad_to == padded;
    for (; pos < pad_to; ++pos) {
        const int s = (pos & ~7) | ((pos & 1) * 4) | ((pos & 7) >> 1);
        for (int pt = 0; pt < PT; ++pt) want[((s >> 2) * PT + pt) * 4 + (s & 3)] = 0.f;
        wantk[s] = 0;
    }
    for (int s = 0; s < HP; ++s) {
        const int once = s < padded ? 1 : 0;
        ok = ok && T.kwrites[s] == once && T.klist[s] == wantk[s];
        for (int pt = 0; pt < PT; ++pt) {
            const int d = dword_of(s, pt);
            ok = ok && T.writes[d] == once && T.image[d] == want[d];
        }
    }
    return ok;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s masks.bin out.bin [dump]\n", argv[0]); return 2; }
    const bool dump = argc > 3 && !strcmp(argv[3], "dump");
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    Tile T;
    uint64_t cm[NW];
    int n = 0, bad = 0;
    while (fread(cm, sizeof(uint64_t), NW, fi) == (size_t)NW) {
        int tot = 0, padded = 0;
        const bool ok = run_case(cm, T, tot, padded);
        const int32_t head[3] = {ok ? 1 : 0, tot, padded};
        fwrite(head, sizeof(int32_t), 3, fo);
        fwrite(T.klist, sizeof(int32_t), HP, fo);
        if (dump) fwrite(T.image.data(), sizeof(float), T.image.size(), fo);
        ++n;
        bad += ok ? 0 : 1;
    }
    fclose(fi);
    fclose(fo);
    printf("cases %d bad %d\n", n, bad);
    return bad ? 1 : 0;
}
