// Host emulation of one workgroup's KC epilogue with the k-major image of the compacted operand (csrc/kc_slots.h, the sdfr_kcm_* functions;
// mlp_kernel.h, kc_store of the 64-row kernels): 8 waves x 64 lanes, lane by lane, with the header's own arithmetic.  Reads mask sets
// (8 x uint64 chain masks per case, bit c = 2 q + g of wave w), gives every accumulator register a tag of its own, and writes per case
//     int32 ok, tot, padded, pad_wave, klist[512]  (+ float image[512 * 64] with "dump")
// ok = 0 when a dword of rows [0, padded) was not written exactly once, when one outside was written, when an 8-byte survivor store or a
// 16-byte padding store is not aligned to its size, or when the image is not the one the rule defines (survivor at chain position pos ->
// row pos, point p 32 + lp at dword 2 lp + p; zero rows up to the next multiple of 16), which is restated here without the header.
// pad_wave = the wave that wrote the padding (-1: nothing to pad).  The k list is the one of the old image (slot rule restated here).
// With "addrs" instead of "dump" a case is followed by int32 store[8 waves][32 registers][64 lanes]: the byte address of the lane's 8-byte
// survivor store of register q (-1: the lane stores nothing), for the bank check of tests/test_kc_kmajor_cpu.py.
//   kc_kmajor_host masks.bin out.bin [dump | addrs]
//   kc_kmajor_host reads out.bin      int32 [64 k tiles][4 steps][64 lanes]: byte address of the product's 8-byte B read (sdfr_kcm_read_row)
#include "kc_slots.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
constexpr int NW = 8, HP = 512, PT = 64;

float tag(int wave, int c, int point) { return (float)((wave * 64 + c) * 64 + point + 1); }

struct Tile {
    std::vector<float> image = std::vector<float>(HP * PT);      // exact size: a store outside the operand is an error under the sanitizers
    std::vector<int> writes = std::vector<int>(HP * PT);
    int klist[HP], kwrites[HP];
    std::vector<int32_t> store_addr = std::vector<int32_t>(NW * 32 * 64);
};

bool run_case(const uint64_t* cm, Tile& T, int& tot, int& padded, int& pad_wave) {
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
    pad_wave = -1;
    bool ok = true;
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
            int n = off;                                                  // as kc_store: a running wave-uniform count over q
            for (int q = 0; q < 32; ++q) {
                const int b0 = (int)((w[wv][0] >> q) & 1u), b1 = (int)((w[wv][1] >> q) & 1u);
                T.store_addr[(wv * 32 + q) * 64 + lane] = -1;
                if (lg ? b1 : b0) {
                    const int d = sdfr_kcm_lane_dword(n + (lg ? b0 : 0), lp);          // one 8-byte store: both points of the lane
                    T.store_addr[(wv * 32 + q) * 64 + lane] = d * 4;
                    ok = ok && d % 2 == 0;
                    for (int p = 0; p < 2; ++p) {
                        T.image.at(d + p) = acc[q / 16][p][q % 16][lane];
                        ++T.writes.at(d + p);
                    }
                }
                n += b0 + b1;
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
        if (sdfr_kcm_pads(wv)) {
            for (int lane = 0; lane < 64; ++lane) {
                for (int i = 0; i < SDFR_KCM_PAD_STORES; ++i) {
                    const int v = sdfr_kcm_pad_vec(tot, i, lane);         // one 16-byte store
                    if (v < padded * 16) {
                        pad_wave = wv;
                        for (int e = 0; e < 4; ++e) { T.image.at(v * 4 + e) = 0.f; ++T.writes.at(v * 4 + e); }
                    }
                }
                if (lane < padded - tot) {
                    const int s = sdfr_kc_slot(tot + lane);
                    T.klist[s] = 0;
                    ++T.kwrites[s];
                }
            }
        }
    }
    // the rule, restated: walk the full chain, count the survivors
    std::vector<float> want(HP * PT, -1.f);
    std::vector<int> wantk(HP, -1);
    int pos = 0;
    for (int wv = 0; wv < NW; ++wv)
        for (int c = 0; c < 64; ++c)
            if ((cm[wv] >> c) & 1ull) {
                for (int pt = 0; pt < PT; ++pt) want[pos * 64 + 2 * (pt % 32) + pt / 32] = tag(wv, c, pt);
                const int s = (pos & ~7) | ((pos & 1) * 4) | ((pos & 7) >> 1);
                const int q = c >> 1, g = c & 1;
                wantk[s] = (wv * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3)) * HP;
                ++pos;
            }
    ok = ok && pos == tot;
    const int pad_to = (pos + 15) / 16 * 16;
    ok = ok && pad_to == padded;
    ok = ok && pad_wave == (pad_to > pos ? 0 : -1);
    for (; pos < pad_to; ++pos) {
        for (int d = 0; d < 64; ++d) want[pos * 64 + d] = 0.f;
        wantk[(pos & ~7) | ((pos & 1) * 4) | ((pos & 7) >> 1)] = 0;
    }
    for (int s = 0; s < HP; ++s) {
        const int once = s < padded ? 1 : 0;
        ok = ok && T.kwrites[s] == once && T.klist[s] == wantk[s];
        for (int d = s * 64; d < s * 64 + 64; ++d) ok = ok && T.writes[d] == once && T.image[d] == want[d];
    }
    return ok;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s masks.bin out.bin [dump | addrs]  |  %s reads out.bin\n", argv[0], argv[0]); return 2; }
    if (!strcmp(argv[1], "reads")) {
        FILE* fr = fopen(argv[2], "wb");
        if (!fr) { fprintf(stderr, "cannot open files\n"); return 2; }
        for (int t = 0; t < HP / 8; ++t)
            for (int ks = 0; ks < 4; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int32_t a = sdfr_kcm_lane_dword(sdfr_kcm_read_row(t, ks, lane / 32), lane % 32) * 4;
                    fwrite(&a, sizeof(int32_t), 1, fr);
                }
        fclose(fr);
        return 0;
    }
    const bool dump = argc > 3 && !strcmp(argv[3], "dump");
    const bool addrs = argc > 3 && !strcmp(argv[3], "addrs");
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    Tile T;
    uint64_t cm[NW];
    int n = 0, bad = 0;
    while (fread(cm, sizeof(uint64_t), NW, fi) == (size_t)NW) {
        int tot = 0, padded = 0, pad_wave = -1;
        const bool ok = run_case(cm, T, tot, padded, pad_wave);
        const int32_t head[4] = {ok ? 1 : 0, tot, padded, pad_wave};
        fwrite(head, sizeof(int32_t), 4, fo);
        fwrite(T.klist, sizeof(int32_t), HP, fo);
        if (dump) fwrite(T.image.data(), sizeof(float), T.image.size(), fo);
        if (addrs) fwrite(T.store_addr.data(), sizeof(int32_t), T.store_addr.size(), fo);
        ++n;
        bad += ok ? 0 : 1;
    }
    fclose(fi);
    fclose(fo);
    printf("cases %d bad %d\n", n, bad);
    return bad ? 1 : 0;
}
