// Host emulation of one workgroup's KC epilogue and product reads with the DENSE image of the 64-row kernels (csrc/kc_slots.h, the
// sdfr_kcd_* functions; mlp_kernel.h, kc_store and gemm_kc_body): 8 waves x 64 lanes, lane by lane, with the header's own arithmetic.
// Reads mask sets (8 x uint64 chain masks per case, bit c = 2 q + g of wave w), gives every live accumulator register a tag of its own
// (dead ones hold the zero a ReLU leaves), and writes per case
//     int32 ok, tot, padded, pad_wave, klist[512], visit[512]   (+ float image[513 * 64] with "dump")
// visit[pos] = the operand row the emulated product reads at chain position pos (k tile pos / 8, step (pos % 8) / 2, lane group pos % 2),
// -1 for pos >= padded.  ok = 0 when a dword of rows [0, 512) was not written exactly once by the epilogue, when the zero row was written
// by anything but its one-time initialisation, when a store or read is not 8-byte aligned, when the image is not the one the rule defines
// (feature j -> row j, point p 32 + lp at dword 2 lp + p, zeros for dead features), when a lane of the product reads anything but the tags
// of the feature its k word names (zeros for a pad), or when the weight row a k word gives is not that feature's (512 for a pad).  The
// rule is restated here without the header.  pad_wave = the wave that wrote the pad entries (-1: none).
// With "addrs" a case is followed by int32 store[8 waves][32 registers][64 lanes] and int32 read[64 k tiles][4 steps][64 lanes]: byte
// addresses of the 8-byte epilogue stores and product reads (-1: k tile beyond the layer's), for the bank check of
// tests/test_kc_dense_cpu.py.
//   kc_dense_host masks.bin out.bin [dump | addrs]
#include "kc_slots.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
constexpr int NW = 8, HP = 512, PT = 64, ROWS = HP + 1;

float tag(int feature, int point) { return (float)(feature * 64 + point + 1); }

struct Tile {
    std::vector<float> image = std::vector<float>(ROWS * PT);     // exact size: an access outside image + zero row is an error under the sanitizers
    std::vector<int> writes = std::vector<int>(ROWS * PT);
    int klist[HP], kwrites[HP], visit[HP];
    std::vector<int32_t> store_addr = std::vector<int32_t>(NW * 32 * 64);
    std::vector<int32_t> read_addr = std::vector<int32_t>(HP / 8 * 4 * 64);
};

float image_at(const Tile& T, uint32_t byte) { return T.image.at(byte / 4); }

bool run_case(const uint64_t* cm, Tile& T, int& tot, int& padded, int& pad_wave) {
    for (auto& v : T.image) v = -1.f;
    for (auto& v : T.writes) v = 0;
    for (auto& v : T.read_addr) v = -1;
    for (int s = 0; s < HP; ++s) { T.klist[s] = -1; T.kwrites[s] = 0; T.visit[s] = -1; }
    bool ok = true;
    // once per workgroup: threads 0..15 zero the row behind the image with one 16-byte store each
    for (int tid = 0; tid < SDFR_KCD_ROW_BYTES / 16; ++tid)
        for (int e = 0; e < 4; ++e) T.image.at(SDFR_KCD_ZERO_ROW * PT + tid * 4 + e) = 0.f;
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
    static float acc[2][2][16][64];                                       // [f][p][r][lane], the kernel's accumulators of one wave
    for (int wv = NW - 1; wv >= 0; --wv) {                                // (any order: the waves' stores do not meet)
        int off = 0;
        for (int u = 0; u < wv; ++u) off += cnt[u];
        // lane (g, lp) holds the feature of (register q, g) at points p 32 + lp: its tag where it lives, the ReLU's zero where it is dead
        for (int f = 0; f < 2; ++f)
            for (int p = 0; p < 2; ++p)
                for (int r = 0; r < 16; ++r)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int q = f * 16 + r, g = lane / 32;
                        const bool alive = (w[wv][g] >> q) & 1u;
                        acc[f][p][r][lane] = alive ? tag(sdfr_kcd_feature(wv, q, g), p * 32 + lane % 32) : 0.f;
                    }
        for (int lane = 0; lane < 64; ++lane) {
            const int lp = lane % 32, lg = lane / 32;
            // 32 unconditional 8-byte stores: the lane's address register plus the register's constant
            const int dl = sdfr_kcm_lane_dword(sdfr_kcd_row(wv * 64 + sdfr_kcd_row_lane(0, lg)), lp);
            for (int q = 0; q < 32; ++q) {
                const int d = dl + sdfr_kcm_lane_dword(sdfr_kcd_row_reg(q), 0);
                T.store_addr[(wv * 32 + q) * 64 + lane] = d * 4;
                ok = ok && d % 2 == 0;
                for (int p = 0; p < 2; ++p) {
                    T.image.at(d + p) = acc[q / 16][p][q % 16][lane];
                    ++T.writes.at(d + p);
                }
            }
            // k list: lane (g, q) enters the row of register q's feature, lane group g
            const int q = lane % 32, g = lane / 32;
            if ((w[wv][g] >> q) & 1u) {
                const int s = sdfr_kc_slot(off + sdfr_kc_rank(w[wv][0], w[wv][1], q, g));
                T.klist[s] = sdfr_kcd_entry(wv * 64 + sdfr_kcd_feature(0, q, g));
                ++T.kwrites[s];
            }
        }
        if (sdfr_kcm_pads(wv)) {
            for (int lane = 0; lane < 64; ++lane)
                if (lane < padded - tot) {
                    const int s = sdfr_kc_slot(tot + lane);
                    T.klist[s] = sdfr_kcd_pad_entry();
                    ++T.kwrites[s];
                    pad_wave = wv;
                }
        }
    }
    // the product: k tile t, step ks; lane (lp, lg) takes component ks of the k-list vector [t][lg] and reads its 8 bytes of that row
    const int* kl = T.klist;
    for (int t = 0; t < padded / 8; ++t)
        for (int ks = 0; ks < 4; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int lp = lane % 32, lg = lane / 32;
                const int entry = kl[(t * 2 + lg) * 4 + ks];
                const uint32_t a = sdfr_kcd_operand_byte(entry, lp);
                T.read_addr[(t * 4 + ks) * 64 + lane] = (int32_t)a;
                ok = ok && a % 8 == 0;
                const int row = entry / 256;                                  // (restated: 256 bytes per row)
                const int pos = 8 * t + 2 * ks + lg;
                if (lp == 0) T.visit[pos] = row;
                ok = ok && T.visit[pos] == row;
                const int krow = (int)(sdfr_kcd_weight_byte(entry) / (512 * 4));   // (restated: 512 floats per k row of Wk)
                ok = ok && krow == row && sdfr_kcd_weight_byte(entry) % (512 * 4) == 0;
                for (int p = 0; p < 2; ++p) {
                    const float v = image_at(T, a + 4 * p);
                    ok = ok && v == (row == 512 ? 0.f : tag(row, p * 32 + lp));
                }
            }
    // the rule, restated: walk the full chain, count the survivors
    std::vector<float> want(ROWS * PT, 0.f);
    std::vector<int> wantk(HP, -1), wantv(HP, -1);
    int pos = 0;
    for (int wv = 0; wv < NW; ++wv)
        for (int c = 0; c < 64; ++c)
            if ((cm[wv] >> c) & 1ull) {
                const int q = c >> 1, g = c & 1;
                const int j = wv * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3);
                for (int pt = 0; pt < PT; ++pt) want[j * 64 + 2 * (pt % 32) + pt / 32] = tag(j, pt);
                wantk[(pos & ~7) | ((pos & 1) * 4) | ((pos & 7) >> 1)] = j * 256;
                wantv[pos] = j;
                ++pos;
            }
    ok = ok && pos == tot;
    const int pad_to = (pos + 15) / 16 * 16;
    ok = ok && pad_to == padded;
    ok = ok && pad_wave == (pad_to > pos ? 0 : -1);
    for (; pos < pad_to; ++pos) {
        wantk[(pos & ~7) | ((pos & 1) * 4) | ((pos & 7) >> 1)] = 512 * 256;
        wantv[pos] = 512;
    }
    for (int s = 0; s < HP; ++s) {
        ok = ok && T.kwrites[s] == (s < padded ? 1 : 0) && T.klist[s] == wantk[s] && T.visit[s] == wantv[s];
        for (int d = s * 64; d < s * 64 + 64; ++d) ok = ok && T.writes[d] == 1 && T.image[d] == want[d];
    }
    for (int d = HP * 64; d < ROWS * 64; ++d) ok = ok && T.writes[d] == 0 && T.image[d] == 0.f;
    return ok;
}

// the operand's place in the ring: two stages, refilled component by component behind the chain step that has just read the component
// (with the weights, sdfr_kcd_ring_operand_tile); every chain step must find its own tile's component in its stage
bool ring_ok(int nkt) {
    int stage[SDFR_KC_RING_STAGES][4];
    for (int ks = 0; ks < 4; ++ks) { stage[0][ks] = 0; stage[1][ks] = sdfr_kc_ring_clamp(1, nkt); }   // prologue
    for (int t = 0; t < nkt; ++t)
        for (int ks = 0; ks < 4; ++ks) {
            if (stage[sdfr_kc_ring_stage(t)][ks] != t) return false;
            stage[sdfr_kc_ring_stage(t)][ks] = sdfr_kcd_ring_operand_tile(t, nkt);
            if (stage[sdfr_kc_ring_stage(t)][ks] >= nkt) return false;                               // never a tile beyond the list
        }
    return true;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s masks.bin out.bin [dump | addrs]\n", argv[0]); return 2; }
    for (int nkt = 2; nkt <= HP / 8; nkt += 2)
        if (!ring_ok(nkt)) { fprintf(stderr, "ring rule fails at %d k tiles\n", nkt); return 3; }
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
        fwrite(T.visit, sizeof(int32_t), HP, fo);
        if (dump) fwrite(T.image.data(), sizeof(float), T.image.size(), fo);
        if (addrs) {
            fwrite(T.store_addr.data(), sizeof(int32_t), T.store_addr.size(), fo);
            fwrite(T.read_addr.data(), sizeof(int32_t), T.read_addr.size(), fo);
        }
        ++n;
        bad += ok ? 0 : 1;
    }
    fclose(fi);
    fclose(fo);
    printf("cases %d bad %d\n", n, bad);
    return bad ? 1 : 0;
}
