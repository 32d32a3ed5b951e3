// Host emulation of the band Jacobian's compaction stage with chain-order survivor words (csrc/kcjd_slots.h; mlp_kernel.h, KCJ: kcj_vote and
// the stage of store_in_grad).  For every case -- four waves' survivor words w[wave][g] -- it builds the chain words as the vote does (each
// lane group's part, ORed), takes every lane's 32 places with the header's masked population count, as the kernel does, and enters the
// feature at its place; the places must be those of kcj_slots.h (sdfr_kcj_rank), a bijection onto [0, tot).  Every array has exactly the
// kernel's size, so the sanitizer builds see a place out of range.
//   kcjd_host OUT   writes per case 16 words, 16 chain words, tot, padded and the 512 features by chain position (int32, -1 beyond tot) to OUT;
//                   prints "cases N bad B"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kcjd_slots.h"

static const int HP = 512, NW = 4;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

struct Case { uint32_t w[NW][4]; };

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad < 10) fprintf(stderr, "case %d: check failed at line %d: %s\n", case_no, __LINE__, #c); ++bad; delete[] feat; return; } } while (0)

static void run_case(int case_no, const Case& cs, FILE* out) {
    int* feat = new int[HP];                                        // the compacted chain: feature at each place
    for (int i = 0; i < HP; ++i) feat[i] = -1;
    int cnt[NW], tot = 0;
    uint32_t chain[NW][4];
    for (int wv = 0; wv < NW; ++wv) {
        const uint32_t* w = cs.w[wv];
        cnt[wv] = sdfr_kcj_count(w[0], w[1], w[2], w[3]);
        tot += cnt[wv];
        for (int j = 0; j < 4; ++j) {                               // the vote: every lane group's part of chain word j, ORed
            uint32_t c = 0;
            for (int g = 0; g < 4; ++g) {
                const uint32_t part = sdfr_kcjd_group_part(w[g], j, g);
                CHECK((part & c) == 0u && (part & ~(0x11111111u << g)) == 0u);
                c |= part;
            }
            CHECK(c == sdfr_kcjd_chain_word(w[0], w[1], w[2], w[3], j));
            chain[wv][j] = c;
        }
        CHECK(sdfr_kcj_popc(chain[wv][0]) + sdfr_kcj_popc(chain[wv][1]) + sdfr_kcj_popc(chain[wv][2]) + sdfr_kcj_popc(chain[wv][3]) == cnt[wv]);
        for (int q = 0; q < 32; ++q)
            for (int g = 0; g < 4; ++g) CHECK(((chain[wv][q >> 3] >> (4 * (q & 7) + g)) & 1u) == ((w[g] >> q) & 1u));
    }
    const int padded = sdfr_kcj_padded(tot);
    for (int wv = 0; wv < NW; ++wv) {
        const uint32_t* w = cs.w[wv];
        int off = 0;
        for (int v = 0; v < wv; ++v) off += cnt[v];
        int cfront[4];
        cfront[0] = off;
        for (int j = 1; j < 4; ++j) cfront[j] = cfront[j - 1] + sdfr_kcj_popc(chain[wv][j - 1]);
        for (int lane = 0; lane < 64; ++lane) {
            const int lg = lane / 16;
            for (int q = 0; q < 32; ++q) {
                if (!((w[lg] >> q) & 1u)) continue;
                const int pos = sdfr_kcjd_rank_in_word(chain[wv][q >> 3], cfront[q >> 3], q, lg);
                CHECK(pos == off + sdfr_kcj_rank(w[0], w[1], w[2], w[3], q, lg));
                CHECK(pos == off + sdfr_kcjd_rank(chain[wv], q, lg));
                CHECK(pos >= 0 && pos < tot);
                const int k = wv * 128 + sdfr_kcj_feature(q, lg);
                CHECK(feat[pos] == -1 || feat[pos] == k);           // (the 16 lanes of a lane group agree; nobody else takes the place)
                feat[pos] = k;
                // the operand element and the k-list int of the place lie inside the kernel's arrays
                CHECK(sdfr_kcj_elem(pos, lane % 16) >= 0 && sdfr_kcj_elem(pos, lane % 16) < HP * SDFR_KCJ_PT && sdfr_kcj_kidx(pos) >= 0 && sdfr_kcj_kidx(pos) < HP);
            }
        }
    }
    for (int pos = 0; pos < HP; ++pos) CHECK((feat[pos] >= 0) == (pos < tot));
    {   // the place of the registers that did not survive: no survivor's, inside the operand, a padding slot or behind the product's K extent
        const int dead = sdfr_kcjd_dead_pos(tot);
        CHECK(tot == HP || (dead >= tot && dead < HP && feat[dead] == -1));
        CHECK(tot == HP || dead < padded || padded == tot);
        for (int pt = 0; pt < SDFR_KCJ_PT; ++pt) CHECK(sdfr_kcj_elem(dead, pt) >= 0 && sdfr_kcj_elem(dead, pt) < HP * SDFR_KCJ_PT);
    }
    int32_t rec[16 + 16 + 2];
    for (int wv = 0; wv < NW; ++wv)
        for (int g = 0; g < 4; ++g) { rec[wv * 4 + g] = (int32_t)cs.w[wv][g]; rec[16 + wv * 4 + g] = (int32_t)chain[wv][g]; }
    rec[32] = tot; rec[33] = padded;
    fwrite(rec, sizeof(int32_t), 34, out);
    fwrite(feat, sizeof(int), HP, out);
    delete[] feat;
}

static Case with_count(int n) {                                     // n survivors at random places
    Case c;
    memset(&c, 0, sizeof c);
    int left = n;
    while (left > 0) {
        const int wv = rnd() % NW, g = rnd() % 4, q = rnd() % 32;
        if ((c.w[wv][g] >> q) & 1u) continue;
        c.w[wv][g] |= 1u << q;
        --left;
    }
    return c;
}
static Case with_density(int permille) {
    Case c;
    memset(&c, 0, sizeof c);
    for (int wv = 0; wv < NW; ++wv)
        for (int g = 0; g < 4; ++g)
            for (int q = 0; q < 32; ++q)
                if ((int)(rnd() % 1000) < permille) c.w[wv][g] |= 1u << q;
    return c;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: kcjd_host OUT\n"); return 2; }
    FILE* out = fopen(argv[1], "wb");
    if (!out) return 2;
    std::vector<Case> cases;
    const int counts[] = {0, 1, 63, 64, 65, 128, 512};
    for (int n : counts)
        for (int r = 0; r < (n == 0 || n == 512 ? 1 : 20); ++r) cases.push_back(with_count(n));
    for (int wv = 0; wv < NW; ++wv)                                  // an empty wave block
        for (int r = 0; r < 10; ++r) {
            Case c = with_density(500);
            memset(c.w[wv], 0, sizeof c.w[wv]);
            cases.push_back(c);
        }
    for (int r = 0; r < 12; ++r) {                                   // survivors only in the last lane group of the last wave
        Case c;
        memset(&c, 0, sizeof c);
        c.w[3][3] = r == 0 ? 0xFFFFFFFFu : (r == 1 ? 0x80000000u : (r == 2 ? 1u : rnd()));
        cases.push_back(c);
    }
    const int dens[] = {100, 500, 900};
    for (int d : dens)
        for (int r = 0; r < 200; ++r) cases.push_back(with_density(d));
    for (size_t i = 0; i < cases.size(); ++i) run_case((int)i, cases[i], out);
    fclose(out);
    printf("cases %d bad %d\n", (int)cases.size(), bad);
    return bad ? 1 : 0;
}
