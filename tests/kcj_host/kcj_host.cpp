// Host emulation of the band Jacobian's K compaction (csrc/kcj_slots.h; mlp_kernel.h, KCJ: store_in_grad's compacted operand and gemm_kcj).
// For every case -- four waves' survivor words w[wave][g] -- it writes the compacted operand, the k list and the padding with the header's
// own arithmetic, lane by lane as the kernel does, walks the product loop's ring, and compares the compacted product with the full chain
// bit for bit (float fmaf in chain order).  Every array has exactly the kernel's size, so the sanitizer builds see a slot out of range.
//   kcj_host OUT   writes per case 16 words, tot, padded and the 512 k-list entries (int32) to OUT; prints "cases N bad B"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kcj_slots.h"

static const int HP = 512, PT = SDFR_KCJ_PT, NW = 4, COLS = 2;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static float rndf() { return (float)((int)(rnd() % 2001) - 1000) / 512.0f; }

struct Case { uint32_t w[NW][4]; };

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad < 10) fprintf(stderr, "case %d: check failed at line %d: %s\n", case_no, __LINE__, #c); ++bad; return; } } while (0)

static std::vector<float> Wt;           // [k][col] weights of COLS in-features

static void run_case(int case_no, const Case& cs, FILE* out) {
    // the full operand: g (.) mask, exactly +0 where the row's mask bit is 0; a survivor is alive in at least one row
    std::vector<float> full((size_t)HP * PT, 0.0f);
    for (int wv = 0; wv < NW; ++wv)
        for (int g = 0; g < 4; ++g)
            for (int q = 0; q < 32; ++q)
                if ((cs.w[wv][g] >> q) & 1u) {
                    const int k = wv * 128 + sdfr_kcj_feature(q, g);
                    const int alive = (int)(rnd() % PT);
                    for (int pt = 0; pt < PT; ++pt)
                        if (pt == alive || (rnd() & 1u)) full[(size_t)k * PT + pt] = rndf();
                }
    int cnt[NW], tot = 0;
    for (int wv = 0; wv < NW; ++wv) { cnt[wv] = sdfr_kcj_count(cs.w[wv][0], cs.w[wv][1], cs.w[wv][2], cs.w[wv][3]); tot += cnt[wv]; }
    const int padded = sdfr_kcj_padded(tot);
    CHECK(padded % (SDFR_KCJ_KT * SDFR_KCJ_RING) == 0 && padded >= SDFR_KCJ_KT * SDFR_KCJ_RING && padded >= tot && padded <= HP);
    // what the kernel's LDS holds: garbage first, so that a slot nobody writes shows
    float* act = new float[(size_t)HP * PT];
    int* klist = new int[HP];
    unsigned char* seen = new unsigned char[HP];
    for (int i = 0; i < HP * PT; ++i) act[i] = NAN;
    for (int i = 0; i < HP; ++i) { klist[i] = -1; seen[i] = 0; }
    auto done = [&]() { delete[] act; delete[] klist; delete[] seen; };
    for (int wv = 0; wv < NW; ++wv) {
        const uint32_t* w = cs.w[wv];
        int off = 0;
        for (int v = 0; v < wv; ++v) off += cnt[v];
        for (int lane = 0; lane < 64; ++lane) {                     // the values: running count over the registers, as store_in_grad does
            const int lp = lane % 16, lg = lane / 16;
            int n = off;
            for (int q = 0; q < 32; ++q) {
                const int b0 = (w[0] >> q) & 1u, b1 = (w[1] >> q) & 1u, b2 = (w[2] >> q) & 1u, b3 = (w[3] >> q) & 1u;
                const int front = (((b0 << 2) | ((b0 + b1) << 4) | ((b0 + b1 + b2) << 6)) >> (2 * lg)) & 3;
                if ((w[lg] >> q) & 1u) {
                    const int pos = n + front;
                    if (!(pos == off + sdfr_kcj_rank(w[0], w[1], w[2], w[3], q, lg) && pos >= 0 && pos < tot)) { done(); CHECK(!"rank"); }
                    act[sdfr_kcj_elem(pos, lp)] = full[(size_t)(wv * 128 + sdfr_kcj_feature(q, lg)) * PT + lp];
                }
                n += b0 + b1 + b2 + b3;
            }
            for (int h = 0; h < 2; ++h) {                           // the k list: registers lp and lp + 16 of the lane's lane group
                const int q = lp + 16 * h;
                if ((w[lg] >> q) & 1u) {
                    const int pos = off + sdfr_kcj_rank(w[0], w[1], w[2], w[3], q, lg);
                    if (!(pos >= 0 && pos < tot && !seen[pos])) { done(); CHECK(!"ranks are a bijection"); }
                    seen[pos] = 1;
                    klist[sdfr_kcj_kidx(pos)] = (wv * 128 + sdfr_kcj_feature(q, lg)) * HP;
                }
            }
        }
    }
    for (int pos = 0; pos < tot; ++pos) if (!seen[pos]) { done(); CHECK(!"every chain position below tot is taken"); }
    for (int tid = 0; tid < 64 * NW; ++tid)                         // the padding
        for (int e = tid; e < (padded - tot) * PT; e += 64 * NW) {
            const int pos = sdfr_kcj_pad_pos(tot, e);
            if (!(pos >= tot && pos < padded)) { done(); CHECK(!"pad position"); }
            act[sdfr_kcj_elem(pos, sdfr_kcj_pad_point(e))] = 0.0f;
            if (sdfr_kcj_pad_point(e) == 0) klist[sdfr_kcj_kidx(pos)] = 0;
        }
    // chain order: the survivors appear in the compacted chain in the order the full chain visits them; pads are zero with k entry 0
    {
        int pos = 0;
        for (int t = 0; t < HP / 16; ++t)
            for (int s = 0; s < 4; ++s)
                for (int g = 0; g < 4; ++g) {
                    const int k = 16 * t + 4 * g + s, wv = k / 128, q = ((k % 128) / 16) * 4 + s;
                    if (!((cs.w[wv][g] >> q) & 1u)) continue;
                    if (klist[sdfr_kcj_kidx(pos)] != k * HP) { done(); CHECK(!"chain order"); }
                    ++pos;
                }
        if (pos != tot) { done(); CHECK(!"survivor count"); }
        for (pos = 0; pos < padded; ++pos) {
            const int e = klist[sdfr_kcj_kidx(pos)];
            if (!(e >= 0 && e % HP == 0 && e / HP < HP)) { done(); CHECK(!"k-list entry"); }
            for (int pt = 0; pt < PT; ++pt) {
                const float v = act[sdfr_kcj_elem(pos, pt)];
                if (pos >= tot && !(v == 0.0f && !std::signbit(v) && e == 0)) { done(); CHECK(!"pad slot"); }
                if (v != v) { done(); CHECK(!"slot never written"); }
            }
        }
    }
    // the product loop's ring (gemm_kcj): stages hold tile numbers; every index lies in [0, nkt)
    const int nkt = padded / SDFR_KCJ_KT, R = SDFR_KCJ_RING;
    std::vector<float> accc((size_t)COLS * PT, 0.0f), accf((size_t)COLS * PT, 0.0f);
    {
        int a_tile[SDFR_KCJ_RING], b_tile[2], ko;
        auto in_range = [&](int t) { return t >= 0 && t < nkt; };
        ko = 0;
        for (int u = 0; u < R - 1; ++u) {
            a_tile[u] = ko;
            ko = sdfr_kcj_ring_clamp(u + 1, nkt);
            if (!in_range(ko)) { done(); CHECK(!"ring prologue index"); }
        }
        b_tile[0] = 0;
        for (int t = 0; t < nkt; t += R)
            for (int u = 0; u < R; ++u) {
                a_tile[(u + R - 1) % R] = ko;
                if (ko != sdfr_kcj_ring_gather_tile(t + u, nkt)) { done(); CHECK(!"gather addressed by its own tile's words"); }
                b_tile[(u + 1) % 2] = sdfr_kcj_ring_operand_tile(t + u, nkt);
                ko = sdfr_kcj_ring_klist_tile(t + u, nkt);
                if (!(in_range(ko) && in_range(b_tile[(u + 1) % 2]) && in_range(a_tile[(u + R - 1) % R]))) { done(); CHECK(!"ring index"); }
                if (!(a_tile[u] == t + u && b_tile[u % 2] == t + u)) { done(); CHECK(!"chain step reads its own tile"); }
                const int tile = a_tile[u];
                for (int s = 0; s < 4; ++s)
                    for (int g = 0; g < 4; ++g) {
                        const int vec = tile * 4 + g, krow = klist[vec * 4 + s] / HP;
                        for (int c = 0; c < COLS; ++c)
                            for (int pt = 0; pt < PT; ++pt)
                                accc[c * PT + pt] = fmaf(Wt[(size_t)krow * COLS + c], act[(vec * PT + pt) * 4 + s], accc[c * PT + pt]);
                    }
            }
    }
    for (int t = 0; t < HP / 16; ++t)                               // the full chain: k = 16 t + 4 g + s in the order (t, s, g)
        for (int s = 0; s < 4; ++s)
            for (int g = 0; g < 4; ++g) {
                const int k = 16 * t + 4 * g + s;
                for (int c = 0; c < COLS; ++c)
                    for (int pt = 0; pt < PT; ++pt)
                        accf[c * PT + pt] = fmaf(Wt[(size_t)k * COLS + c], full[(size_t)k * PT + pt], accf[c * PT + pt]);
            }
    if (memcmp(accc.data(), accf.data(), accc.size() * sizeof(float)) != 0) { done(); CHECK(!"compacted product == full chain, bit for bit"); }
    if (out) {
        int32_t head[18];
        for (int wv = 0; wv < NW; ++wv) for (int g = 0; g < 4; ++g) head[wv * 4 + g] = (int32_t)cs.w[wv][g];
        head[16] = tot; head[17] = padded;
        fwrite(head, sizeof(int32_t), 18, out);
        fwrite(klist, sizeof(int32_t), HP, out);
    }
    done();
}

// c random survivors among a wave's 128 features
static void pick(uint32_t* w, int c) {
    int order[128];
    for (int i = 0; i < 128; ++i) order[i] = i;
    for (int i = 127; i > 0; --i) { const int j = (int)(rnd() % (uint32_t)(i + 1)), x = order[i]; order[i] = order[j]; order[j] = x; }
    w[0] = w[1] = w[2] = w[3] = 0u;
    for (int i = 0; i < c; ++i) w[order[i] / 32] |= 1u << (order[i] % 32);
}

int main(int argc, char** argv) {
    FILE* out = argc > 1 ? fopen(argv[1], "wb") : nullptr;
    Wt.resize((size_t)HP * COLS);
    for (auto& w : Wt) w = rndf();
    int n = 0;
    Case cs;
    for (int wv = 0; wv < NW; ++wv)                                 // every per-wave count in each wave's position, the others random
        for (int c = 0; c <= 128; ++c) {
            for (int v = 0; v < NW; ++v) pick(cs.w[v], (int)(rnd() % 129));
            pick(cs.w[wv], c);
            run_case(n++, cs, out);
        }
    for (int c : {0, 128}) {                                        // no survivor at all; every feature
        for (int v = 0; v < NW; ++v) pick(cs.w[v], c);
        run_case(n++, cs, out);
    }
    for (int i = 0; i < 3000; ++i) {                                // random 4x4 survivor words at mixed densities
        for (int v = 0; v < NW; ++v)
            for (int g = 0; g < 4; ++g) {
                uint32_t x = rnd() ^ (rnd() << 16);
                if (i % 3 == 1) x &= rnd() ^ (rnd() << 16);
                if (i % 3 == 2) x &= (rnd() ^ (rnd() << 16)) & (rnd() ^ (rnd() << 16));
                cs.w[v][g] = x;
            }
        run_case(n++, cs, out);
    }
    if (out) fclose(out);
    printf("cases %d bad %d\n", n, bad);
    return bad ? 1 : 0;
}
