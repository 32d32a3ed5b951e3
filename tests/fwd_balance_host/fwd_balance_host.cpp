// Host harness of csrc/tile_balance.h (tests/test_fwd_balance_cpu.py): the ranking of sdfr_tile_balance_kernel entry by entry, as the kernel
// walks it -- the costs copied (the kernel's LDS copy), a rank per chunk summed from the 64 parts the lanes of a wave count, then every entry of the static order to sdfr_tb_dest -- on buffers of
// exactly the sizes the state has, so that the sanitizer build faults on any index outside them.
//   fwd_balance_host IN OUT     IN: int32 records [order_rows, cost[T], fixed[order_rows]] back to back, T = sdfr_tb_chunks(order_rows)
//                               OUT: per record next[order_rows], then last[T], cost[T], at[T] as the kernel leaves them
// Prints "cases N bad B": B counts records where an entry of next[] was written twice or never, or where sdfr_tb_next_order_host disagrees.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tile_balance.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> in;
    int32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    size_t at = 0;
    int cases = 0, bad = 0;
    while (at < in.size()) {
        const int64_t order_rows = in[at++];
        const int64_t T = sdfr_tb_chunks(order_rows), full = sdfr_tb_full_chunks(order_rows);
        if (order_rows <= 0 || at + (size_t)(T + order_rows) > in.size() || !sdfr_tb_ranked(order_rows)) return 3;
        if (sdfr_tb_state_words(order_rows) != 3 * T + SDFR_TB_CTL + 2 * order_rows || sdfr_tb_fixed_word(order_rows) - sdfr_tb_order_word(order_rows) != order_rows ||
            sdfr_tb_last_word(order_rows) != T || sdfr_tb_at_word(order_rows) != 2 * T || sdfr_tb_ctl_word(order_rows) != 3 * T || sdfr_tb_order_word(order_rows) != 3 * T + SDFR_TB_CTL) return 4;
        // the state, one exact-size allocation per field
        std::vector<int32_t> g_cost(in.begin() + at, in.begin() + at + T);
        at += T;
        std::vector<int32_t> fixed(in.begin() + at, in.begin() + at + order_rows);
        at += order_rows;
        std::vector<int32_t> g_last(T, -1), g_at(T, -1), order(order_rows, -1), cost(T), rank(T), expect(order_rows, -2), expect_at(T, -2);
        std::vector<int> written(order_rows, 0);
        sdfr_tb_next_order_host(g_cost.data(), fixed.data(), expect.data(), expect_at.data(), order_rows);
        for (int64_t c = 0; c < T; ++c) { cost[c] = g_cost[c]; g_last[c] = g_cost[c]; g_cost[c] = 0; }
        for (int64_t c = 0; c < T; ++c) {
            int r = (int)c;
            if (c < full) {
                r = 0;
                for (int lane = 0; lane < 64; ++lane) r += sdfr_tb_rank_part(cost.data(), (int)full, (int)c, lane, 64);
            }
            rank[c] = r;
            g_at.at((size_t)rank[c]) = (int32_t)c;
        }
        for (int64_t i = 0; i < order_rows; ++i) {
            const int64_t c = i / SDFR_TB_CHUNK;
            const int64_t d = sdfr_tb_dest(c, rank[c], (int)(i - c * SDFR_TB_CHUNK), full);
            order.at((size_t)d) = fixed[i];
            ++written.at((size_t)d);
        }
        bool ok = true;
        for (int64_t i = 0; i < order_rows; ++i) ok = ok && written[i] == 1 && order[i] == expect[i];
        for (int64_t c = 0; c < T; ++c) ok = ok && g_at[c] == expect_at[c] && rank[g_at[c]] == (int)c;
        // a tile of a one-crop launch sits at its own place; the cost word is at[place] unless that names no chunk
        for (int64_t t = 0; t < T; ++t) ok = ok && sdfr_tb_place_of_tile(t, order_rows) == (int)t;
        if (order_rows % SDFR_TB_CHUNK == 0)
            for (int64_t t = 0; t < 3 * T; ++t) ok = ok && sdfr_tb_place_of_tile(t, order_rows) == (int)(t % T);
        ok = ok && sdfr_tb_cost_index((int)T - 1, 0, order_rows) == (int)T - 1 && sdfr_tb_cost_index((int)T, 5, order_rows) == 5 &&
             sdfr_tb_cost_index(-1, 7, order_rows) == 7;
        // the cost of a layer: its survivors padded to the k list's granule of 16
        for (int sv = 0; sv <= 512; ++sv) ok = ok && sdfr_tb_layer_cost(sv) == (sv + 15) / 16 * 16 && sdfr_tb_layer_cost(sv) == sdfr_kc_padded(sv);
        bad += ok ? 0 : 1;
        ++cases;
        fwrite(order.data(), 4, order.size(), o);
        fwrite(g_last.data(), 4, g_last.size(), o);
        fwrite(g_cost.data(), 4, g_cost.size(), o);
        fwrite(g_at.data(), 4, g_at.size(), o);
    }
    fclose(o);
    printf("cases %d bad %d\n", cases, bad);
    return 0;
}
