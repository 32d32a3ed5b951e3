// Host harness of csrc/train_cells.h (tests/test_prior_train_cpu.py): the dropout words and decisions of a block of units, the chunk count
// and the workspace layout of a described decoder, printed as integers for the comparison with tests/_prior_train_ref.py.
//   prior_train_host hash SEED LAYER ROW0 ROWS WIDTH THRESHOLD     -> ROWS x WIDTH lines "word keep"
//   prior_train_host layout N N_LIN in_dim... out_dim... inj_n...  -> chunks x0 act... tail delta0 delta1 ginj... part total
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "train_cells.h"

int main(int argc, char** argv) {
    if (argc >= 8 && std::strcmp(argv[1], "hash") == 0) {
        const uint64_t seed = std::strtoull(argv[2], nullptr, 0);
        const int layer = std::atoi(argv[3]);
        const int64_t row0 = std::atoll(argv[4]), rows = std::atoll(argv[5]);
        const int width = std::atoi(argv[6]);
        const uint32_t thr = (uint32_t)std::strtoul(argv[7], nullptr, 0);
        for (int64_t r = row0; r < row0 + rows; ++r)
            for (int j = 0; j < width; ++j)
                std::printf("%u %d\n", train_drop_word(seed, layer, r, j), train_keep(seed, layer, r, j, thr) ? 1 : 0);
        return 0;
    }
    if (argc >= 4 && std::strcmp(argv[1], "layout") == 0) {
        const int64_t n = std::atoll(argv[2]);
        const int n_lin = std::atoi(argv[3]);
        if (n_lin < 1 || n_lin > 16 || argc != 4 + 3 * n_lin) return 2;
        std::vector<int> in_dim(n_lin), out_dim(n_lin), inj_n(n_lin);
        for (int l = 0; l < n_lin; ++l) {
            in_dim[l] = std::atoi(argv[4 + l]);
            out_dim[l] = std::atoi(argv[4 + n_lin + l]);
            inj_n[l] = std::atoi(argv[4 + 2 * n_lin + l]);
        }
        const TrainLayout L = train_layout(n_lin, in_dim.data(), out_dim.data(), inj_n.data(), n);
        std::printf("%lld %lld", (long long)train_chunks(n), (long long)L.x0);
        for (int l = 0; l < n_lin - 1; ++l) std::printf(" %lld", (long long)L.act[l]);
        std::printf(" %lld %lld %lld", (long long)L.tail, (long long)L.delta[0], (long long)L.delta[1]);
        for (int l = 1; l < n_lin; ++l) std::printf(" %lld", (long long)L.ginj[l]);
        std::printf(" %lld %lld\n", (long long)L.part, (long long)L.total);
        return 0;
    }
    return 2;
}
