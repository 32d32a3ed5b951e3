// Integer rules of the decoder's training kernels (mlp_train.hip): the stateless dropout decision, the fixed row chunks of the weight
// gradient and the workspace layout.  Plain functions of integers, compiled for the device by mlp_train.hip and for the host by
// tests/prior_train_host/prior_train_host.cpp, which is compared with the numpy restatement (tests/_prior_train_ref.py) word for word.
// DESIGN.md 7j has the rules.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TRAIN_HD __host__ __device__ __forceinline__
#else
#define TRAIN_HD static inline
#endif

#define TRAIN_CHUNK 1024         // rows per partial of dW / db: a constant, so the summation order is a function of n alone
#define TRAIN_MAX_WIDTH 512      // largest out_dim of a layer
#define TRAIN_MAX_IN 1024        // largest in_dim of a layer (a hidden width plus re-injected columns)
#define TRAIN_HEADER_FLOATS 16   // words in front of the workspace: [0] float 1/(1-p) of the forward that filled it, [1] int32 drop_layers

TRAIN_HD uint64_t train_mix64(uint64_t z) {          // splitmix64 finaliser: synth_mix64 of synth_cells.h, restated so this header stands alone
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the 24-bit word of unit (layer, row, feature): the top 24 bits of mix64(seed ^ mix64((row << 14 | layer << 10 | feature) * golden + 1));
// layer < 16, feature < 1024
TRAIN_HD uint32_t train_drop_word(uint64_t seed, int layer, int64_t row, int feature) {
    const uint64_t key = (uint64_t)row << 14 | (uint64_t)(uint32_t)layer << 10 | (uint64_t)(uint32_t)feature;
    return (uint32_t)(train_mix64(seed ^ train_mix64(key * 0x9E3779B97F4A7C15ull + 1ull)) >> 40);
}

// the unit is kept when its word is >= threshold = rint(p 2^24) (train_drop_threshold, on the host); p = 0 takes no hash
TRAIN_HD bool train_keep(uint64_t seed, int layer, int64_t row, int feature, uint32_t threshold) {
    return train_drop_word(seed, layer, row, feature) >= threshold;
}

TRAIN_HD int64_t train_chunks(int64_t n) { return (n + TRAIN_CHUNK - 1) / TRAIN_CHUNK; }

// Workspace layout in floats, for n rows of the described decoder (nh = n_lin - 1 hidden layers):
//   header   TRAIN_HEADER_FLOATS words
//   x0       [n][in_dim[0]]                      the input rows
//   act[l]   [n][in_dim[l + 1]], l < nh          a_l in columns 0 .. out_dim[l] - 1, the re-injected input columns behind them
//   tail     [n][2]                              y1 (what the final tanh sees) and out = tanh(y1)
//   delta    2 x [n][max out_dim]                d_l, ping-pong
//   ginj[l]  [n][inj_n[l]], l >= 1               the re-injected columns' share of the input gradient
//   part     [chunks][out][in] then [chunks][out] of the layer the backward handled last (layer 0), sized for the largest layer
struct TrainLayout {
    int64_t x0, act[16], tail, delta[2], ginj[16], part, total;
};

TRAIN_HD TrainLayout train_layout(int n_lin, const int* in_dim, const int* out_dim, const int* inj_n, int64_t n) {
    TrainLayout L;
    int64_t at = TRAIN_HEADER_FLOATS;
    L.x0 = at;
    at += n * in_dim[0];
    int64_t max_out = 1, max_part = 0;
    for (int l = 0; l < 16; ++l) L.act[l] = L.ginj[l] = 0;
    for (int l = 0; l < n_lin; ++l) {
        if (l < n_lin - 1) {
            L.act[l] = at;
            at += n * in_dim[l + 1];
        }
        if (out_dim[l] > max_out) max_out = out_dim[l];
        const int64_t p = (int64_t)out_dim[l] * in_dim[l] + out_dim[l];
        if (p > max_part) max_part = p;
    }
    L.tail = at;
    at += 2 * n;
    L.delta[0] = at;
    L.delta[1] = at + n * max_out;
    at += 2 * n * max_out;
    for (int l = 1; l < n_lin; ++l) {
        L.ginj[l] = at;
        at += n * inj_n[l];
    }
    L.part = at;
    at += train_chunks(n) * max_part;
    L.total = at;
    return L;
}
