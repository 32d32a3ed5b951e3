// Host harness of csrc/encode_cells.h (tests/test_encode_cpu.py): the three kernels of csrc/encode.hip as the loops of tests/fit_host.h over
// the policies the kernels take (EncExactRows; EncExactRule and EncLatentCols; EncNoPose).  Reads one binary file, writes one; all buffers
// have their exact sizes, so a sanitizer build sees any step outside them.
//   encode_host rows   IN OUT   IN: int64 head[9] = S B k draw seed iter L unit shape0 | int64 soff[B + 1] | float samples[S][4] | float z[B][L]
//                               OUT: float inputs[B k][L + 3] | float target[B k] | float zn[B][L] | int32 flags[B]
//   encode_host reduce IN OUT   IN: int64 head[9] = B k L Jstride clamp_bits 0 0 0 0 | float pred[B k] | float target[B k] | float J[B k][Jstride] | int32 flags[B]
//                               OUT: double loss[B] | double g_zn[B][L] | double part[B][chunks][L + 2] | int32 flags[B]
//   encode_host step   IN OUT   IN: int64 head[9] = B L unit t code_reg_bits lr_bits 0 0 0 | float z, m, v [B][L] | double g_zn[B][L] | int32 flags[B]
//                               OUT: float z, m, v [B][L] | int32 flags[B]
#include "../fit_host.h"

static int run_rows(FILE* in, FILE* out, const int64_t* head) {
    const int64_t S = head[0], k = head[2], iter = head[5];
    const int B = (int)head[1], draw = (int)head[3], L = (int)head[6], unit = (int)head[7], shape0 = (int)head[8];
    if (S < 0 || !host_sizes_ok(B, k, L)) return 2;
    std::vector<int64_t> soff(B + 1);
    std::vector<float> samples(S * 4), z((size_t)B * L);
    if (!read_all(in, soff, samples, z)) return 3;
    std::vector<float> inputs((size_t)B * k * (L + 3)), target((size_t)B * k), zn((size_t)B * L);
    std::vector<int32_t> flags(B);
    host_rows(samples, S, soff, B, shape0, k, draw, (uint64_t)head[4], iter, z, L, unit, EncExactRows{target.data(), nullptr}, inputs, zn, flags);
    return write_all(out, inputs, target, zn, flags) ? 0 : 4;
}

static int run_reduce(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[2], Jstride = (int)head[3];
    const int64_t k = head[1];
    if (!host_sizes_ok(B, k, L) || Jstride < L) return 2;
    const size_t n_all = (size_t)B * k;
    std::vector<float> pred(n_all), target(n_all), J(n_all * Jstride);
    std::vector<int32_t> flags(B);
    if (!read_all(in, pred, target, J, flags)) return 3;
    std::vector<double> part((size_t)B * enc_chunks(k) * (L + 2)), loss(B), g_zn((size_t)B * L);
    host_reduce(pred, EncExactRule{target.data()}, EncLatentCols{J.data(), Jstride}, L, B, k, bits_float(head[4]), part, loss, g_zn, flags);
    return write_all(out, loss, g_zn, part, flags) ? 0 : 4;
}

static int run_step(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[1], unit = (int)head[2], t = (int)head[3];
    if (!host_sizes_ok(B, 1, L) || t < 1) return 2;
    const size_t n = (size_t)B * L;
    std::vector<float> z(n), m(n), v(n);
    std::vector<double> g_zn(n);
    std::vector<int32_t> flags(B);
    if (!read_all(in, z, m, v, g_zn, flags)) return 3;
    host_step(z, m, v, L, B, unit, EncNoPose{}, g_zn, flags, bits_float(head[4]), bits_float(head[5]), t);
    return write_all(out, z, m, v, flags) ? 0 : 4;
}

static int run(const char* mode, FILE* in, FILE* out, const int64_t* head) {
    if (std::strcmp(mode, "rows") == 0) return run_rows(in, out, head);
    if (std::strcmp(mode, "reduce") == 0) return run_reduce(in, out, head);
    return std::strcmp(mode, "step") == 0 ? run_step(in, out, head) : 2;
}

int main(int argc, char** argv) { return host_main(argc, argv, 9, run); }     // (reduce and step use eight words and leave the ninth 0)
