// Host harness of csrc/complete_cells.h (tests/test_complete_cpu.py): the kernels of csrc/complete.hip as the loops of tests/fit_host.h over
// the policies the kernels take (the posed samples; CplBoundRows; CplBoundRule and EncLatentCols).  Reads one binary file, writes one; all
// buffers have their exact sizes, so a sanitizer build sees any step outside them.  int64 head[10] first.
//   complete_host row    IN: head = n clamp_bits | float p[n] | float lo[n] | float hi[n]
//                        OUT: per rule (cpl_row(p, lo, hi), cpl_row(p, lo, lo), enc_row(p, lo)): double e[n] | float w[n] | int32 ok[n]
//   complete_host view   IN: head = N B F shape0 seed eta_bits s_max_bits has_normals | int64 ptoff[B + 1] | float pose[B][6] | float origin[3] |
//                            float points[N][3] | double normals[N][3] (with has_normals)
//                        OUT: float rows[N (3 + F)][5] | int32 flags[B]
//   complete_host rows   IN: head = S B k draw seed iter L unit shape0 | int64 soff[B + 1] | float samples[S][5] | float z[B][L]
//                        OUT: float inputs[B k][L + 3] | float lo[B k] | float hi[B k] | float zn[B][L] | int32 flags[B]
//   complete_host reduce IN: head = B k L Jstride clamp_bits | float pred[B k] | float lo[B k] | float hi[B k] | float J[B k][Jstride] | int32 flags[B]
//                        OUT: double loss[B] | double g_zn[B][L] | double part[B][chunks][L + 2] | int32 flags[B]
#include "../fit_host.h"

static int run_row(FILE* in, FILE* out, const int64_t* head) {
    const int64_t n = head[0];
    const float clamp = bits_float(head[1]);
    if (n < 0) return 2;
    std::vector<float> p(n), lo(n), hi(n);
    if (!read_all(in, p, lo, hi)) return 3;
    for (int rule = 0; rule < 3; ++rule) {
        std::vector<double> e(n);
        std::vector<float> w(n);
        std::vector<int32_t> ok(n);
        for (int64_t i = 0; i < n; ++i) {
            const EncRow q = rule == 0 ? cpl_row(p[i], lo[i], hi[i], clamp) : (rule == 1 ? cpl_row(p[i], lo[i], lo[i], clamp) : enc_row(p[i], lo[i], clamp));
            e[i] = q.e, w[i] = q.w, ok[i] = q.ok;
        }
        if (!write_all(out, e, w, ok)) return 4;
    }
    return 0;
}

static int run_view(FILE* in, FILE* out, const int64_t* head) {
    const int64_t N = head[0];
    const int B = (int)head[1], F = (int)head[2], shape0 = (int)head[3];
    const bool has_normals = head[7] != 0;
    if (N < 0 || B < 1 || F < 0 || F > CPL_MAX_FREE) return 2;
    std::vector<int64_t> ptoff(B + 1);
    std::vector<float> pose((size_t)B * VERIFY_POSE), origin(3), points((size_t)N * 3);
    std::vector<double> normals(has_normals ? (size_t)N * 3 : 0);
    if (!read_all(in, ptoff, pose, origin, points, normals)) return 3;
    std::vector<float> rows((size_t)N * (3 + F) * CPL_ROW);
    std::vector<int32_t> flags(B);
    host_samples<true>(points, normals, has_normals, N, ptoff, B, pose, origin, shape0, F, bits_double(head[5]), bits_double(head[6]), (uint64_t)head[4], rows,
                       flags);
    return write_all(out, rows, flags) ? 0 : 4;
}

static int run_rows(FILE* in, FILE* out, const int64_t* head) {
    const int64_t S = head[0], k = head[2], iter = head[5];
    const int B = (int)head[1], draw = (int)head[3], L = (int)head[6], unit = (int)head[7], shape0 = (int)head[8];
    if (S < 0 || !host_sizes_ok(B, k, L)) return 2;
    std::vector<int64_t> soff(B + 1);
    std::vector<float> samples(S * CPL_ROW), z((size_t)B * L);
    if (!read_all(in, soff, samples, z)) return 3;
    std::vector<float> inputs((size_t)B * k * (L + 3)), lo((size_t)B * k), hi((size_t)B * k), zn((size_t)B * L);
    std::vector<int32_t> flags(B);
    host_rows(samples, S, soff, B, shape0, k, draw, (uint64_t)head[4], iter, z, L, unit, CplBoundRows{lo.data(), hi.data()}, inputs, zn, flags);
    return write_all(out, inputs, lo, hi, zn, flags) ? 0 : 4;
}

static int run_reduce(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[2], Jstride = (int)head[3];
    const int64_t k = head[1];
    if (!host_sizes_ok(B, k, L) || Jstride < L) return 2;
    const size_t n_all = (size_t)B * k;
    std::vector<float> pred(n_all), lo(n_all), hi(n_all), J(n_all * Jstride);
    std::vector<int32_t> flags(B);
    if (!read_all(in, pred, lo, hi, J, flags)) return 3;
    std::vector<double> part((size_t)B * enc_chunks(k) * (L + 2)), loss(B), g_zn((size_t)B * L);
    host_reduce(pred, CplBoundRule{lo.data(), hi.data()}, EncLatentCols{J.data(), Jstride}, L, B, k, bits_float(head[4]), part, loss, g_zn, flags);
    return write_all(out, loss, g_zn, part, flags) ? 0 : 4;
}

static int run(const char* mode, FILE* in, FILE* out, const int64_t* head) {
    if (std::strcmp(mode, "row") == 0) return run_row(in, out, head);
    if (std::strcmp(mode, "view") == 0) return run_view(in, out, head);
    if (std::strcmp(mode, "rows") == 0) return run_rows(in, out, head);
    return std::strcmp(mode, "reduce") == 0 ? run_reduce(in, out, head) : 2;
}

int main(int argc, char** argv) { return host_main(argc, argv, 10, run); }
