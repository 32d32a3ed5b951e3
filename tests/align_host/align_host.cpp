// Host harness of csrc/align_cells.h (tests/test_align_cpu.py): the kernels of csrc/align.hip as the loops of tests/fit_host.h over the
// policies the kernels take (the samples without a pose; AlnPosedRows; AlnRowRule and AlnCols; AlnPoseStep).  Reads one binary file, writes
// one; all buffers have their exact sizes, so a sanitizer build sees any step outside them.  int64 head[10] first.
//   align_host samples IN: head = N B F shape0 seed eta_bits s_max_bits has_normals | int64 ptoff[B + 1] | float origin[3] | float points[N][3] |
//                          double normals[N][3] (with has_normals)
//                      OUT: float rows[N (3 + F)][5] | int32 flags[B]
//   align_host rows    IN: head = S B k draw seed iter L unit shape0 | int64 soff[B + 1] | float samples[S][5] | float z[B][L] | float pose[B][6]
//                      OUT: float inputs[B k][L + 3] | float cam[B k][3] | float lo[B k] | float hi[B k] | float zn[B][L] | int32 flags[B]
//   align_host reduce  IN: head = B k L Jstride clamp_bits | float pred[B k] | float lo[B k] | float hi[B k] | float J[B k][Jstride] |
//                          float cam[B k][3] | float pose[B][6] | int32 flags[B]
//                      OUT: double loss[B] | double g[B][L + 5] | double part[B][chunks][L + 7] | int32 flags[B]
//   align_host step    IN: head = B L unit t code_reg_bits lr_bits | float lr_pose[5] | float z, m, v [B][L] | float theta, tm, tv [B][5] |
//                          float pose[B][6] | double g[B][L + 5] | int32 flags[B]
//                      OUT: float z, m, v [B][L] | float theta, tm, tv [B][5] | float pose[B][6] | int32 flags[B]
#include "../fit_host.h"

static int run_samples(FILE* in, FILE* out, const int64_t* head) {
    const int64_t N = head[0];
    const int B = (int)head[1], F = (int)head[2], shape0 = (int)head[3];
    const bool has_normals = head[7] != 0;
    if (N < 0 || B < 1 || F < 0 || F > CPL_MAX_FREE) return 2;
    std::vector<int64_t> ptoff(B + 1);
    std::vector<float> origin(3), points((size_t)N * 3), no_pose;
    std::vector<double> normals(has_normals ? (size_t)N * 3 : 0);
    if (!read_all(in, ptoff, origin, points, normals)) return 3;
    std::vector<float> rows((size_t)N * (3 + F) * ALN_ROW);
    std::vector<int32_t> flags(B);
    host_samples<false>(points, normals, has_normals, N, ptoff, B, no_pose, origin, shape0, F, bits_double(head[5]), bits_double(head[6]), (uint64_t)head[4],
                        rows, flags);
    return write_all(out, rows, flags) ? 0 : 4;
}

static int run_rows(FILE* in, FILE* out, const int64_t* head) {
    const int64_t S = head[0], k = head[2], iter = head[5];
    const int B = (int)head[1], draw = (int)head[3], L = (int)head[6], unit = (int)head[7], shape0 = (int)head[8];
    if (S < 0 || !host_sizes_ok(B, k, L)) return 2;
    std::vector<int64_t> soff(B + 1);
    std::vector<float> samples(S * ALN_ROW), z((size_t)B * L), pose((size_t)B * VERIFY_POSE);
    if (!read_all(in, soff, samples, z, pose)) return 3;
    std::vector<float> inputs((size_t)B * k * (L + 3)), cam((size_t)B * k * 3), lo((size_t)B * k), hi((size_t)B * k), zn((size_t)B * L);
    std::vector<int32_t> flags(B);
    host_rows(samples, S, soff, B, shape0, k, draw, (uint64_t)head[4], iter, z, L, unit, AlnPosedRows{pose.data(), cam.data(), lo.data(), hi.data()}, inputs, zn,
              flags);
    return write_all(out, inputs, cam, lo, hi, zn, flags) ? 0 : 4;
}

static int run_reduce(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[2], Jstride = (int)head[3];
    const int64_t k = head[1];
    if (!host_sizes_ok(B, k, L) || Jstride < L + 3) return 2;
    const size_t n_all = (size_t)B * k;
    std::vector<float> pred(n_all), lo(n_all), hi(n_all), J(n_all * Jstride), cam(n_all * 3), pose((size_t)B * VERIFY_POSE);
    std::vector<int32_t> flags(B);
    if (!read_all(in, pred, lo, hi, J, cam, pose, flags)) return 3;
    const int G = L + ALN_POSE;
    std::vector<double> part((size_t)B * enc_chunks(k) * (G + 2)), loss(B), g((size_t)B * G);
    host_reduce(pred, AlnRowRule{lo.data(), hi.data(), pose.data()}, AlnCols{pred.data(), J.data(), cam.data(), pose.data(), Jstride, L}, G, B, k,
                bits_float(head[4]), part, loss, g, flags);
    return write_all(out, loss, g, part, flags) ? 0 : 4;
}

static int run_step(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[1], unit = (int)head[2], t = (int)head[3];
    if (!host_sizes_ok(B, 1, L) || t < 1) return 2;
    std::vector<float> rates(ALN_POSE), z((size_t)B * L), m((size_t)B * L), v((size_t)B * L), theta((size_t)B * ALN_POSE), tm((size_t)B * ALN_POSE),
        tv((size_t)B * ALN_POSE), pose((size_t)B * VERIFY_POSE);
    std::vector<double> g((size_t)B * (L + ALN_POSE));
    std::vector<int32_t> flags(B);
    if (!read_all(in, rates, z, m, v, theta, tm, tv, pose, g, flags)) return 3;
    AlnPoseStep step{theta.data(), tm.data(), tv.data(), pose.data(), {0.f, 0.f, 0.f, 0.f, 0.f}};
    for (int i = 0; i < ALN_POSE; ++i) step.lr[i] = rates[i];
    host_step(z, m, v, L, B, unit, step, g, flags, bits_float(head[4]), bits_float(head[5]), t);
    return write_all(out, z, m, v, theta, tm, tv, pose, flags) ? 0 : 4;
}

static int run(const char* mode, FILE* in, FILE* out, const int64_t* head) {
    if (std::strcmp(mode, "samples") == 0) return run_samples(in, out, head);
    if (std::strcmp(mode, "rows") == 0) return run_rows(in, out, head);
    if (std::strcmp(mode, "reduce") == 0) return run_reduce(in, out, head);
    return std::strcmp(mode, "step") == 0 ? run_step(in, out, head) : 2;
}

int main(int argc, char** argv) { return host_main(argc, argv, 10, run); }
