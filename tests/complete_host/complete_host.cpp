// Host harness of csrc/complete_cells.h (tests/test_complete_cpu.py): the kernels of csrc/complete.hip with their workgroups and threads as
// loops, every per-element rule taken from the headers.  Reads one binary file, writes one; all buffers have their exact sizes, so a sanitizer
// build sees any step outside them.  int64 head[10] first.
//   complete_host row    IN: head = n clamp_bits | float p[n] | float lo[n] | float hi[n]
//                        OUT: per rule (cpl_row(p, lo, hi), cpl_row(p, lo, lo), enc_row(p, lo)): double e[n] | float w[n] | int32 ok[n]
//   complete_host view   IN: head = N B F shape0 seed eta_bits s_max_bits has_normals | int64 ptoff[B + 1] | float pose[B][6] | float origin[3] |
//                            float points[N][3] | double normals[N][3] (with has_normals)
//                        OUT: float rows[N (3 + F)][5] | int32 flags[B]
//   complete_host rows   IN: head = S B k draw seed iter L unit shape0 | int64 soff[B + 1] | float samples[S][5] | float z[B][L]
//                        OUT: float inputs[B k][L + 3] | float lo[B k] | float hi[B k] | float zn[B][L] | int32 flags[B]
//   complete_host reduce IN: head = B k L Jstride clamp_bits | float pred[B k] | float lo[B k] | float hi[B k] | float J[B k][Jstride] | int32 flags[B]
//                        OUT: double loss[B] | double g_zn[B][L] | double part[B][chunks][L + 2] | int32 flags[B]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "complete_cells.h"

#define THREADS 256

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_exact(FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }
static float bits_float(int64_t w) {
    const uint32_t u = (uint32_t)w;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static double bits_double(int64_t w) {
    double d;
    std::memcpy(&d, &w, 8);
    return d;
}

static int run_row(FILE* in, FILE* out, const int64_t* head) {
    const int64_t n = head[0];
    const float clamp = bits_float(head[1]);
    if (n < 0) return 2;
    std::vector<float> p(n), lo(n), hi(n);
    if (!read_exact(in, p.data(), n * 4) || !read_exact(in, lo.data(), n * 4) || !read_exact(in, hi.data(), n * 4)) return 3;
    for (int rule = 0; rule < 3; ++rule) {
        std::vector<double> e(n);
        std::vector<float> w(n);
        std::vector<int32_t> ok(n);
        for (int64_t i = 0; i < n; ++i) {
            const EncRow q = rule == 0 ? cpl_row(p[i], lo[i], hi[i], clamp) : (rule == 1 ? cpl_row(p[i], lo[i], lo[i], clamp) : enc_row(p[i], lo[i], clamp));
            e[i] = q.e, w[i] = q.w, ok[i] = q.ok;
        }
        if (!write_exact(out, e.data(), n * 8) || !write_exact(out, w.data(), n * 4) || !write_exact(out, ok.data(), n * 4)) return 4;
    }
    return 0;
}

static int run_view(FILE* in, FILE* out, const int64_t* head) {
    const int64_t N = head[0];
    const int B = (int)head[1], F = (int)head[2], shape0 = (int)head[3];
    const uint64_t seed = (uint64_t)head[4];
    const double eta = bits_double(head[5]), s_max = bits_double(head[6]);
    const bool has_normals = head[7] != 0;
    if (N < 0 || B < 1 || F < 0 || F > CPL_MAX_FREE) return 2;
    std::vector<int64_t> ptoff(B + 1);
    std::vector<float> pose((size_t)B * VERIFY_POSE), origin(3), points((size_t)N * 3);
    std::vector<double> normals(has_normals ? (size_t)N * 3 : 0);
    if (!read_exact(in, ptoff.data(), ptoff.size() * 8) || !read_exact(in, pose.data(), pose.size() * 4) || !read_exact(in, origin.data(), 12) ||
        !read_exact(in, points.data(), points.size() * 4) || !read_exact(in, normals.data(), normals.size() * 8))
        return 3;
    const int P = 3 + F;
    std::vector<float> rows((size_t)N * P * CPL_ROW);
    std::vector<int32_t> flags(B);
    const int64_t threads = N > B ? N : (int64_t)B;
    for (int64_t g = 0; g < threads; ++g) {                                          // sdfr_view_samples_kernel, thread g
        if (g < B) flags[g] = cpl_view_flags(ptoff.data(), pose.data(), (int)g, N);
        if (g >= N) continue;
        const int b = cpl_owner(ptoff.data(), B, N, g);
        const int bb = b < 0 ? 0 : b;
        const bool usable = b >= 0 && cpl_pose_ok(pose.data() + VERIFY_POSE * bb);
        // exact-size copies of what the thread may read: the sanitizer build sees a step outside the point's own words
        std::vector<float> p(points.begin() + 3 * g, points.begin() + 3 * g + 3), ps(pose.begin() + VERIFY_POSE * bb, pose.begin() + VERIFY_POSE * (bb + 1));
        std::vector<double> n;
        if (has_normals) n.assign(normals.begin() + 3 * g, normals.begin() + 3 * g + 3);
        std::vector<float> o((size_t)P * CPL_ROW);
        cpl_view_row(p.data(), has_normals ? n.data() : nullptr, ps.data(), origin.data(), usable, seed, shape0 + bb, b < 0 ? 0 : g - ptoff[b], F, eta, s_max,
                     o.data());
        std::memcpy(rows.data() + (size_t)g * P * CPL_ROW, o.data(), o.size() * 4);
    }
    return write_exact(out, rows.data(), rows.size() * 4) && write_exact(out, flags.data(), flags.size() * 4) ? 0 : 4;
}

static int run_rows(FILE* in, FILE* out, const int64_t* head) {
    const int W = 5;
    const int64_t S = head[0], k = head[2], iter = head[5];
    const int B = (int)head[1], draw = (int)head[3], L = (int)head[6], unit = (int)head[7], shape0 = (int)head[8];
    const uint64_t seed = (uint64_t)head[4];
    if (S < 0 || B < 0 || B > ENC_MAX_B || k < 1 || k > ENC_MAX_K || L < 1 || L > ENC_MAX_L) return 2;
    const int NI = L + 3;
    std::vector<int64_t> soff(B + 1);
    std::vector<float> samples(S * W), z((size_t)B * L);
    if (!read_exact(in, soff.data(), soff.size() * 8) || !read_exact(in, samples.data(), samples.size() * 4) || !read_exact(in, z.data(), z.size() * 4))
        return 3;
    std::vector<float> inputs((size_t)B * k * NI), lo((size_t)B * k), hi((size_t)B * k), zn((size_t)B * L);
    std::vector<int32_t> flags(B);
    const int64_t blocks = (k + THREADS - 1) / THREADS;
    for (int b = 0; b < B; ++b)
        for (int64_t bx = 0; bx < blocks; ++bx) {                                    // enc_rows_kernel<5>, workgroup (bx, b)
            std::vector<float> s_zn(L);
            std::vector<int64_t> s_src(THREADS);
            const int64_t count = enc_count(soff.data(), b, S);
            const bool bad = count < 0 || (!draw && count > 0 && k > count);
            const bool zero = bad || count == 0;
            const float nrm = unit ? latent_norm(z.data() + (size_t)b * L, L) : 1.f;
            for (int tid = 0; tid < L; ++tid) {
                const float v = unit ? z[(size_t)b * L + tid] / nrm : z[(size_t)b * L + tid];
                s_zn[tid] = v;
                if (bx == 0) zn[(size_t)b * L + tid] = v;
            }
            if (bx == 0) flags[b] = bad ? ENC_BAD_TABLE : (count == 0 ? ENC_EMPTY : 0);
            const int64_t s0 = bx * THREADS;
            const int rows = (int)((k - s0) < THREADS ? (k - s0) : THREADS);
            for (int tid = 0; tid < rows; ++tid) {
                const int64_t s = s0 + tid;
                const int64_t src = zero ? -1 : soff[b] + (draw ? enc_draw(seed, iter, shape0 + b, s, count) : s);
                s_src[tid] = src;
                lo[(size_t)b * k + s] = zero ? 0.f : samples.at((size_t)src * W + 3);
                hi[(size_t)b * k + s] = zero ? 0.f : samples.at((size_t)src * W + 4);
            }
            float* o = inputs.data() + ((size_t)b * k + s0) * NI;
            for (int e = 0; e < rows * NI; ++e) {
                const int r = e / NI, c = e - r * NI;
                o[e] = zero ? 0.f : (c < L ? s_zn[c] : samples.at((size_t)s_src[r] * W + (c - L)));
            }
        }
    return write_exact(out, inputs.data(), inputs.size() * 4) && write_exact(out, lo.data(), lo.size() * 4) && write_exact(out, hi.data(), hi.size() * 4) &&
                   write_exact(out, zn.data(), zn.size() * 4) && write_exact(out, flags.data(), flags.size() * 4) ? 0 : 4;
}

static int run_reduce(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[2], Jstride = (int)head[3];
    const int64_t k = head[1];
    const float clamp = bits_float(head[4]);
    if (B < 0 || B > ENC_MAX_B || k < 1 || k > ENC_MAX_K || L < 1 || L > ENC_MAX_L || Jstride < L) return 2;
    const size_t n_all = (size_t)B * k;
    std::vector<float> pred(n_all), lo(n_all), hi(n_all), J(n_all * Jstride);
    std::vector<int32_t> flags(B);
    if (!read_exact(in, pred.data(), n_all * 4) || !read_exact(in, lo.data(), n_all * 4) || !read_exact(in, hi.data(), n_all * 4) ||
        !read_exact(in, J.data(), J.size() * 4) || !read_exact(in, flags.data(), flags.size() * 4))
        return 3;
    const int64_t chunks = enc_chunks(k);
    const int NC = L + 2;
    std::vector<double> part((size_t)B * chunks * NC), loss(B), g_zn((size_t)B * L);
    for (int b = 0; b < B; ++b)
        for (int64_t ch = 0; ch < chunks; ++ch) {                                  // enc_chunk_kernel<CplBoundRule>, workgroup (ch, b)
            const int64_t row0 = ch * ENC_CHUNK;
            const int n = (int)((k - row0) < ENC_CHUNK ? (k - row0) : ENC_CHUNK);
            const size_t base = (size_t)b * k + row0;
            std::vector<double> s_e(n), s_acc((size_t)ENC_SLOTS * (ENC_COLS + 1));
            std::vector<float> s_w(n);
            std::vector<unsigned char> s_ok(n);
            for (int r = 0; r < n; ++r) {
                const EncRow q = cpl_row(pred[base + r], lo[base + r], hi[base + r], clamp);
                s_e[r] = q.e; s_w[r] = q.w; s_ok[r] = (unsigned char)q.ok;
            }
            for (int c0 = 0; c0 < NC; c0 += ENC_COLS) {
                const int nc = (NC - c0) < ENC_COLS ? (NC - c0) : ENC_COLS;
                for (int e = 0; e < ENC_SLOTS * nc; ++e) {
                    const int j = e / nc, c = c0 + (e - j * nc);
                    double a = 0.0;
                    ENC_SLOT_ROWS(r, j, n) a += enc_value(c, L, s_w[r], s_e[r], s_ok[r], J.data() + (base + r) * Jstride);
                    s_acc[(size_t)j * (ENC_COLS + 1) + (c - c0)] = a;
                }
                for (int o = ENC_SLOTS / 2; o > 0; o >>= 1)
                    for (int e = 0; e < o * nc; ++e) {
                        const int j = e / nc, cc = e - j * nc;
                        enc_tree_step(s_acc.data() + cc, ENC_COLS + 1, j, o);
                    }
                for (int c = 0; c < nc; ++c) part[((size_t)b * chunks + ch) * NC + c0 + c] = s_acc[c];
            }
        }
    for (int b = 0; b < B; ++b) {                                                    // enc_fold_kernel, workgroup b
        std::vector<double> tot(NC);
        for (int c = 0; c < NC; ++c) {
            double a = 0.0;
            for (int64_t ch = 0; ch < chunks; ++ch) a += part[((size_t)b * chunks + ch) * NC + c];
            tot[c] = a;
        }
        const double n_ok = tot[L + 1];
        for (int c = 0; c < L; ++c) g_zn[(size_t)b * L + c] = enc_mean(tot[c], n_ok);
        loss[b] = enc_mean(tot[L], n_ok);
        if (!(n_ok > 0.0)) flags[b] |= ENC_NO_ROWS;
    }
    return write_exact(out, loss.data(), loss.size() * 8) && write_exact(out, g_zn.data(), g_zn.size() * 8) &&
                   write_exact(out, part.data(), part.size() * 8) && write_exact(out, flags.data(), flags.size() * 4) ? 0 : 4;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int64_t head[10];
    int rc = 3;
    if (read_exact(in, head, sizeof(head))) {
        if (std::strcmp(argv[1], "row") == 0) rc = run_row(in, out, head);
        else if (std::strcmp(argv[1], "view") == 0) rc = run_view(in, out, head);
        else if (std::strcmp(argv[1], "rows") == 0) rc = run_rows(in, out, head);
        else if (std::strcmp(argv[1], "reduce") == 0) rc = run_reduce(in, out, head);
        else rc = 2;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? rc : 4;
}
