// Host harness of csrc/search_cells.h (tests/test_search_cpu.py): the kernels of csrc/search.hip as the loops of tests/fit_host.h over the
// policies the kernels take (SrchRows over CplBoundRows / SrchPosedRows; CplBoundRule / AlnRowRule and SrchLossCols), and the select
// kernel's workgroup as a loop over the rules of search_cells.h.  A start is a workgroup row of its own: the rows loop runs once per start
// on the two table words of the shape srch_owner gives it, as enc_rows_kernel does with a policy that has an owner.  Reads one binary
// file, writes one; all buffers have their exact sizes, so a sanitizer build sees any step outside them.  int64 head[12] first.
//   search_host rows   IN: head = S B N k draw seed iter L unit shape0 posed want_cam | int64 soff[B + 1] | int32 own[N] | float samples[S][5] |
//                          float z[N][L] | float pose[N][6] (with posed)
//                      OUT: float inputs[N k][L + 3] | float cam[N k][3] (with posed and want_cam) | float lo[N k] | float hi[N k] | float zn[N][L] |
//                           int32 flags[N]
//   search_host reduce IN: head = N k clamp_bits posed | float pred[N k] | float lo[N k] | float hi[N k] | int32 flags[N] | float pose[N][6] (with posed)
//                      OUT: double loss[N] | double part[N][chunks][2] | int32 flags[N]
//   search_host select IN: head = B N keep n (the words loss and flags really hold) | int64 coff[B + 1] | double loss[n] | int32 flags[n]
//                      OUT: int32 order[B][keep] | int32 count[B]
#include <algorithm>

#include "../fit_host.h"
#include "search_cells.h"

template <class Inner>
static void start_rows(const Inner& inner, const std::vector<float>& samples, int64_t S, const int64_t* table, int shape0, int64_t k, int draw, uint64_t seed,
                       int64_t iter, const std::vector<float>& z1, int L, int unit, std::vector<float>& in1, std::vector<float>& zn1, std::vector<int32_t>& fl1) {
    const std::vector<int64_t> soff1(table, table + 2);
    const int32_t own1[1] = {0};
    host_rows(samples, S, soff1, 1, shape0, k, draw, seed, iter, z1, L, unit, SrchRows<Inner>{inner, own1, 1}, in1, zn1, fl1);
}

static int run_rows(FILE* in, FILE* out, const int64_t* head) {
    const int64_t S = head[0], k = head[3], iter = head[6];
    const int B = (int)head[1], N = (int)head[2], draw = (int)head[4], L = (int)head[7], unit = (int)head[8], shape0 = (int)head[9];
    const bool posed = head[10] != 0, want_cam = posed && head[11] != 0;
    if (S < 0 || B < 0 || !host_sizes_ok(N, k, L)) return 2;
    std::vector<int64_t> soff(B + 1);
    std::vector<int32_t> own(N);
    std::vector<float> samples(S * CPL_ROW), z((size_t)N * L), pose(posed ? (size_t)N * VERIFY_POSE : 0);
    if (!read_all(in, soff, own, samples, z, pose)) return 3;
    std::vector<float> inputs((size_t)N * k * (L + 3)), cam(want_cam ? (size_t)N * k * 3 : 0), lo((size_t)N * k), hi((size_t)N * k), zn((size_t)N * L);
    std::vector<int32_t> flags(N);
    const int64_t none[2] = {0, -1};                                 // a table entry the rows loop refuses: what a start without an owner sees
    for (int s = 0; s < N; ++s) {
        const int o = SrchRows<CplBoundRows>{CplBoundRows{nullptr, nullptr}, own.data(), B}.owner(s);        // the hook enc_rows_kernel asks
        const int64_t* table = o < 0 ? none : soff.data() + o;
        std::vector<float> z1(z.begin() + (size_t)s * L, z.begin() + (size_t)(s + 1) * L), in1((size_t)k * (L + 3)), lo1(k), hi1(k), zn1(L), cam1(want_cam ? k * 3 : 0);
        std::vector<int32_t> fl1(1);
        if (posed) {
            const std::vector<float> ps(pose.begin() + (size_t)s * VERIFY_POSE, pose.begin() + (size_t)(s + 1) * VERIFY_POSE);
            SrchPosedRows inner;
            inner.pose = ps.data(), inner.cam = want_cam ? cam1.data() : nullptr, inner.lo = lo1.data(), inner.hi = hi1.data();
            start_rows(inner, samples, S, table, shape0 + (o < 0 ? 0 : o), k, draw, (uint64_t)head[5], iter, z1, L, unit, in1, zn1, fl1);
        } else {
            start_rows(CplBoundRows{lo1.data(), hi1.data()}, samples, S, table, shape0 + (o < 0 ? 0 : o), k, draw, (uint64_t)head[5], iter, z1, L, unit, in1, zn1,
                       fl1);
        }
        std::copy(in1.begin(), in1.end(), inputs.begin() + (size_t)s * k * (L + 3));
        std::copy(cam1.begin(), cam1.end(), cam.begin() + (want_cam ? (size_t)s * k * 3 : 0));
        std::copy(lo1.begin(), lo1.end(), lo.begin() + (size_t)s * k);
        std::copy(hi1.begin(), hi1.end(), hi.begin() + (size_t)s * k);
        std::copy(zn1.begin(), zn1.end(), zn.begin() + (size_t)s * L);
        flags[s] = fl1[0];
    }
    return write_all(out, inputs, cam, lo, hi, zn, flags) ? 0 : 4;
}

static int run_reduce(FILE* in, FILE* out, const int64_t* head) {
    const int N = (int)head[0];
    const int64_t k = head[1];
    const bool posed = head[3] != 0;
    if (!host_sizes_ok(N, k, 1)) return 2;
    const size_t n_all = (size_t)N * k;
    std::vector<float> pred(n_all), lo(n_all), hi(n_all), pose(posed ? (size_t)N * VERIFY_POSE : 0);
    std::vector<int32_t> flags(N);
    if (!read_all(in, pred, lo, hi, flags, pose)) return 3;
    std::vector<double> part((size_t)N * enc_chunks(k) * 2), loss(N), g;
    if (posed)
        host_reduce(pred, AlnRowRule{lo.data(), hi.data(), pose.data()}, SrchLossCols(), 0, N, k, bits_float(head[2]), part, loss, g, flags);
    else
        host_reduce(pred, CplBoundRule{lo.data(), hi.data()}, SrchLossCols(), 0, N, k, bits_float(head[2]), part, loss, g, flags);
    return write_all(out, loss, part, flags) ? 0 : 4;
}

// srch_select_kernel, workgroup b
static int run_select(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], keep = (int)head[2];
    const int64_t N = head[1], n_words = head[3];
    if (B < 0 || N < 0 || n_words < 0 || keep < 1 || keep > SRCH_MAX_KEEP) return 2;
    std::vector<int64_t> coff(B + 1);
    std::vector<double> loss(n_words);
    std::vector<int32_t> flags(n_words);
    if (!read_all(in, coff, loss, flags)) return 3;
    std::vector<int32_t> order((size_t)B * keep), count(B);
    for (int b = 0; b < B; ++b) {
        int32_t* ob = order.data() + (size_t)b * keep;
        const int64_t cnt = srch_count(coff.data(), b, N);
        if (cnt < 0) {
            for (int r = 0; r < keep; ++r) ob[r] = -1;
            count[b] = -1;
            continue;
        }
        const int n = (int)cnt;
        const int64_t c0 = coff[b];
        std::vector<double> s_loss(n);
        std::vector<unsigned char> s_ok(n);
        int usable = 0;
        for (int i = 0; i < n; ++i) {
            const double l = loss.data()[c0 + i];                    // (no .at(): the sanitizer build is what watches these reads)
            const bool ok = srch_usable(flags.data()[c0 + i], l);
            s_loss[i] = l, s_ok[i] = ok ? 1 : 0, usable += ok ? 1 : 0;
        }
        const int kept = usable < keep ? usable : keep;
        count[b] = kept;
        for (int r = kept; r < keep; ++r) ob[r] = -1;
        for (int i = 0; i < n; ++i) {
            if (!s_ok[i]) continue;
            const int r = srch_rank(s_loss.data(), s_ok.data(), n, i);
            if (r < keep) ob[r] = (int32_t)(c0 + i);
        }
    }
    return write_all(out, order, count) ? 0 : 4;
}

static int run(const char* mode, FILE* in, FILE* out, const int64_t* head) {
    if (std::strcmp(mode, "rows") == 0) return run_rows(in, out, head);
    if (std::strcmp(mode, "reduce") == 0) return run_reduce(in, out, head);
    return std::strcmp(mode, "select") == 0 ? run_select(in, out, head) : 2;
}

int main(int argc, char** argv) { return host_main(argc, argv, 12, run); }
