// Per-element rules of the shape encoder (encode.hip): which sample a row takes, what a row contributes to its shape's loss and latent
// gradient, the order in which a chunk of rows is summed, and the gradient an Adam update of a latent element sees -- and, at the end, the
// policy structs through which the kernels of encode_kernels.h see them.  Plain functions and structs, compiled for the device by
// encode.hip and for the host by tests/encode_host/encode_host.cpp, which loops over every thread's work (tests/fit_host.h) and is compared
// with the numpy restatement (tests/_encode_ref.py) bit for bit.  DESIGN.md 7k has the rules.
#pragma once
#include <math.h>
#include <stdint.h>

#include "latent_cells.h"
#include "train_cells.h"

#define ENC_HD TRAIN_HD
#if defined(__HIPCC__)
#define ENC_HDM __host__ __device__ __forceinline__          // a member function of a policy struct
#else
#define ENC_HDM
#endif

#define ENC_THREADS 256          // threads of a workgroup of the rows, chunk, step and samples kernels
#define ENC_CHUNK 1024           // rows per partial sum: a constant, so the summation order is a function of k alone
#define ENC_SLOTS 64             // accumulators of a chunk: slot j sums the chunk's rows j, j + 64, ... in ascending order
#define ENC_COLS 32              // columns a workgroup folds at a time (LDS: ENC_SLOTS x ENC_COLS doubles)
#define ENC_MAX_L 256
#define ENC_MAX_K (1 << 20)
#define ENC_MAX_B 65535
#define ENC_MAX_ITER (1 << 24)

#define ENC_EMPTY 1              // flags: the shape has no samples; its rows are zero
#define ENC_NO_ROWS 2            //        no row with a finite prediction and target
#define ENC_SKIPPED 4            //        the latent was not stepped
#define ENC_BAD_TABLE 8          //        soff is broken at this shape, or draw = 0 with k > count; its rows are zero

ENC_HD uint64_t enc_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// samples of shape b, or -1 when the table is broken there (S: rows of the sample array)
ENC_HD int64_t enc_count(const int64_t* soff, int b, int64_t S) {
    const int64_t a = soff[b], e = soff[b + 1];
    return (a < 0 || e < a || e > S) ? -1 : e - a;
}

// the sample (relative to soff[b]) row s of shape b takes on iteration iter: with replacement, uniform up to the 2^-64 of the range reduction
ENC_HD int64_t enc_draw(uint64_t seed, int64_t iter, int b, int64_t s, int64_t count) {
    const uint64_t key = (uint64_t)iter << 40 | (uint64_t)(uint32_t)b << 24 | (uint64_t)s;
    return (int64_t)enc_mulhi64(train_mix64(seed ^ train_mix64(key * 0x9E3779B97F4A7C15ull + 1ull)), (uint64_t)count);
}

ENC_HD int64_t enc_chunks(int64_t k) { return (k + ENC_CHUNK - 1) / ENC_CHUNK; }

// What row (pred p, target t) adds to its shape: e = |clamp(p) - clamp(t)| in float64, w = sgn(clamp(p) - clamp(t)) [-clamp <= p <= clamp]
// (sgn(0) = 0: what torch.abs and torch.clamp differentiate to), ok = both finite.  A row that is not ok adds nothing.
struct EncRow {
    double e;
    float w;
    int ok;
};

ENC_HD EncRow enc_row(float p, float t, float clamp) {
    EncRow r;
    r.ok = (isfinite(p) && isfinite(t)) ? 1 : 0;
    r.e = 0.0;
    r.w = 0.f;
    if (r.ok) {
        const float cp = fminf(fmaxf(p, -clamp), clamp), ct = fminf(fmaxf(t, -clamp), clamp);
        const double d = (double)cp - (double)ct;
        r.e = fabs(d);
        const float sg = d > 0.0 ? 1.f : (d < 0.0 ? -1.f : 0.f);
        r.w = (p >= -clamp && p <= clamp) ? sg : 0.f;
    }
    return r;
}

// the row's term of gradient column c: w J, and nothing (not 0 x inf) where w is 0
ENC_HD double enc_term(float w, float j) { return w != 0.f ? (double)w * (double)j : 0.0; }

// Column c of the L + 2 a chunk sums: c < L the gradient column, c == L the loss, c == L + 1 the count of ok rows
ENC_HD double enc_value(int c, int L, float w, double e, int ok, const float* jrow) {
    if (c < L) return enc_term(w, jrow[c]);
    return c == L ? e : (ok ? 1.0 : 0.0);
}

// THE ORDER.  A chunk of n <= ENC_CHUNK rows: slot j < ENC_SLOTS holds the sum of rows j, j + ENC_SLOTS, ... taken in ascending order
// (0.0 for a slot without rows); then for o = 32, 16, .., 1, slot j < o takes slot j + o.  Slot 0 is the chunk's sum.  enc_slot_rows
// walks a slot; enc_tree_step is one addition of the tree (the device runs the j of one o in parallel, the host in a loop).
#define ENC_SLOT_ROWS(r, j, n) for (int r = (j); r < (n); r += ENC_SLOTS)
ENC_HD void enc_tree_step(double* slots, int stride, int j, int o) { slots[(int64_t)j * stride] += slots[(int64_t)(j + o) * stride]; }

// Chunk sums are folded in chunk order, then divided by the count (0 when the count is 0).
ENC_HD double enc_mean(double sum, double n_ok) { return n_ok > 0.0 ? sum / n_ok : 0.0; }

// The gradient element i of shape's raw latent z from g = the mean gradient with respect to what the decoder saw (rounded to float32):
// through the normalisation (nrm, dot of latent_cells.h) with unit, plus the regulariser code_reg ||z|| (nz = ||z||, 0 at z = 0) without
ENC_HD float enc_step_grad(float zi, float gi, int unit, float nrm, float dot, float nz, float code_reg) {
    if (unit) return latent_unit_grad(zi, gi, nrm, dot);
    return nz > 0.f ? gi + code_reg * (zi / nz) : gi;
}

// ||z|| without the floor, in index order (the regulariser's norm)
ENC_HD float enc_raw_norm(const float* z, int L) {
    float ss = 0.f;
    for (int c = 0; c < L; ++c) ss += z[c] * z[c];
    return sqrtf(ss);
}

// Adam's bias corrections for step t >= 1, formed in double as torch forms them and rounded once
ENC_HD void enc_bias(int t, float* bc1, float* bc2) {
    *bc1 = (float)(1.0 - pow(0.9, (double)t));
    *bc2 = (float)(1.0 - pow(0.999, (double)t));
}

// ---- the policies of the fits' kernels --------------------------------------------------------------------------------------------------------
// Plain structs of pointers and rules, instantiated by the kernels of encode_kernels.h and by a host program alike.
//
// A ROW POLICY of the rows kernel: W floats a sample; shape(b) what a workgroup keeps of its shape; flags() the shape's flag word; stage()
// stores the side arrays of row i (an index into the [B k] arrays) from sample `src` (a row of `samples`; -1: a zero row) and returns what
// the workgroup keeps of the row until the decoder's inputs are written; xyz() gives word a of the row's position from that.
// EncTargetRows: x y z and W - 3 target words, word 3 to t0, word 4 (W = 5) to t1; the position is read where it is written.
template <int WIDTH>
struct EncTargetRows {
    static constexpr int W = WIDTH;
    struct Shape {};
    typedef int64_t Staged;
    float *t0, *t1;
    ENC_HDM Shape shape(int) const { return Shape(); }
    ENC_HDM int32_t flags(const Shape&, bool bad, int64_t count) const { return bad ? ENC_BAD_TABLE : (count == 0 ? ENC_EMPTY : 0); }
    ENC_HDM Staged stage(const Shape&, const float* samples, int64_t src, int64_t i) const {
        t0[i] = src < 0 ? 0.f : samples[src * W + 3];
        if (W == 5) t1[i] = src < 0 ? 0.f : samples[src * W + 4];
        return src;
    }
    ENC_HDM float xyz(const float* samples, const Staged& src, int a) const { return samples[src * W + a]; }
};
typedef EncTargetRows<4> EncExactRows;

// A ROW RULE of the reduce gives the EncRow of row i of shape b from its prediction; a COLUMN RULE the value of column c < G + 2 of that row
// (G gradient columns, then the loss and the count of ok rows).  A column rule may keep EXTRA float64 words a row, written once per row
// (prepare) before the columns are summed: values that are costly and shared by no other row.  What is summed, and in which order, does not
// depend on where a value was formed.
struct EncExactRule {
    const float* target;
    ENC_HDM EncRow operator()(float p, int64_t i, int, float clamp) const { return enc_row(p, target[i], clamp); }
};

struct EncLatentCols {               // the latent fits: the latent columns of J, G = L
    static constexpr int EXTRA = 0;
    const float* J;
    int Jstride;
    ENC_HDM void prepare(double*, float, int64_t, int) const {}
    ENC_HDM double operator()(int c, int G, float w, double e, int ok, int64_t i, int, const double*) const {
        return enc_value(c, G, w, e, ok, J + i * Jstride);
    }
};

// A POSE POLICY of the step kernel: EXTRA gradient columns after the latent's, the flags that keep a shape from being stepped, ok() whatever
// else does, whether the latent is stepped at the rate lr, and the step of the pose itself (thread 0).  EncNoPose: a latent alone, which
// Adam visits at lr == 0 too (m and v move).
struct EncNoPose {
    static constexpr int EXTRA = 0;
    static constexpr int SKIP = ENC_EMPTY | ENC_NO_ROWS | ENC_BAD_TABLE;
    ENC_HDM bool ok(int, const double*, int, float, float) const { return true; }
    ENC_HDM bool steps_latent(float) const { return true; }
    ENC_HDM void step(int, const double*, int, float, float) const {}
};
