// Per-element rules of the search for a fit's start (search.hip): many candidate starts (a latent, and with a pose a pose row) share the
// samples of one shape, are scored on the SAME drawn rows of it by the loss alone, and are ranked per shape.  Here: which shape a start
// draws from, the row policies of the rows kernel for a start (SrchRows wraps the fits' own policy and adds the owner; SrchPosedRows is
// AlnPosedRows with an optional camera array), the column rule of a reduce without gradient columns, and the rules of the ranking -- which
// starts are usable and which of two comes first.  Plain functions and structs, compiled for the device by search.hip and for the host by
// tests/search_host/search_host.cpp, which is compared with the numpy restatement (tests/_search_ref.py) bit for bit.  Every operation
// rounds on its own (-ffp-contract=off).  DESIGN.md 7p has the rules.
#pragma once
#include <math.h>
#include <stdint.h>

#include "align_cells.h"

#define SRCH_MAX_KEEP 64         // ranks kept per shape at the most
#define SRCH_MAX_STARTS 4096     // starts of one shape at the most: the workgroup keeps their losses in LDS (32 KB of float64)
#define SRCH_THREADS 256         // threads of the select kernel's workgroup
#define SRCH_BAD_OWNER ENC_BAD_TABLE                                              // flags: own[s] outside [0, B); the start's rows are zero
#define SRCH_UNUSABLE (ENC_EMPTY | ENC_NO_ROWS | ENC_BAD_TABLE | ALN_BAD_POSE)    // bits 0, 1, 3, 4: such a start is not ranked

// the shape start s draws its samples from, or -1: nothing is read through an entry outside [0, B)
ENC_HD int srch_owner(const int32_t* own, int s, int B) {
    const int o = own[s];
    return (o >= 0 && o < B) ? o : -1;
}

// The rows kernel's policy for a start: everything of the wrapped policy (indexed by the START: its pose, its side arrays), and owner(),
// through which the kernel finds the sample range and the draw's shape.  A start without an owner has a broken table as far as the kernel
// is concerned: zero rows and ENC_BAD_TABLE.
template <class Inner>
struct SrchRows {
    static constexpr int W = Inner::W;
    typedef typename Inner::Shape Shape;
    typedef typename Inner::Staged Staged;
    Inner inner;
    const int32_t* own;
    int B;
    ENC_HDM int owner(int s) const { return srch_owner(own, s, B); }
    ENC_HDM Shape shape(int s) const { return inner.shape(s); }
    ENC_HDM int32_t flags(const Shape& sh, bool bad, int64_t count) const { return inner.flags(sh, bad, count); }
    ENC_HDM Staged stage(const Shape& sh, const float* samples, int64_t src, int64_t i) const { return inner.stage(sh, samples, src, i); }
    ENC_HDM float xyz(const float* samples, const Staged& st, int a) const { return inner.xyz(samples, st, a); }
};

// AlnPosedRows for a scoring pass: the same shape, flags and rows (aln_row), but the camera-frame point is stored only where the caller
// wants it -- a loss without a gradient needs none.
struct SrchPosedRows : AlnPosedRows {
    ENC_HDM Staged stage(const Shape& s, const float* samples, int64_t src, int64_t i) const {
        float q[3] = {0.f, 0.f, 0.f}, l = 0.f, h = 0.f;
        Staged st = {{0.f, 0.f, 0.f}};
        if (src >= 0) {
            const float* row = samples + src * W;
            q[0] = row[0], q[1] = row[1], q[2] = row[2], l = row[3], h = row[4];
            aln_row(q, s.ps, s.ok, st.x, &l, &h);
        }
        if (cam) cam[3 * i] = q[0], cam[3 * i + 1] = q[1], cam[3 * i + 2] = q[2];
        lo[i] = l, hi[i] = h;
        return st;
    }
};

// The reduce's column rule without gradient columns (G = 0): column 0 the loss, column 1 the count of ok rows -- the last two columns of
// every other reduce, summed in the same order.
struct SrchLossCols {
    static constexpr int EXTRA = 0;
    ENC_HDM void prepare(double*, float, int64_t, int) const {}
    ENC_HDM double operator()(int c, int G, float, double e, int ok, int64_t, int, const double*) const { return c == G ? e : (ok ? 1.0 : 0.0); }
};

// starts of shape b, or -1 when the table is broken there or the shape has too many (N: starts of the call)
ENC_HD int64_t srch_count(const int64_t* coff, int b, int64_t N) {
    const int64_t a = coff[b], e = coff[b + 1];
    return (a < 0 || e < a || e > N || e - a > SRCH_MAX_STARTS) ? -1 : e - a;
}

// a start is ranked: none of the flags that keep a fit from stepping a shape, and a finite loss
ENC_HD bool srch_usable(int32_t flag, double loss) { return !(flag & SRCH_UNUSABLE) && isfinite(loss); }

// THE ORDER of two usable starts of a shape: (loss, index) ascending; equal losses (-0.0 == 0.0 too) go to the lower index
ENC_HD bool srch_before(double lj, int j, double li, int i) { return lj < li || (lj == li && j < i); }

// the rank of usable start i among the n starts of its shape: how many usable starts come before it
ENC_HD int srch_rank(const double* loss, const unsigned char* ok, int n, int i) {
    const double li = loss[i];
    int r = 0;
    for (int j = 0; j < n; ++j) r += (ok[j] && srch_before(loss[j], j, li, i)) ? 1 : 0;
    return r;
}
