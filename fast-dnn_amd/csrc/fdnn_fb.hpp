// fdnn_fb.hpp -- the HIP-free half of ALIGNMENT GRAPHS, SUMMED (fdnn_fb.hip): the likelihood of a whole graph, ln of the sum
// over its paths, and the state occupancies gamma[t][j], where fdnn_align_graph.hpp gives the best path.  The two stated
// functions, the recursion, the total's order, the transposer, the launch plan and a plain host restatement.  The arithmetic
// is stated here and nowhere else: the kernels call exp_neg(), ladd(), gamma_of() of this header, loglik::ln and
// align::emission of the siblings'.  tests/host/fb_check.cpp builds it alone, under the sanitizers.
//
// THE INPUTS are those of fdnn_align_graph.hpp, checked by align_graph::check unchanged: segments (LazyOutputActivations'
// caller, src/cpp/dnn.cc:355-392) of T >= 1 rows and 1 <= S <= 16 384 states, state j's incoming arcs arc_ptr[j] ..
// arc_ptr[j + 1] in the caller's order, arc_src local to the segment, arc_lp finite, start_lp / final_lp finite or -inf or
// null (state 0 / state S - 1), e(t, j) = align::emission(...): an F32 / F16 handle, or the rows are scores.
//
// fp32 throughout, every + and - rounded once, nothing contracted (-ffp-contract=off on host and device, no fast-math or
// flush-to-zero flag), selections by compare and select -- not fmaxf.
//
// TWO STATED FUNCTIONS
//   exp_neg(x): exp on (-inf, 0].  A NaN -> +0.0f; x < -87.0f -> +0.0f, so no result is a denormal (exp(-87) = 1.6e-38 is
//     above the smallest normal); x > 0 is taken as 0 (the result 1.0f): a caller with a positive argument decides itself
//     what it means, as gamma_of does.  Else ONE fixed sequence in the style of loglik::ln, the single-precision Cephes scheme:
//       n = round(x log2 e):  k = (x * 1.44269504f + 12582912.0f) - 12582912.0f, three operations each rounded once (adding
//           1.5 x 2^23 rounds to an integer, ties to even)
//       r = fmaf(-k, 0.693359375f, x);  r = fmaf(-k, -2.12194440e-4f, r)           |r| <= 0.35
//       p = a degree-5 Horner polynomial in fmaf for (e^r - 1 - r) / r^2;  y = fmaf(p, r * r, r) + 1.0f
//       2^n by adding n to y's exponent field (n >= -126 and y >= 1 there, so the field stays above 0)
//     FROZEN: results depend on every constant and on the order of the operations.
//   ladd(a, b) = ln(e^a + e^b):  hi = (b > a) ? b : a, lo = the other;  lo == -inf -> hi;  hi == +inf -> +inf;
//     else hi + loglik::ln(1.0f + exp_neg(lo - hi))        (loglik::ln is the frozen logarithm, included, not restated)
//     A NaN operand gives 0x7fc00000 (the recursion never adds one).  ladd is commutative in its bytes, ladd(-inf, x) has x's
//     bytes, and since ln(1) = +0 and ln is monotone (both swept), ladd(a, b) >= max(a, b) as floats.
//
// Measured over ALL floats of the domain against float64 (tools/exp_sweep.cpp, profiles/exp_sweep.log): exp_neg on every
// float of [-87, -0] against exp, and ln(1 + exp_neg(d)) on every d <= 0 against log1p(exp(d)).  kExpMaxUlp and kLse1MaxAbs
// are that run's worst values rounded up one step (0.05 ulp; 0.05 x 2^-24).
//
// THE RECURSION
//   alpha[0][j] = start_of(start_lp, j) + e(0, j)
//   t >= 1:       acc = -inf;  for a in arc_ptr[j] .. arc_ptr[j + 1], in that order:
//                   cand = alpha[t-1][arc_src[a]] + arc_lp[a];  if (cand == cand) acc = ladd(acc, cand)    (a NaN is never added)
//                 alpha[t][j] = acc + e(t, j)
//   total:        term_j = alpha[T-1][j] + final_of(final_lp, j, S), a NaN skipped;
//                 256 partial sums, state j dealt to partial j mod 256 and added there in ascending j (from -inf);
//                 then the tree  for step = 128, 64, .., 1:  partial[i] = ladd(partial[i], partial[i + step]), i < step;
//                 total = partial[0]
//   backward:     THE SAME recursion on the transposed graph, in reversed time, with final_lp for the start.  bb[t][i] is the
//                 backward score INCLUDING i's own emission: bb[T-1][i] = final_of(i) + e(T-1, i); for t < T - 1, bb[t][i] =
//                 (ladd over i's outgoing arcs, in ascending arc index, of bb[t+1][dst] + lp) + e(t, i).  The transposed
//                 tables are a stable counting sort by source, transpose() below: t_ptr [N + 1], t_src [arcs] (it holds
//                 the DESTINATION, local to the segment), t_lp [arcs].
//   gamma[t][j]:  x = ((alpha[t][j] + bb[t][j]) - e(t, j)) - total;  x > 0 -> 0;  gamma = exp_neg(x)      -- gamma_of()
//                 row-major [t][j] per segment; segment s begins at the sum of T S over the segments before it, a 64-bit offset.
//
// CONSEQUENCES
//   The total is never a NaN: acc begins at -inf, a NaN candidate is never added, and ladd of two non-NaNs is none (hi is
//     -inf, finite or +inf; ln(1 + exp_neg(.)) lies in [0, ln 2]); the terms of the total skip NaNs the same way.
//   -inf means no path.  A total that is not finite (-inf or +inf) gives gamma = +0.0f everywhere.  A NaN x gives +0.0f and
//     gamma <= 1.
//   gamma == null means forward only: no transposed tables are needed, there is no backward launch, no lattice scratch,
//     and four bytes per segment leave the device.
//   On any input total >= the best-path total of align_graph::ref (fdnn_debug_align_graph_ref), as floats: the additions
//     are rounded monotonically, so by induction alpha[t][j] >= d[t][j] wherever d is no NaN -- each sum candidate is >= the
//     matching best candidate, ladd >= max --, and the total's ladd tree is >= the maximum of its terms.
//   On a graph with exactly ONE path of finite score the two totals are equal as bits: every acc is ladd(-inf, cand) = cand,
//     the additions are the same chain, and the tree adds -inf to the one finite term.
//   The order of a state's arcs is part of the input: reversing it may change low bits.
//   Device-rows form: a source or destination outside [0, S) makes the candidate a NaN and reads nothing; a column or node
//     out of range makes the emission a NaN; every arc index is bounded from the HOST arc_ptr / t_ptr, as the sibling
//     bounds them.
//
// THE ACCURACY BOUND (what tests hold the restatement and the kernels to, against float64).  Log-sum-exp is 1-Lipschitz in
// the sup norm: an error of at most d in every alpha[t-1] moves the exact alpha[t] by at most d.  With A the largest
// in-degree (out-degree for bb), M the largest finite magnitude of an alpha, a bb, a candidate or a term of the total (at
// most the largest |alpha| or |bb| plus the largest |arc_lp| or finite |final_lp|) and u = 2^-24, one frame adds: the candidates' additions,
// each off by at most u M, which the sum passes on ONCE (they err side by side, not one after the other); the first ladd of a
// state is exact (ladd(-inf, x) = x) and each of the A - 1 others is off by at most
//   L = u M + kLse1MaxAbs + 0.37 u
// -- the rounding of its own addition, the swept error of ln(1 + exp_neg(d)) at the float d, and the rounding of d = lo - hi
// itself, which moves the exact value by at most |d| u e^-|d| <= u / e --; then the emission's addition, u M.  So a frame
// adds at most 2 u M + (A - 1) L = (A + 1) u M + (A - 1)(kLse1MaxAbs + 0.37 u).  The total adds final_lp (u M) and a chain
// of at most (S - 1) / 256 ladds in a partial and 8 in the tree:
//   |total - total64| <= delta = T (2 u M + (A - 1) L) + u M + (8 + (S - 1) / 256) L               -- delta_bound()
// alpha[t] carries t frames and bb[t] the other T - 1 - t (each after one first addition), so alpha[t][j] + bb[t][j] is
// within delta too.  gamma = exp(x) with |x - x64| <= 2 delta + 6 u M: that sum, the total, and three more roundings, each
// of a value of magnitude at most 2 M (alpha + bb and what is taken from it).  exp_neg is within kExpMaxUlp ulp of exp, so
// with gamma <= 1
//   |gamma - gamma64| <= exp(2 delta + 6 u M) (1 + kExpMaxUlp 2^-23) - 1 + 2^-126                -- gamma_bound()
// (2^-126: below -87 exp_neg gives +0 where exp gives up to 1.7e-38.)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fdnn_align_graph.hpp"

#if defined(__HIPCC__)
#define FDNN_FB_HD __host__ __device__ __forceinline__
#else
#define FDNN_FB_HD inline
#endif

namespace fdnn {
namespace fb {

using align::bits_of;
using align::finite_bits;
using align::float_of;
using align::kMinusInf;
using align::kQuietNaN;
using align::kScores;
using align_graph::final_of;
using align_graph::start_of;

// ---------------------------------------------------------------- the limits
using align::kMaxScratchBytes;  // the lattice of one call (T S fp32 words a segment, only when gamma is wanted): above it FDNN_E_ARG
using align::kMaxSegs;
using align::kMaxStates;
using align::kWaveLanes;
using align::kWgThreads;
using align_graph::kArcLdsArcs;   // the wave form stages a segment's arc table in LDS up to here
using align_graph::kEmissionRing;
using align_graph::kMaxArcs;
using align_graph::kRowValues;
using align_graph::kWaveStates;   // the wave form may be FORCED up to here: 4 states a lane
using align_graph::frames_in_flight;
using align_graph::wave_slots;
// The rule's threshold, MEASURED (tools/fb_sweep.py, profiles/fb_sweep.log), not copied: the chain per
// arc is a log-add of about forty dependent VALU operations, not a compare, yet the crossover is where the sibling's is.  At
// 1000 frames the wave form takes 0.79 x the workgroup form's time at 31 and 61 states (one state a lane; 0.83 with
// gamma), 1.35 x at 91 and 127 (two a lane), 1.85 x at 187 and 2.33 x at 253; 64 segments a launch give the same ratios.
constexpr int kWaveRuleStates = 64;
static_assert(kWaveRuleStates == kWaveLanes, "the rule takes the wave form while a lane owns one state");
constexpr int kPartials = 256;  // the total's partial sums

constexpr double kExpMaxUlp = 1.05;             // the exhaustive sweep's worst error of exp_neg, 1.0103 ulp (at 0xc0bc17a1), rounded up to 0.05
constexpr double kLse1MaxAbs = 1.50 / 16777216; // the sweep's worst |ln(1 + exp_neg(d)) - log1p(exp(d))|, d <= 0: 1.4821 x 2^-24 (at 0xbed5a860), rounded up to 0.05 x 2^-24

// ---------------------------------------------------------------- the two stated functions
FDNN_FB_HD float exp_neg(float x) {
  if (!(x >= -87.0f)) return 0.0f;  // a NaN, or below -87
  if (x > 0.0f) x = 0.0f;
  const float t = x * 1.44269504f;
  const float k = (t + 12582912.0f) - 12582912.0f;  // round(t), ties to even: an integer in [-126, 0]
  float r = fmaf(-k, 0.693359375f, x);
  r = fmaf(-k, -2.12194440e-4f, r);
  float p = 1.9875691500e-4f;
  p = fmaf(p, r, 1.3981999507e-3f);
  p = fmaf(p, r, 8.3334519073e-3f);
  p = fmaf(p, r, 4.1665795894e-2f);
  p = fmaf(p, r, 1.6666665459e-1f);
  p = fmaf(p, r, 5.0000001201e-1f);
  const float z = r * r;
  const float y = fmaf(p, z, r) + 1.0f;
  const int32_t n = static_cast<int32_t>(k);
  return float_of(bits_of(y) + (static_cast<uint32_t>(n) << 23));
}

FDNN_FB_HD float ladd(float a, float b) {
  if (a != a || b != b) return float_of(kQuietNaN);
  const bool sw = b > a;
  const float hi = sw ? b : a, lo = sw ? a : b;
  if (bits_of(lo) == kMinusInf) return hi;
  if (bits_of(hi) == 0x7f800000u) return hi;
  return hi + loglik::ln(1.0f + exp_neg(lo - hi));
}

// one candidate into a state's sum: d_src = d[t-1][src] (any NaN where src is outside [0, S))
FDNN_FB_HD float accumulate(float acc, float d_src, float lp) {
  const float cand = d_src + lp;
  return cand == cand ? ladd(acc, cand) : acc;
}

// one occupancy: alpha and bb of (t, j), both including e = e(t, j)
FDNN_FB_HD float gamma_of(float alpha, float bb, float e, float total) {
  if (!finite_bits(bits_of(total))) return 0.0f;
  float x = ((alpha + bb) - e) - total;
  if (x > 0.0f) x = 0.0f;
  return exp_neg(x);
}

// the total from the 256 partial sums, in place
inline float total_tree(float *partial) {
  for (int step = kPartials / 2; step >= 1; step /= 2)
    for (int i = 0; i < step; ++i) partial[i] = ladd(partial[i], partial[i + step]);
  return partial[0];
}

// the total of a last row (alpha[T-1][.]): the contract's order
inline float total_of(const float *last, const float *final_lp, int S) {
  float partial[kPartials];
  for (int i = 0; i < kPartials; ++i) partial[i] = float_of(kMinusInf);
  for (int j = 0; j < S; ++j) {
    const float term = last[j] + final_of(final_lp, j, S);
    if (term == term) partial[j % kPartials] = ladd(partial[j % kPartials], term);
  }
  return total_tree(partial);
}

// ---------------------------------------------------------------- the transposer
// A stable counting sort of every segment's arcs by source: t_ptr [N + 1] (global, as arc_ptr: a segment's transposed arcs
// occupy the range of its arcs), t_src [arcs] = the DESTINATION of the arc, local to the segment, t_lp [arcs].  State i's
// outgoing arcs come in ascending arc index.  0, or -(s + 1) of the first segment with a source outside [0, S) or a
// decreasing arc_ptr (nothing of that segment or a later one is then defined).
inline int transpose(const int32_t *state_ptr, int n_segs, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, int32_t *t_ptr,
                     int32_t *t_src, float *t_lp) {
  if (n_segs <= 0) return 0;
  t_ptr[0] = 0;
  std::vector<int32_t> cursor;
  for (int s = 0; s < n_segs; ++s) {
    const int32_t b = state_ptr[s], S = state_ptr[s + 1] - b;
    const int32_t a0 = arc_ptr[b], a1 = arc_ptr[b + S];
    if (S < 0 || a1 < a0) return -(s + 1);
    cursor.assign(static_cast<size_t>(S) + 1, 0);
    for (int32_t j = 0; j < S; ++j) {
      if (arc_ptr[b + j + 1] < arc_ptr[b + j] || arc_ptr[b + j] < a0 || arc_ptr[b + j + 1] > a1) return -(s + 1);
      for (int32_t a = arc_ptr[b + j]; a < arc_ptr[b + j + 1]; ++a) {
        if (arc_src[a] < 0 || arc_src[a] >= S) return -(s + 1);
        ++cursor[static_cast<size_t>(arc_src[a]) + 1];
      }
    }
    for (int32_t i = 0; i < S; ++i) cursor[static_cast<size_t>(i) + 1] += cursor[static_cast<size_t>(i)];
    for (int32_t i = 0; i < S; ++i) t_ptr[b + i + 1] = a0 + cursor[static_cast<size_t>(i) + 1];
    for (int32_t j = 0; j < S; ++j)
      for (int32_t a = arc_ptr[b + j]; a < arc_ptr[b + j + 1]; ++a) {
        const int32_t at = a0 + cursor[static_cast<size_t>(arc_src[a])]++;
        t_src[at] = j, t_lp[at] = arc_lp[a];
      }
  }
  return 0;
}

// ---------------------------------------------------------------- the host restatement, over bit patterns
// One segment; rows, col, node, log_prior, type, arc_ptr [S + 1] (the segment's entries of the call's table), arc_src, arc_lp,
// start_lp, final_lp as align_graph::ref.  -> *total (bits) and, where gamma is not null, gamma [T S] (bits) from t_ptr
// [S + 1] (the segment's entries), t_src, t_lp (the call's arrays).  A source or destination outside [0, S) gives a NaN
// candidate and reads nothing.
inline void ref(const uint32_t *rows, int T, long long ld, const int32_t *col, const int32_t *node, int S, const float *log_prior, int width,
                float floor, int type, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp,
                const float *final_lp, const int32_t *t_ptr, const int32_t *t_src, const float *t_lp, uint32_t *total, uint32_t *gamma) {
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);
  const size_t Ss = static_cast<size_t>(S), Ts = static_cast<size_t>(T);
  auto e = [&](int t, int j) {
    const bool ok = col[j] >= 0 && col[j] < ld && (type == kScores || (node[j] >= 0 && node[j] < width));
    const float v = ok ? float_of(rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(col[j])]) : nan;
    return align::emission(v, ok && type != kScores ? log_prior[node[j]] : 0.0f, floor, type);
  };
  // one direction: lat [T][S], row `frame`
  auto sweep = [&](bool backward, const int32_t *ptr, const int32_t *src, const float *lp, std::vector<float> *lat) {
    lat->assign(Ts * Ss, ninf);
    for (int u = 0; u < T; ++u) {
      const int t = backward ? T - 1 - u : u;
      float *d = lat->data() + static_cast<size_t>(t) * Ss;
      const float *prev = u ? lat->data() + static_cast<size_t>(backward ? t + 1 : t - 1) * Ss : nullptr;
      for (int j = 0; j < S; ++j) {
        float acc;
        if (!u) {
          acc = backward ? final_of(final_lp, j, S) : start_of(start_lp, j);
        } else {
          acc = ninf;
          for (int32_t a = ptr[j]; a < ptr[j + 1]; ++a) acc = accumulate(acc, src[a] >= 0 && src[a] < S ? prev[src[a]] : nan, lp[a]);
        }
        d[j] = acc + e(t, j);
      }
    }
  };
  std::vector<float> alpha, bb;
  sweep(false, arc_ptr, arc_src, arc_lp, &alpha);
  const float tot = total_of(alpha.data() + (Ts - 1) * Ss, final_lp, S);
  *total = bits_of(tot);
  if (!gamma) return;
  sweep(true, t_ptr, t_src, t_lp, &bb);
  for (int t = 0; t < T; ++t)
    for (int j = 0; j < S; ++j) {
      const size_t at = static_cast<size_t>(t) * Ss + static_cast<size_t>(j);
      gamma[at] = bits_of(gamma_of(alpha[at], bb[at], e(t, j), tot));
    }
}

// ---------------------------------------------------------------- the accuracy bound (see the top)
inline double delta_bound(int T, int S, int max_degree, double max_abs) {
  const double u = 1.0 / 16777216, L = u * max_abs + kLse1MaxAbs + 0.37 * u;
  return T * (2 * u * max_abs + std::max(max_degree - 1, 0) * L) + u * max_abs + (8 + (S - 1) / 256) * L;
}
inline double gamma_bound(double delta, double max_abs) {
  const double u = 1.0 / 16777216;
  return std::exp(2 * delta + 6 * u * max_abs) * (1.0 + kExpMaxUlp * 2 * u) - 1.0 + 1.2e-38;
}

// ---------------------------------------------------------------- the launch plan
// The sibling's two forms (fdnn_align_graph.hpp), each run forward and, where gamma is wanted, backward over the transposed
// tables -- one kernel body with a direction.  Wave form (S <= kWaveRuleStates by the rule, <= kWaveStates forced): one wave
// per segment, lane l owns states l, l + 64, ..; d as two rows in LDS, a ring of emissions, the arc offsets and -- where
// the segment has at most kArcLdsArcs arcs -- the arc table staged in LDS; no workgroup barrier.  Workgroup form (any S):
// 256 threads, thread i owns states i, i + 256, ..; one barrier per frame.  The lattice: the forward sweep with gamma wanted
// writes alpha[t][.] to the call's scratch, T S fp32 words a segment at the segment's gamma offset; the backward sweep reads
// it and the total and writes gamma[t][.] as it goes.
enum Form { kWave = 0, kWorkgroup = 1 };

// mode (fdnn_debug_set_fb_kernel): 0 the rule, 1 wave where allowed (up to kWaveStates), 2 always workgroup
inline Form form_for(int S, int mode) { return (mode == 1 ? S <= kWaveStates : (mode == 0 && S <= kWaveRuleStates)) ? kWave : kWorkgroup; }
inline bool arcs_staged(Form f, int n_arcs) { return f == kWave && n_arcs <= kArcLdsArcs; }

// One launch's segments, a kernel argument passed by value (2.8 KB).  Workgroup s of the launch is segment s of this table.
struct Launch {
  int form, n_segs, lds_bytes;
  int K;         // wave form: states per lane, 1, 2 or 4
  int d_floats;  // floats of ONE row of d in LDS: the launch's largest graph, rounded up to 64 (wave form: 64 K)
  int arc_cap;   // wave form: the most arcs a segment of the launch stages (even; 0: none does)
  int T[kMaxSegs], ld[kMaxSegs], state0[kMaxSegs], S[kMaxSegs], total_off[kMaxSegs];
  int arc0[kMaxSegs], n_arcs[kMaxSegs];  // the segment's arcs in the call's arrays, FROM THE HOST TABLE: what bounds every arc index, either direction
  long long row_off[kMaxSegs];           // the segment's first row, in elements from the rows' base
  long long out_off[kMaxSegs];           // the segment's gamma, and its lattice in the scratch: the sum of T S before it
};

// the wave form's LDS, in 32-bit words: two rows of d, the rings of emissions and (backward) of alphas, the arc offsets [S + 1],
// the staged scores and sources: 36 KiB at the most
inline int wave_lds_words(int d_floats, int arc_cap) { return 2 * d_floats + 2 * kEmissionRing + (d_floats + 64) + arc_cap + arc_cap / 2; }
inline int wg_lds_words(int d_floats) { return 2 * d_floats + kPartials; }

struct Plan {
  std::vector<Launch> launches;  // each is launched forward and, with gamma, backward
  long long gamma_words = 0;     // the sum of T S over the call
  long long scratch_words = 0;   // the lattice: gamma_words where gamma is wanted, else 0
};

// seg_T, row_off, row_ld [n_segs], state_ptr [n_segs + 1], arc_ptr [state_ptr[n_segs] + 1] or null (no arcs: the scratch
// size does not depend on them).  Every kMaxSegs consecutive segments give one launch per form that occurs among them.
inline Plan plan(const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr, const int32_t *arc_ptr, int n_segs,
                 bool want_gamma, int mode) {
  Plan p;
  std::vector<long long> out_off(static_cast<size_t>(std::max(n_segs, 0)));
  for (int s = 0; s < n_segs; ++s) {
    out_off[static_cast<size_t>(s)] = p.gamma_words;
    p.gamma_words += static_cast<long long>(seg_T[s]) * (state_ptr[s + 1] - state_ptr[s]);
  }
  p.scratch_words = want_gamma ? p.gamma_words : 0;
  for (int s0 = 0; s0 < n_segs; s0 += kMaxSegs) {
    const int s1 = std::min(n_segs, s0 + kMaxSegs);
    for (int f = kWave; f <= kWorkgroup; ++f) {
      Launch l{};
      l.form = f;
      int max_s = 0;
      for (int s = s0; s < s1; ++s) {
        const int S = state_ptr[s + 1] - state_ptr[s];
        if (form_for(S, mode) != f) continue;
        const int i = l.n_segs++;
        max_s = std::max(max_s, S);
        l.T[i] = seg_T[s], l.ld[i] = row_ld[s], l.state0[i] = state_ptr[s], l.S[i] = S, l.total_off[i] = s;
        l.row_off[i] = row_off[s], l.out_off[i] = out_off[static_cast<size_t>(s)];
        l.arc0[i] = arc_ptr ? arc_ptr[state_ptr[s]] : 0;
        l.n_arcs[i] = arc_ptr ? arc_ptr[state_ptr[s + 1]] - arc_ptr[state_ptr[s]] : 0;
        if (arcs_staged(static_cast<Form>(f), l.n_arcs[i])) l.arc_cap = std::max(l.arc_cap, (l.n_arcs[i] + 1) / 2 * 2);
      }
      if (!l.n_segs) continue;
      l.K = f == kWave ? wave_slots(max_s) : 1;
      l.d_floats = f == kWave ? l.K * kWaveLanes : (max_s + 63) / 64 * 64;
      l.lds_bytes = 4 * (f == kWave ? wave_lds_words(l.d_floats, l.arc_cap) : wg_lds_words(l.d_floats));
      p.launches.push_back(l);
    }
  }
  return p;
}

}  // namespace fb
}  // namespace fdnn
