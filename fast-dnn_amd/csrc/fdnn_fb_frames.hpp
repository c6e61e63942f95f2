// fdnn_fb_frames.hpp -- the HIP-free half of the FRAMES FORM of alignment graphs, summed (fdnn_fb_frames.hip): the graph's
// likelihood at EVERY frame, a start that may be free, and a row carried from one call to the next.  Forward only.  No
// arithmetic of its own: accumulate, ladd, total_of of fdnn_fb.hpp, start_of / final_of of fdnn_align_graph.hpp and
// align::emission are called, not restated.  tests/host/fb_frames_check.cpp builds it alone, under the sanitizers.
//
// THE INPUTS are fdnn_fb.hpp's, checked by align_graph::check unchanged, and beside them
//   free_start  0 or 1, per call.  1: a path may begin at any frame.
//   alpha_in    null, or one fp32 per state of the call, laid out like `states`: the recursion's row from the frame before
//               this call's first row.
//   alpha_out   null, or the same shape: the last row's alpha, for the next call.
//   frame_total one fp32 per row of the call; segment s begins at the sum of T over the segments before it, a 64-bit offset.
//
// THE CONTRACT
//   frame 0 without alpha_in:   alpha[0][j] = start_of(start_lp, j) + e(0, j)                          -- as fdnn_fb.hpp
//   every other frame, and frame 0 with alpha_in:
//       prev = alpha_in for frame 0 with alpha_in, alpha's row before otherwise
//       acc = -inf;  for a in arc_ptr[j] .. arc_ptr[j + 1], in that order:  acc = accumulate(acc, prev[arc_src[a]], arc_lp[a])
//       if free_start:  acc = ladd(acc, start_of(start_lp, j))       -- the start term LAST; ladd(x, -inf) has x's bytes, so
//                                                                       it is unconditional
//       alpha[t][j] = acc + e(t, j)
//     A NaN in alpha_in makes a NaN candidate, which accumulate never adds.
//   frame_total[t] = total_of(alpha[t][.], final_lp, S): the existing order -- 256 partials, state j in partial j mod 256 in
//     ascending j, then the tree.
//   alpha_out = alpha[T-1][.], as bits.  Where that alpha is a NaN it is SOME NaN: payload and sign are not part of the
//     contract (the host's and the device's inf - inf need not share a sign bit); frame_total is never one, so its bits are.
//   alpha_out may be the very buffer alpha_in points to: every sweep loads its segment's carry row into d before it stores
//     anything, stores alpha_out last, and touches no other segment's states.  A partial overlap is not allowed.
//
// CONSEQUENCES (each is tested)
//   (a) free_start = 0 and no alpha_in: rows 0 .. t are fb::ref's recursion on the segment cut to t + 1 rows -- row t depends
//       on the rows before it alone --, and the total is the same function of row t.  So frame_total[t] has the bytes of
//       fb::ref's total on that prefix, and frame_total[T-1] those of fdnn_calculate_fb's total.
//   (b) A segment cut at ANY frame c into two calls, the second taking the first's alpha_out as alpha_in: the second call's
//       frame 0 takes the ordinary step from prev = alpha[c-1][.], bit for bit the row the uncut call steps from, and every
//       later row follows by induction; totals and alpha_out are functions of rows.  So the two calls give the uncut call's
//       frame_total and alpha_out byte for byte, with either value of free_start.
//   (c) frame_total is never a NaN: acc begins at -inf, accumulate adds no NaN, ladd of two non-NaNs is none (start_of is finite
//       or -inf by the validator), and total_of skips NaN terms -- whatever the emissions or alpha_in hold.
//   (d) Where no emission and no alpha_in value is +inf, no alpha is +inf, so an alpha is a NaN exactly where e(t, j) is one,
//       with either value of free_start.  Every other alpha[t][j] with free_start = 1 is >= the anchored one, as floats:
//       candidates are rounded sums of values that are >= (additions round monotonically), ladd(x, s) >= x (fdnn_fb.hpp), and
//       ladd is monotone in either operand -- its logarithm is swept monotone; for exp_neg and the final addition this is
//       observed on every case of the tests, not proven.  The total's terms and tree are monotone the same way:
//       frame_total[t] (free) >= frame_total[t] (anchored).
//   (e) Against float64, |frame_total[t] - total64[t]| <= fb::delta_bound(t + 1, S, A + free_start, M): the start term is one
//       more log-add per state and frame, which is what one more arc costs in fdnn_fb.hpp's derivation; M also covers the
//       finite start_lp values.  With t counted from the STREAM's first frame the bound holds under carry, by (b).
#pragma once
#include "fdnn_fb.hpp"

namespace fdnn {
namespace fb_frames {

using align::bits_of;
using align::float_of;
using align::kMinusInf;
using align::kQuietNaN;
using align::kScores;
using align_graph::final_of;
using align_graph::start_of;
using fb::kMaxScratchBytes;  // the lattice of one call, T S fp32 words a segment: always needed here; above it FDNN_E_ARG
using fb::kMaxSegs;
using fb::kPartials;
using fb::kWaveLanes;

constexpr int kRowsPerGroup = 4;  // the row-total kernel: one wave per lattice row, four rows a workgroup

// one state of one frame after the first (or of the first, with alpha_in): prev is the row before, arcs local to the segment
inline float step(const float *prev, int S, const int32_t *arc_src, const float *arc_lp, int32_t a0, int32_t a1, const float *start_lp, int j,
                  bool free_start) {
  float acc = float_of(kMinusInf);
  for (int32_t a = a0; a < a1; ++a) acc = fb::accumulate(acc, arc_src[a] >= 0 && arc_src[a] < S ? prev[arc_src[a]] : float_of(kQuietNaN), arc_lp[a]);
  if (free_start) acc = fb::ladd(acc, start_of(start_lp, j));
  return acc;
}

// ---------------------------------------------------------------- the host restatement, over bit patterns
// One segment; rows .. final_lp as fb::ref.  alpha_in / alpha_out [S] or null (bits), frame_total [T] (bits).
inline void ref(const uint32_t *rows, int T, long long ld, const int32_t *col, const int32_t *node, int S, const float *log_prior, int width,
                float floor, int type, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp,
                const float *final_lp, bool free_start, const uint32_t *alpha_in, uint32_t *alpha_out, uint32_t *frame_total) {
  const float nan = float_of(kQuietNaN);
  const size_t Ss = static_cast<size_t>(S);
  auto e = [&](int t, int j) {
    const bool ok = col[j] >= 0 && col[j] < ld && (type == kScores || (node[j] >= 0 && node[j] < width));
    const float v = ok ? float_of(rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(col[j])]) : nan;
    return align::emission(v, ok && type != kScores ? log_prior[node[j]] : 0.0f, floor, type);
  };
  std::vector<float> prev(Ss), cur(Ss);
  if (alpha_in)
    for (int j = 0; j < S; ++j) prev[static_cast<size_t>(j)] = float_of(alpha_in[j]);
  for (int t = 0; t < T; ++t) {
    for (int j = 0; j < S; ++j) {
      const float acc = (t == 0 && !alpha_in) ? start_of(start_lp, j)
                                              : step(prev.data(), S, arc_src, arc_lp, arc_ptr[j], arc_ptr[j + 1], start_lp, j, free_start);
      cur[static_cast<size_t>(j)] = acc + e(t, j);
    }
    frame_total[t] = bits_of(fb::total_of(cur.data(), final_lp, S));
    prev.swap(cur);
  }
  if (alpha_out)
    for (int j = 0; j < S; ++j) alpha_out[j] = bits_of(prev[static_cast<size_t>(j)]);
}

// ---------------------------------------------------------------- the launch plan
// fb::Plan's launches for the forward sweep (the same two forms under fb::form_for and the same forcing), the lattice always
// wanted, and behind each of them ONE row-total launch over the rows that sweep launch left in the lattice: a grid of
// (ceil(the launch's longest T / kRowsPerGroup), its segments) workgroups of kRowsPerGroup waves, from the host tables.
struct RowLaunch {
  int n_segs, max_T;
  int T[kMaxSegs], S[kMaxSegs], state0[kMaxSegs];
  long long lat_off[kMaxSegs];    // the segment's lattice in the scratch: the sum of T S before it
  long long frame_off[kMaxSegs];  // the segment's frame_total: the sum of T before it
};

// the sweep's wave form needs no ring of alphas: two rows of d, the emissions, the arc offsets, the staged arcs
inline int wave_lds_words(int d_floats, int arc_cap) { return 2 * d_floats + fb::kEmissionRing + (d_floats + 64) + arc_cap + arc_cap / 2; }

struct Plan {
  fb::Plan sweep;               // launches[i] is followed by rows[i]
  std::vector<RowLaunch> rows;
  long long scratch_words = 0;  // the lattice: the sum of T S over the call
  long long total_rows = 0;     // the sum of T: frame_total's length
};

inline Plan plan(const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr, const int32_t *arc_ptr, int n_segs,
                 int mode) {
  Plan p;
  p.sweep = fb::plan(seg_T, row_off, row_ld, state_ptr, arc_ptr, n_segs, true, mode);
  p.scratch_words = p.sweep.scratch_words;
  std::vector<long long> frame_off(static_cast<size_t>(std::max(n_segs, 0)));
  for (int s = 0; s < n_segs; ++s) frame_off[static_cast<size_t>(s)] = p.total_rows, p.total_rows += seg_T[s];
  for (fb::Launch &l : p.sweep.launches) {
    if (l.form == fb::kWave) l.lds_bytes = 4 * wave_lds_words(l.d_floats, l.arc_cap);
    else l.lds_bytes = 4 * 2 * l.d_floats;  // the workgroup form: two rows of d, no reduction
    RowLaunch r{};
    r.n_segs = l.n_segs;
    for (int i = 0; i < l.n_segs; ++i) {
      r.T[i] = l.T[i], r.S[i] = l.S[i], r.state0[i] = l.state0[i], r.lat_off[i] = l.out_off[i];
      r.frame_off[i] = frame_off[static_cast<size_t>(l.total_off[i])];  // (total_off is the segment's index in the call)
      r.max_T = std::max(r.max_T, l.T[i]);
    }
    p.rows.push_back(r);
  }
  return p;
}

}  // namespace fb_frames
}  // namespace fdnn
