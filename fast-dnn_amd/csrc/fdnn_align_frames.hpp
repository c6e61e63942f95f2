// fdnn_align_frames.hpp -- the HIP-free half of the FRAMES FORM of alignment graphs, best path (fdnn_align_frames.hip): the best
// path's score at EVERY frame, the state it ends in and THE FRAME IT BEGAN AT, with a start that may be free and a row carried
// from one call to the next.  No arithmetic of its own beyond the begin bookkeeping: relax, better_end, start_of, final_of of
// fdnn_align_graph.hpp, align::emission and align::total_bits are called, not restated.  tests/host/align_frames_check.cpp
// builds it alone, under the sanitizers.
//
// A sum over paths (fdnn_fb_frames.hpp) has no begin frame; the best path has one, and it costs nothing to track: a token
// carries the frame at which its path started along the recursion (token passing), so the begin frame of the best path ending
// at frame t is known at frame t without back-pointers, a lattice or a back-trace.
//
// THE INPUTS are fdnn_align_graph.hpp's, checked by align_graph::check unchanged (S <= kMaxStates below), and beside them
//   free_start  0 or 1, per call.  1: a path may begin at any frame.
//   frame_base  int32 per segment, or null for zeros: the caller's number for the segment's first row in this call.  Begin
//               frames are reported in that numbering (frame_base + t, two's complement).
//   d_in, begin_in    both null or both given: one fp32 and one int32 per state of the call, laid out like `states`: the
//               recursion's row from the frame before this call's first row.  begin_in values are opaque and pass through.
//   d_out, begin_out  null, or the same shape: the last row, for the next call.  Each may be the very buffer of its _in twin
//               (a sweep loads its segment's carry row before it stores anything, stores the out row last and touches no
//               other segment's states); a partial overlap is not allowed.
//   frame_best fp32, frame_end int32, frame_begin int32: one each per row of the call; segment s begins at the sum of T over
//               the segments before it.
//
// THE CONTRACT (fp32, every + rounded once, nothing contracted, compare and select -- not fmaxf)
//   frame 0 without carry:   d[0][j] = start_of(start_lp, j) + e(0, j);   b[0][j] = start_of(start_lp, j) > -inf ? frame_base : -1
//   every other frame, and frame 0 with carry (prev = the row before, or d_in / begin_in):
//       best = -inf; from = -1;  for a in arc_ptr[j] .. arc_ptr[j + 1], in that order: relax(prev_d[arc_src[a]], arc_lp[a], ..)
//                                 -- a source outside [0, S) is a NaN candidate and reads nothing
//       bg = from >= 0 ? prev_b[from] : -1
//       if free_start:  s = start_of(start_lp, j);  if (s > best) best = s, bg = frame_base + t
//                                 -- the start term LAST; a tie keeps the path that is already running
//       d[t][j] = best + e(t, j);  b[t][j] = bg                                                          -- step()
//   per frame:  (best, end) = better_end over j ascending of d[t][j] + final_of(final_lp, j, S), from (-inf, -1)
//       frame_best[t] = total_bits(best);  frame_end[t] = end;  frame_begin[t] = end >= 0 ? b[t][end] : -1   -- select()
//   d_out = d[T-1][.] as bits; where it is a NaN it is SOME NaN (payload and sign are not part of the contract: the host's and
//     the device's inf - inf need not share a sign bit, as in fdnn_fb_frames.hpp).  begin_out = b[T-1][.]
//
// CONSEQUENCES (each is tested)
//   (a) free_start = 0 and no carry: rows 0 .. t of d are align_graph::ref's on the segment cut to t + 1 rows (row t depends
//       on the rows before it alone) and select() is its final selection, so frame_best[t] has the bytes of that total.  Every
//       b that is not -1 is frame_base: b[0] is, and a later bg copies a source's.  Where the total is finite, the end is
//       ref's `end` = path[t], and d[t][end] is finite, so a candidate was taken at every frame back to a start state:
//       frame_begin[t] = frame_base.
//   (b) A segment cut at ANY frame c into two calls, the second taking the first's d_out / begin_out and frame_base + c: its
//       frame 0 takes the ordinary step from the very row the uncut call steps from (a NaN's payload does not matter: a NaN
//       candidate is never taken), frame_base + c + t' = frame_base + t, and later rows follow by induction.  So the two
//       calls give the uncut call's three per-frame arrays and begin_out byte for byte, and d_out under the NaN rule.
//   (c) frame_best is never a NaN: better_end takes no NaN, whatever the rows or d_in hold.
//   (d) With free_start = 1, frame_best[t] >= the anchored value, as floats.  PROOF, not observation: a rounded addition is
//       monotone in either operand, and compare-and-select returns the maximum of its non-NaN candidates, which is monotone in
//       each; the free recursion has every anchored candidate (by induction >= the anchored one, or the anchored one is a
//       NaN and then was never taken) and the start term besides.  A d that is a NaN in one run is a NaN in the other unless
//       the free run's operand became +inf, which only raises what follows or makes a NaN that neither run takes.
//   (e) THE BEGIN FRAME IS TRUE.  free_start = 1, frame_best[t] finite, b = frame_begin[t] - frame_base inside the stream's
//       rows: align_graph::ref, anchored, on rows b .. t gives frame_best[t]'s bytes as its total, and its path[t - b] is
//       frame_end[t].  The winning path is a concrete anchored path from b whose score was added up in the same order, so
//       ref's total is >= it; every anchored path from b is a candidate of the free recursion, so it is <= it; at equal
//       scores both selections keep the lowest end.
//   (f) Against float64: a path's score takes 2 (t + 1) additions (the start term, an arc and an emission per later frame, the
//       emission of frame 0 and the final term), each off by at most u M, u = 2^-24, M the largest magnitude the recursion
//       meets; the maximum over candidates moves by no more than its operands do.  By induction over the frames
//         |frame_best[t] - best64[t]| <= 2 (t + 1) u M                                                      -- best_bound()
//       with t counted from the STREAM's first frame under carry, by (b); the free start term is exact.
//
// THE PATH ITSELF (a back-trace across calls) is out of scope: once (e) has given the span, fdnn_calculate_align_graph on rows
// b .. t returns it.
#pragma once
#include "fdnn_align_graph.hpp"

namespace fdnn {
namespace align_frames {

using align::bits_of;
using align::float_of;
using align::kMinusInf;
using align::kQuietNaN;
using align::kScores;
using align_graph::better_end;
using align_graph::final_of;
using align_graph::kArcLdsArcs;
using align_graph::kEmissionRing;
using align_graph::kMaxSegs;
using align_graph::kWaveLanes;
using align_graph::kWgThreads;
using align_graph::relax;
using align_graph::start_of;

// d and b as two rows each in LDS, whatever the form: four 32-bit rows of the largest graph inside the 160 KiB a workgroup
// can have.  Above it FDNN_E_ARG (the best-path sibling, which keeps no b, goes to align::kMaxStates)
constexpr int kMaxStates = 8192;
constexpr int kWgSlotWords = 2 * 3 * (kWgThreads / kWaveLanes);  // the workgroup form: (best, end, begin) per wave, by frame parity

// the caller's number of the call's frame t
FDNN_ALIGN_HD int32_t frame_no(int32_t frame_base, int t) { return static_cast<int32_t>(static_cast<uint32_t>(frame_base) + static_cast<uint32_t>(t)); }

// the start row: frame 0 without carry
FDNN_ALIGN_HD int32_t start_begin(float start, int32_t frame_base) { return start > float_of(kMinusInf) ? frame_base : -1; }

// what follows a state's arcs (best, from the result of relax over them, prev_b_from = prev_b[from], read only where
// from >= 0): the begin of the candidate taken, then the start term, last
FDNN_ALIGN_HD void after_arcs(int from, int32_t prev_b_from, bool free_start, float start, int32_t now, float *best, int32_t *bg) {
  *bg = from >= 0 ? prev_b_from : -1;
  if (free_start && start > *best) *best = start, *bg = now;
}

// one state into a frame's selection: better_end on (value, index), the begin riding along (an index is taken at most once,
// so `end` changes exactly where the candidate is taken).  Order-free like better_end
FDNN_ALIGN_HD void fold(float cand, int idx, int32_t begin, float *best, int *end, int32_t *bg) {
  const int before = *end;
  better_end(cand, idx, best, end);
  if (*end != before) *bg = begin;
}

// one state of one frame after the first (or of the first, with carry); arcs local to the segment
inline void step(const float *prev_d, const int32_t *prev_b, int S, const int32_t *arc_src, const float *arc_lp, int32_t a0, int32_t a1, float start,
                 bool free_start, int32_t now, float *best, int32_t *bg) {
  *best = float_of(kMinusInf);
  int from = -1;
  for (int32_t a = a0; a < a1; ++a) {
    const int src = arc_src[a];
    relax(src >= 0 && src < S ? prev_d[src] : float_of(kQuietNaN), arc_lp[a], src, best, &from);
  }
  after_arcs(from, from >= 0 ? prev_b[from] : -1, free_start, start, now, best, bg);
}

// a frame's selection over a row
inline void select(const float *d, const int32_t *b, const float *final_lp, int S, uint32_t *best_bits, int32_t *end_out, int32_t *begin_out) {
  float best = float_of(kMinusInf);
  int end = -1;
  int32_t bg = -1;
  for (int j = 0; j < S; ++j) fold(d[j] + final_of(final_lp, j, S), j, b[j], &best, &end, &bg);
  *best_bits = align::total_bits(best), *end_out = end, *begin_out = end >= 0 ? bg : -1;
}

// ---------------------------------------------------------------- the host restatement, over bit patterns
// One segment; rows .. final_lp as align_graph::ref.  d_in / begin_in / d_out / begin_out [S] or null; the results [T].
inline void ref(const uint32_t *rows, int T, long long ld, const int32_t *col, const int32_t *node, int S, const float *log_prior, int width,
                float floor, int type, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp,
                const float *final_lp, bool free_start, int32_t frame_base, const uint32_t *d_in, const int32_t *begin_in, uint32_t *d_out,
                int32_t *begin_out, uint32_t *frame_best, int32_t *frame_end, int32_t *frame_begin) {
  const float nan = float_of(kQuietNaN);
  const size_t Ss = static_cast<size_t>(S);
  auto e = [&](int t, int j) {
    const bool ok = col[j] >= 0 && col[j] < ld && (type == kScores || (node[j] >= 0 && node[j] < width));
    const float v = ok ? float_of(rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(col[j])]) : nan;
    return align::emission(v, ok && type != kScores ? log_prior[node[j]] : 0.0f, floor, type);
  };
  std::vector<float> d(Ss), nd(Ss);
  std::vector<int32_t> b(Ss), nb(Ss);
  if (d_in)
    for (size_t j = 0; j < Ss; ++j) d[j] = float_of(d_in[j]), b[j] = begin_in[j];
  for (int t = 0; t < T; ++t) {
    for (int j = 0; j < S; ++j) {
      const size_t js = static_cast<size_t>(j);
      const float start = start_of(start_lp, j);
      float best;
      if (t == 0 && !d_in) best = start, nb[js] = start_begin(start, frame_base);
      else step(d.data(), b.data(), S, arc_src, arc_lp, arc_ptr[j], arc_ptr[j + 1], start, free_start, frame_no(frame_base, t), &best, &nb[js]);
      nd[js] = best + e(t, j);
    }
    d.swap(nd), b.swap(nb);
    select(d.data(), b.data(), final_lp, S, frame_best + t, frame_end + t, frame_begin + t);
  }
  if (d_out)
    for (size_t j = 0; j < Ss; ++j) d_out[j] = bits_of(d[j]);
  if (begin_out)
    for (size_t j = 0; j < Ss; ++j) begin_out[j] = b[j];
}

// ---------------------------------------------------------------- the accuracy bound (consequence (f))
// frames = t + 1 counted from the stream's first frame; max_abs the largest magnitude of any finite value of the recursion
inline double best_bound(int frames, double max_abs) { return 2.0 * frames * max_abs / 16777216; }

// ---------------------------------------------------------------- the launch plan
// The sibling's launches (align_graph::plan: the same two forms under form_for and the same forcing, up to kMaxSegs segments
// a launch per form, arc counts from the host table), ONE launch per form and no scratch: path_off is the segment's first
// frame in the results, total_off its index in the call; the back-pointer fields are not used.
// Wave form LDS: d and b as two rows each, the ring of emissions, the arc offsets, the staged arcs.  Workgroup form: the four
// rows and the waves' triples by frame parity.
inline int wave_lds_words(int d_floats, int arc_cap) { return 4 * d_floats + kEmissionRing + (d_floats + 64) + arc_cap + arc_cap / 2; }
inline int wg_lds_words(int d_floats) { return 4 * d_floats + kWgSlotWords; }

inline align_graph::Plan plan(const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr, const int32_t *arc_ptr,
                              int n_segs, int mode) {
  align_graph::Plan p = align_graph::plan(seg_T, row_off, row_ld, state_ptr, arc_ptr, n_segs, mode);
  p.scratch_words = 0;
  for (align_graph::Launch &l : p.launches) {
    l.bp_words = 0;
    l.lds_bytes = 4 * (l.form == align_graph::kWave ? wave_lds_words(l.d_floats, l.arc_cap) : wg_lds_words(l.d_floats));
  }
  return p;
}

// the first segment with more than kMaxStates states, or -1
inline int too_many_states(const int32_t *state_ptr, int n_segs) {
  for (int s = 0; s < n_segs; ++s)
    if (state_ptr[s + 1] - state_ptr[s] > kMaxStates) return s;
  return -1;
}

}  // namespace align_frames
}  // namespace fdnn
