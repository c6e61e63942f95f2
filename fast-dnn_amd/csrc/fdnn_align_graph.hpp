// fdnn_align_graph.hpp -- the HIP-free half of ALIGNMENT GRAPHS (fdnn_align_graph.hip): the best path over ANY arc set of a
// segment's states -- optional silence, pronunciation variants, skips, loops --, where fdnn_align.hpp walks a strict chain.
// The candidate step, the final selection, the validator, the launch plan and a plain host restatement.  The arithmetic is
// stated here and nowhere else: the kernels call relax() and better_end() of this header and align::emission() of the
// sibling's.  tests/host/align_graph_check.cpp builds it alone, under the sanitizers.
//
// A SEGMENT is one utterance (LazyOutputActivations' caller, src/cpp/dnn.cc:355-392): T >= 1 rows and a graph of S states,
// 1 <= S <= align::kMaxStates.  State j has an output node states[j] (repeats are normal) and the incoming arcs
// arc_ptr[j] .. arc_ptr[j + 1], IN THE ORDER THE CALLER WROTE THEM.  An arc has a source arc_src[a], a state index local to
// the segment, any value in [0, S) -- self-loops, forward, skip and backward arcs alike -- and a finite score arc_lp[a].
// Every arc consumes a frame: d[t] reads d[t - 1] only, and no topological order is needed.
//
//   seg_rows [n_segs + 1], state_ptr [n_segs + 1], states [N], N = state_ptr[n_segs]      as fdnn_align.hpp
//   arc_ptr  [N + 1]        arc_ptr[0] == 0, non-decreasing: a segment's arcs are contiguous
//   arc_src, arc_lp [arc_ptr[N]]
//   start_lp, final_lp [N] or null: each value finite or -inf.  A null start_lp is +0.0f for the segment's state 0 and -inf
//                           elsewhere; a null final_lp is +0.0f for its state S - 1 and -inf elsewhere.
//
//   e(t, j)  = align::emission(...)                     exactly the sibling's: F32 / F16 handle, or the rows are scores
//   d[0][j]  = start_lp[j] + e(0, j)
//   t >= 1:    best = -inf; from = -1
//              for a in arc_ptr[j] .. arc_ptr[j + 1], in that order:
//                cand = d[t-1][arc_src[a]] + arc_lp[a]
//                if (cand > best) best = cand, from = arc_src[a]          (a tie and a NaN: not taken)      -- relax()
//              d[t][j] = best + e(t, j);  bp[t][j] = from
//   total:     best = -inf; end = -1; for j = 0 .. S-1 ascending: cand = d[T-1][j] + final_lp[j]; if (cand > best) best = cand, end = j
//   path:      j = end; for t = T-1 .. 1: path[t] = j; j = bp[t][j];   path[0] = j
//
// fp32 throughout, every + rounded once, nothing contracted (-ffp-contract=off on host and device, no fast-math or
// flush-to-zero flag), the selection that compare and select -- not fmaxf / v_max_f32.  Additions and comparisons only: the
// bytes are a function of the scores and the graph alone, whatever the parallel schedule.
//
//   total not finite (-inf: no path; +inf): every element of path is -1.  A NaN candidate is never taken ANYWHERE, the final
//     selection included, so the total is never a NaN.  THIS DIFFERS FROM THE CHAIN CONTRACT, whose `stay` is kept when it is
//     a NaN and whose total can be one (returned as 0x7fc00000): here a state whose emission is a NaN holds a NaN for that
//     frame and no arc out of it is taken, which leaves -inf where the chain leaves a NaN.
//   ties: among equal candidates the EARLIEST arc of the list wins, among equal final states the lowest.  The order of a
//     state's arcs is part of the input.
//   a state without arcs is reachable at t = 0 only.
//   device-rows form: a source outside [0, S) makes that candidate a NaN and reads nothing; a column or node out of range
//     makes the emission a NaN, as in the sibling.
//   a finite total's path never meets from = -1: d[t][j] is finite only if a candidate was taken, a taken candidate is above
//     -inf, so its source's d[t-1] is finite or +inf, and +inf anywhere on the best path makes the total +inf or a NaN that
//     is not taken.
//
// THE CHAIN AS A SPECIAL CASE.  Take state j's arcs as (j with self_lp[j], then j - 1 with next_lp[j - 1]; state 0 the first
// alone) and null start_lp / final_lp.  Let stay and move be the sibling's two candidates and let no d be a NaN (emissions
// neither a NaN nor +inf: -inf + +inf is the one NaN additions make).  stay > -inf: best = stay after the first arc, and the
// second is taken iff move > stay -- the sibling's `take`; a tie stays.  stay = -inf: the first arc is not taken (a tie with
// best), the second iff move > -inf = stay, again `take`; d = move + e either way.  Both -inf: nothing is taken, d = -inf +
// e = the sibling's stay + e.  So every d has the sibling's bytes, and from = j - 1 exactly where take is set.  d[0]: 0.0f +
// e(0, 0) and the sibling's e(0, 0); the total: d[T-1][S-1] + 0.0f and the sibling's d[T-1][S-1].  x + 0.0f has x's bytes
// for every x but -0.0f, which becomes +0.0f; a -0.0f there needs an emission of -0.0f added to a -0.0f (x + y is -0.0f
// only where both are), i.e. a caller who writes -0.0f transition scores over -0.0f emissions, and then differs in the sign
// bit of a zero total only.  T < S: the last state is never entered, the total is -inf, the path -1 everywhere, both ways.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fdnn_align.hpp"

namespace fdnn {
namespace align_graph {

using align::bits_of;
using align::finite_bits;
using align::float_of;
using align::kMinusInf;
using align::kQuietNaN;
using align::kScores;

// ---------------------------------------------------------------- the limits
using align::kMaxScratchBytes;  // the back-pointers of one call that do not fit LDS: above it FDNN_E_ARG
using align::kMaxSegs;          // segments per launch
using align::kMaxStates;        // two fp32 rows of d in LDS
using align::kWgThreads;
using align::kWaveLanes;
// the wave form's largest graph: 4 states a lane -- and the largest the RULE gives it: one state a lane.  One wave walks its
// lane's states one after the other, each a chain of dependent LDS reads per arc, while the workgroup form spreads them over
// four waves: measured, the wave form -- it alone keeps the next rows' loads in flight across frames
// -- takes a quarter less time up to 64 states, 11 % more at 128 and 77 % more at 256.  So it may be FORCED up to 256 states and is
// chosen up to 64, not the chain form's 1024
constexpr int kWaveStates = 256;
constexpr int kWaveRuleStates = 64;
// the wave form's states per lane K = 1, 2 or 4 (the LAUNCH's largest graph) and the rows whose loads are in flight ahead of
// the frame that consumes them: 16 values a lane, whatever K; their emissions wait in an LDS ring of 16 / K frames x 64 K states
inline int wave_slots(int S) {
  int k = 1;
  while (k * kWaveLanes < S) k *= 2;
  return k;
}
constexpr int kRowValues = 16;
constexpr int frames_in_flight(int K) { return kRowValues / K; }
constexpr int kEmissionRing = kRowValues * kWaveLanes;  // floats
// arcs of one segment: 8 a state at the longest graph.  Both forms read the arc table of a large graph again every frame;
// at 8 bytes an arc 2^17 of them are 1 MiB, which stays in the 4 MiB L2 beside the rows
constexpr int kMaxArcs = 1 << 17;
// the wave form stages a segment's arc table in LDS (lp 4 bytes, src 2) where it has at most this many arcs: 24 KiB, so that
// d (2 KiB), the emissions (4 KiB), the arc offsets (1.3 KiB), the arcs and the back-pointers (16 KiB) stay inside the 64 KiB every
// launch gets unasked
constexpr int kArcLdsArcs = 4096;
constexpr int kBpLdsWords = align::kBpLdsWords;  // a segment's back-pointers (16 bits a state and frame) stay in LDS up to here
constexpr uint16_t kNoSource = 0xffffu;          // from = -1 in 16 bits; also what a staged source outside [0, S) becomes

// ---------------------------------------------------------------- the arithmetic
// one arc into a state: d_src = d[t-1][src] (any NaN where src is outside [0, S))
FDNN_ALIGN_HD void relax(float d_src, float lp, int src, float *best, int *from) {
  const float cand = d_src + lp;
  if (cand > *best) *best = cand, *from = src;
}

// the final selection, one state: cand = d[T-1][j] + final_lp[j]; among equal candidates the lowest j.  Walked in ascending
// j with (-inf, -1) first this is the contract's loop (idx < *end is then never true); in any other order, e.g. a tree
// over lanes, it gives the same (best, end): the maximum under > and, among its equals, the lowest index.
FDNN_ALIGN_HD void better_end(float cand, int idx, float *best, int *end) {
  if (cand > *best || (cand == *best && idx >= 0 && idx < *end)) *best = cand, *end = idx;
}

// the values a null start_lp / final_lp stands for
FDNN_ALIGN_HD float start_of(const float *start_lp, int j) { return start_lp ? start_lp[j] : (j == 0 ? 0.0f : float_of(kMinusInf)); }
FDNN_ALIGN_HD float final_of(const float *final_lp, int j, int S) { return final_lp ? final_lp[j] : (j == S - 1 ? 0.0f : float_of(kMinusInf)); }

// ---------------------------------------------------------------- the validator
// The tables of a call on the host.  0 = well formed, else -(s + 1) of the first segment that is not, and *why says what.
// kBadRows, kBadStates, kBadNode: the sibling's.  kBadArcPtr: arc_ptr does not begin at 0 or decreases.  kTooManyArcs: above
// kMaxArcs in the segment.  kBadSource: a source outside [0, S).  kBadArcScore: an arc score that is not finite.
// kBadStartFinal: a start or final value that is a NaN or +inf.  kNoStart / kNoFinal: no state with a finite one.
// Malformed tables as a whole answer as segment 0 (kBadRows; arc tables kBadArcPtr).
enum Why { kOk = 0, kBadRows, kBadStates, kBadNode, kBadArcPtr, kTooManyArcs, kBadSource, kBadArcScore, kBadStartFinal, kNoStart, kNoFinal };

struct Tables {
  const int32_t *seg_rows = nullptr, *state_ptr = nullptr, *states = nullptr, *arc_ptr = nullptr, *arc_src = nullptr;
  const float *arc_lp = nullptr, *start_lp = nullptr, *final_lp = nullptr;
  int n_segs = 0;
};

inline bool start_final_ok(float v) { return v == float_of(kMinusInf) || finite_bits(bits_of(v)); }

inline int check(const Tables &t, int output_dim, int ctx_rows, Why *why) {
  Why dummy;
  Why &w = why ? *why : dummy;
  w = kOk;
  if (t.n_segs <= 0) return 0;
  if (!t.seg_rows || !t.state_ptr || !t.states || t.seg_rows[0] < 0 || t.state_ptr[0] != 0) return w = kBadRows, -1;
  if (!t.arc_ptr || t.arc_ptr[0] != 0) return w = kBadArcPtr, -1;
  for (int s = 0; s < t.n_segs; ++s) {
    if (t.seg_rows[s + 1] <= t.seg_rows[s] || t.seg_rows[s + 1] > ctx_rows) return w = kBadRows, -(s + 1);
    const int32_t b = t.state_ptr[s], e = t.state_ptr[s + 1];
    if (e <= b || e - b > kMaxStates) return w = kBadStates, -(s + 1);
    const int S = e - b;
    for (int32_t i = b; i < e; ++i)
      if (t.states[i] < 0 || t.states[i] >= output_dim) return w = kBadNode, -(s + 1);
    for (int32_t i = b; i < e; ++i)
      if (t.arc_ptr[i + 1] < t.arc_ptr[i]) return w = kBadArcPtr, -(s + 1);
    const int32_t a0 = t.arc_ptr[b], a1 = t.arc_ptr[e];
    if (a1 - a0 > kMaxArcs) return w = kTooManyArcs, -(s + 1);
    if (a1 > a0 && (!t.arc_src || !t.arc_lp)) return w = kBadArcPtr, -(s + 1);
    for (int32_t a = a0; a < a1; ++a)
      if (t.arc_src[a] < 0 || t.arc_src[a] >= S) return w = kBadSource, -(s + 1);
    for (int32_t a = a0; a < a1; ++a)
      if (!finite_bits(bits_of(t.arc_lp[a]))) return w = kBadArcScore, -(s + 1);
    bool any_start = !t.start_lp, any_final = !t.final_lp;
    for (int32_t i = b; i < e; ++i) {
      if (t.start_lp && !start_final_ok(t.start_lp[i])) return w = kBadStartFinal, -(s + 1);
      if (t.final_lp && !start_final_ok(t.final_lp[i])) return w = kBadStartFinal, -(s + 1);
      any_start = any_start || finite_bits(bits_of(t.start_lp[i]));
      any_final = any_final || finite_bits(bits_of(t.final_lp[i]));
    }
    if (!any_start) return w = kNoStart, -(s + 1);
    if (!any_final) return w = kNoFinal, -(s + 1);
  }
  return 0;
}

inline const char *why_text(Why w) {
  switch (w) {
    case kBadRows: return "seg_rows must begin at or above 0, rise strictly and end inside the context";
    case kBadStates: return "a graph has 1 .. 16384 states and state_ptr begins at 0";
    case kBadNode: return "a state's node is outside [0, output_dim)";
    case kBadArcPtr: return "arc_ptr begins at 0 and does not decrease";
    case kTooManyArcs: return "a segment has at most 131072 arcs";
    case kBadSource: return "an arc's source is outside [0, S)";
    case kBadArcScore: return "an arc score is not finite";
    case kBadStartFinal: return "a start or final value is finite or -inf";
    case kNoStart: return "no state has a finite start value";
    case kNoFinal: return "no state has a finite final value";
    default: return "";
  }
}

// ---------------------------------------------------------------- the host restatement, over bit patterns
// One segment: rows, col, node, log_prior, type as align::ref.  arc_ptr [S + 1] are the segment's entries of the call's
// table (non-decreasing; they index arc_src / arc_lp, the call's arrays); start_lp / final_lp [S] or null.  A source outside
// [0, S) gives a NaN candidate and reads nothing.  -> path [T], *total (bits).
inline void ref(const uint32_t *rows, int T, long long ld, const int32_t *col, const int32_t *node, int S, const float *log_prior, int width,
                float floor, int type, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp,
                const float *final_lp, int32_t *path, uint32_t *total) {
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);
  const size_t Ss = static_cast<size_t>(S);
  std::vector<uint16_t> bp(static_cast<size_t>(T) * Ss, kNoSource);
  std::vector<float> d(Ss), nd(Ss);
  auto e = [&](int t, int j) {
    const bool ok = col[j] >= 0 && col[j] < ld && (type == kScores || (node[j] >= 0 && node[j] < width));
    const float v = ok ? float_of(rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(col[j])]) : nan;
    return align::emission(v, ok && type != kScores ? log_prior[node[j]] : 0.0f, floor, type);
  };
  for (int j = 0; j < S; ++j) d[static_cast<size_t>(j)] = start_of(start_lp, j) + e(0, j);
  for (int t = 1; t < T; ++t) {
    for (int j = 0; j < S; ++j) {
      float best = ninf;
      int from = -1;
      for (int32_t a = arc_ptr[j]; a < arc_ptr[j + 1]; ++a) {
        const int src = arc_src[a];
        relax(src >= 0 && src < S ? d[static_cast<size_t>(src)] : nan, arc_lp[a], src, &best, &from);
      }
      nd[static_cast<size_t>(j)] = best + e(t, j);
      bp[static_cast<size_t>(t) * Ss + static_cast<size_t>(j)] = static_cast<uint16_t>(from);
    }
    d.swap(nd);
  }
  float best = ninf;
  int end = -1;
  for (int j = 0; j < S; ++j) better_end(d[static_cast<size_t>(j)] + final_of(final_lp, j, S), j, &best, &end);
  *total = align::total_bits(best);
  if (!finite_bits(*total)) {
    std::fill(path, path + T, -1);
    return;
  }
  int j = end;
  for (int t = T - 1; t >= 1; --t) {
    path[t] = j;
    j = std::min<int>(bp[static_cast<size_t>(t) * Ss + static_cast<size_t>(j)], S - 1);  // (never kNoSource on a finite path: see the top)
  }
  path[0] = j;
}

// ---------------------------------------------------------------- the launch plan
// Wave form (S <= kWaveRuleStates by the rule, <= kWaveStates forced): one wave per segment; lane l owns states l, l + 64, ..; d as two rows in LDS and a ring of
// emissions, no workgroup barrier; the segment's arc offsets, and its arc table where it has at most kArcLdsArcs arcs, are staged in LDS once.
// Workgroup form (any S <= kMaxStates): 256 threads per segment; thread i owns states i, i + 256, ..; d as two rows in LDS,
// one barrier per frame; arcs from the L2.
// Back-pointers: T x S 16-bit sources, row t at t S (row 0 is not used); in LDS where they are at most kBpLdsWords 32-bit
// words, else in the call's scratch.
enum Form { kWave = 0, kWorkgroup = 1 };

// mode (fdnn_debug_set_align_graph_kernel): 0 the rule -- wave up to kWaveRuleStates --, 1 wave where allowed (up to kWaveStates),
// 2 always workgroup
inline Form form_for(int S, int mode) { return (mode == 1 ? S <= kWaveStates : (mode == 0 && S <= kWaveRuleStates)) ? kWave : kWorkgroup; }
inline long long bp_words(int T, int S) { return (static_cast<long long>(T) * S + 1) / 2; }
inline bool arcs_staged(Form f, int n_arcs) { return f == kWave && n_arcs <= kArcLdsArcs; }

constexpr int kWgReduceWords = 16;  // the workgroup form's final selection: (best, end) of four waves, then of the segment

// One launch's segments, a kernel argument passed by value (3.1 KB).  Workgroup s of the launch is segment s of this table.
struct Launch {
  int form, n_segs, lds_bytes;
  int K;         // wave form: states per lane, 1, 2 or 4
  int d_floats;  // floats of ONE row of d in LDS: the launch's largest graph, rounded up to 64 (wave form: 64 K)
  int arc_cap;   // wave form: the most arcs a segment of the launch stages (even; 0: none does)
  int bp_words;  // the most back-pointer words a segment of the launch keeps in LDS
  int T[kMaxSegs], ld[kMaxSegs], state0[kMaxSegs], S[kMaxSegs], path_off[kMaxSegs], total_off[kMaxSegs];
  int arc0[kMaxSegs], n_arcs[kMaxSegs];  // the segment's arcs in the call's arrays, FROM THE HOST TABLE: what bounds every arc index
  long long row_off[kMaxSegs];           // the segment's first row, in elements from the rows' base
  long long bp_off[kMaxSegs];            // the segment's back-pointers in the scratch, in 32-bit words; -1: in LDS
};

// the wave form's LDS, in 32-bit words: two rows of d, the ring of emissions, the arc offsets [S + 1], the staged scores and sources, the back-pointers
inline int wave_lds_words(int d_floats, int arc_cap, int bp) { return 2 * d_floats + kEmissionRing + (d_floats + 64) + arc_cap + arc_cap / 2 + bp; }
inline int wg_lds_words(int d_floats, int bp) { return 2 * d_floats + kWgReduceWords + bp; }

struct Plan {
  std::vector<Launch> launches;
  long long scratch_words = 0;  // 32-bit words of back-pointers that do not fit LDS
};

// seg_T, row_off, row_ld [n_segs], state_ptr [n_segs + 1], arc_ptr [state_ptr[n_segs] + 1] or null (no arcs: the scratch
// size does not depend on them); path offsets are the running sum of T, total offsets the segment numbers.  Every kMaxSegs
// consecutive segments give one launch per form that occurs among them.
inline Plan plan(const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr, const int32_t *arc_ptr, int n_segs,
                 int mode) {
  Plan p;
  int path_off = 0;
  for (int s0 = 0; s0 < n_segs; s0 += kMaxSegs) {
    const int s1 = std::min(n_segs, s0 + kMaxSegs);
    const int path0 = path_off;
    for (int f = kWave; f <= kWorkgroup; ++f) {
      Launch l{};
      l.form = f;
      int max_s = 0;
      path_off = path0;
      for (int s = s0; s < s1; ++s) {
        const int S = state_ptr[s + 1] - state_ptr[s], T = seg_T[s];
        if (form_for(S, mode) == f) {
          const int i = l.n_segs++;
          max_s = std::max(max_s, S);
          l.T[i] = T, l.ld[i] = row_ld[s], l.state0[i] = state_ptr[s], l.S[i] = S, l.path_off[i] = path_off, l.total_off[i] = s;
          l.row_off[i] = row_off[s];
          l.arc0[i] = arc_ptr ? arc_ptr[state_ptr[s]] : 0;
          l.n_arcs[i] = arc_ptr ? arc_ptr[state_ptr[s + 1]] - arc_ptr[state_ptr[s]] : 0;
          if (arcs_staged(static_cast<Form>(f), l.n_arcs[i])) l.arc_cap = std::max(l.arc_cap, (l.n_arcs[i] + 1) / 2 * 2);
          const long long words = bp_words(T, S);
          if (words <= kBpLdsWords) {
            l.bp_off[i] = -1;
            l.bp_words = std::max(l.bp_words, static_cast<int>(words));
          } else {
            l.bp_off[i] = p.scratch_words;
            p.scratch_words += words;
          }
        }
        path_off += T;
      }
      if (!l.n_segs) continue;
      l.K = f == kWave ? wave_slots(max_s) : 1;
      l.d_floats = f == kWave ? l.K * kWaveLanes : (max_s + 63) / 64 * 64;  // (the wave form's rows hold every slot of every lane)
      l.lds_bytes = 4 * (f == kWave ? wave_lds_words(l.d_floats, l.arc_cap, l.bp_words) : wg_lds_words(l.d_floats, l.bp_words));
      p.launches.push_back(l);
    }
    path_off = path0;
    for (int s = s0; s < s1; ++s) path_off += seg_T[s];
  }
  return p;
}

}  // namespace align_graph
}  // namespace fdnn
