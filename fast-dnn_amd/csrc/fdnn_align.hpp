// fdnn_align.hpp -- the HIP-free half of FORCED ALIGNMENT (fdnn_align.hip): the best monotone path of a transcript's states
// over a segment's rows.  The emission, the step of the recursion, the validator, the transcript -> node-set conversion, the
// launch plan and a plain host restatement.  The arithmetic is stated here and nowhere else: the kernels call emission() and
// step() of this header.  tests/host/align_check.cpp builds it alone, under the sanitizers.
//
// Forced alignment is the caller of LazyOutputActivations (src/cpp/dnn.cc:355-392) that the per-segment node sets
// (fdnn_sets.hpp) were built for: a SEGMENT is one utterance -- T >= 1 consecutive rows -- with a transcript
// states[0 .. S) of output-node numbers, 1 <= S <= kMaxStates, each in [0, O), in any order, repeats allowed, and optional
// transition scores self_lp[0 .. S) and next_lp[0 .. S) (next_lp[S - 1] is never read; every value that is read is finite; a
// null array is an array of +0.0f, with the same bytes).
//
//   e(t, j) = loglik::score(p, log_prior[states[j]], floor)        p: row t's probability of node states[j]
//             F16 handles: rounded to fp16 (loglik::half_bits) and widened exactly; no handle: the row's value as it is
//   d[0][0] = e(0, 0);   d[0][j] = -inf for j > 0
//   stay = d[t-1][j]   + self_lp[j]
//   move = d[t-1][j-1] + next_lp[j-1]                              (j = 0: -inf + 0)
//   take = move > stay                                             (false on a tie and for a NaN on either side: stay)
//   d[t][j] = (take ? move : stay) + e(t, j)
//   total   = d[T-1][S-1]
//   path:   j = S-1; for t = T-1 .. 1: path[t] = j; if take[t][j]: j -= 1;   path[0] = j
//
// fp32 throughout, every + rounded once, nothing contracted (-ffp-contract=off on host and device), the selection a compare
// and a select -- not fmaxf / v_max_f32, which treat a NaN differently.  Additions and comparisons only: the bytes are a
// function of the scores and the transcript alone, whatever the parallel schedule.
//
//   total not finite (-inf: T < S or no path with a finite score; +inf; a NaN):
//     every element of path is -1.  A node or column out of range makes its state's emissions NaNs: the total is a NaN when
//     it is the last state, else -inf -- the move out of a NaN is never taken, the states above are never entered.  A NaN total is returned as THE quiet NaN 0x7fc00000 (hosts and devices disagree on the
//     payload of a NaN they make; nothing else of a NaN is ever looked at).
//   otherwise: path[t] is a state index, path[0] = 0, path[T-1] = S-1, steps are 0 or 1.
//   the tie rule's consequence: among paths of equal score the one whose moves come EARLIEST is returned; all-zero scores
//     give 0, 1, .., S-1, S-1, ..
//
// The band max(0, S-T+t) <= j <= min(S-1, t) is NOT used: kernels and restatement walk every state of every frame.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fdnn_loglik.hpp"

#if defined(__HIPCC__)
#define FDNN_ALIGN_HD __host__ __device__ __forceinline__
#else
#define FDNN_ALIGN_HD inline
#endif

namespace fdnn {
namespace align {

// ---------------------------------------------------------------- the limits
constexpr int kMaxStates = 16384;                // two fp32 rows of the recursion in LDS: 128 KiB of the CU's 160 KiB
constexpr int kMaxSegs = 64;                     // segments per launch (sets::kMaxSegs): longer tables go as several launches
constexpr int kWaveStates = 1024;                // the wave form's longest transcript: 64 lanes x 16 states
constexpr int kWaveLanes = 64;
constexpr int kWgThreads = 256;                  // the workgroup form
constexpr int kFramesInFlight = 16;              // rows whose probability loads are issued before the step that consumes them ...
constexpr int frames_in_flight(int K) { return K <= 2 ? kFramesInFlight : K >= 16 ? 2 : 32 / K; }  // ... at K states a lane: at most 32 values
constexpr int kBpLdsWords = 4096;                // a segment's take words stay in LDS when they are no more (16 KiB)
constexpr long long kMaxScratchBytes = 1ll << 30;  // the take words of one call that do not fit LDS
constexpr int kScores = -1;                      // `type` of a call without a handle: the rows are scores already
constexpr uint32_t kQuietNaN = 0x7fc00000u;
constexpr uint32_t kMinusInf = 0xff800000u;

using loglik::bits_of;
using loglik::float_of;

FDNN_ALIGN_HD bool finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

// fp16 bits -> fp32, exact (denormals, infinities and NaNs included)
inline float widen_half(uint16_t h) {
  const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16, ex = (h >> 10) & 0x1fu, man = h & 0x3ffu;
  if (ex == 0x1fu) return float_of(sign | 0x7f800000u | (man << 13));
  if (ex != 0) return float_of(sign | ((ex + 112u) << 23) | (man << 13));
  if (man == 0) return float_of(sign);
  uint32_t m = man, e = 113u;  // a denormal: man x 2^-24, normalised
  while (!(m & 0x400u)) m <<= 1, --e;
  return float_of(sign | (e << 23) | ((m & 0x3ffu) << 13));
}

// ---------------------------------------------------------------- the arithmetic
// v: the row's value for the state (a probability under a handle, a score without), or any NaN where the state's column or
// node is out of range
FDNN_ALIGN_HD float emission(float v, float log_prior, float floor, int type) {
  if (type == kScores) return v;
  float s = loglik::score(v, log_prior, floor);
  if (type == loglik::kF16) {
#if defined(__HIP_DEVICE_COMPILE__)
    s = static_cast<float>(static_cast<_Float16>(s));  // (the hardware's conversion is loglik::half_bits: tests hold both)
#else
    s = widen_half(loglik::half_bits(s));
#endif
  }
  return s;
}

// one state of one frame: d_same = d[t-1][j], d_prev = d[t-1][j-1] and next_prev = next_lp[j-1] (j = 0: -inf and +0)
FDNN_ALIGN_HD float step(float d_same, float self, float d_prev, float next_prev, float e, bool *take) {
  const float stay = d_same + self;
  const float move = d_prev + next_prev;
  const bool t = move > stay;
  *take = t;
  return (t ? move : stay) + e;
}

FDNN_ALIGN_HD uint32_t total_bits(float total) {
  const uint32_t b = bits_of(total);
  return (b & 0x7fffffffu) > 0x7f800000u ? kQuietNaN : b;
}

// ---------------------------------------------------------------- the validator
// The tables of a call on the host:
//   seg_rows  [n_segs + 1] int32  non-decreasing from seg_rows[0] >= 0 up to ctx_rows; segment s = rows [seg_rows[s], seg_rows[s + 1])
//   state_ptr [n_segs + 1] int32  state_ptr[0] == 0; segment s's transcript = states[state_ptr[s] .. state_ptr[s + 1])
//   states, self_lp, next_lp [state_ptr[n_segs]]   (the two transition arrays may be null)
// 0 = well formed, else -(s + 1) of the first segment that is not, and *why says what: its rows run backwards, past the
// context or are none (kBadRows), its transcript has no or more than kMaxStates states (kBadStates), one of its nodes is
// outside [0, output_dim) (kBadNode), it has fewer rows than states (kShort, only with need_path), a transition value that
// is read is not finite (kBadTransition).  Malformed tables as a whole answer as segment 0, kBadRows.
enum Why { kOk = 0, kBadRows, kBadStates, kBadNode, kShort, kBadTransition };

inline int check(const int32_t *seg_rows, const int32_t *state_ptr, const int32_t *states, const float *self_lp, const float *next_lp,
                 int n_segs, int output_dim, int ctx_rows, bool need_path, Why *why) {
  Why dummy;
  Why &w = why ? *why : dummy;
  w = kOk;
  if (n_segs <= 0) return 0;
  if (!seg_rows || !state_ptr || !states || seg_rows[0] < 0 || state_ptr[0] != 0) return w = kBadRows, -1;
  for (int s = 0; s < n_segs; ++s) {
    if (seg_rows[s + 1] <= seg_rows[s] || seg_rows[s + 1] > ctx_rows) return w = kBadRows, -(s + 1);
    const int32_t b = state_ptr[s], e = state_ptr[s + 1];
    if (e <= b || e - b > kMaxStates) return w = kBadStates, -(s + 1);
    for (int32_t i = b; i < e; ++i)
      if (states[i] < 0 || states[i] >= output_dim) return w = kBadNode, -(s + 1);
    if (need_path && seg_rows[s + 1] - seg_rows[s] < e - b) return w = kShort, -(s + 1);
    for (int32_t i = b; i < e; ++i) {
      if (self_lp && !finite_bits(bits_of(self_lp[i]))) return w = kBadTransition, -(s + 1);
      if (next_lp && i + 1 < e && !finite_bits(bits_of(next_lp[i]))) return w = kBadTransition, -(s + 1);
    }
  }
  return 0;
}

inline const char *why_text(Why w) {
  switch (w) {
    case kBadRows: return "seg_rows must begin at or above 0, rise strictly and end inside the context";
    case kBadStates: return "a transcript has 1 .. 16384 states and state_ptr begins at 0";
    case kBadNode: return "a transcript's node is outside [0, output_dim)";
    case kShort: return "fewer rows than states: no path";
    case kBadTransition: return "a transition score that is read is not finite";
    default: return "";
  }
}

// ---------------------------------------------------------------- transcripts -> node sets
// Each transcript's distinct nodes, ascending, as fdnn_calculate_lazy_sets takes them (set_ptr [n_segs + 1], nodes), and
// col [state_ptr[n_segs]]: the position of state j's node in its segment's set, i.e. the column of its probability in the
// segment's [rows][len] block.  nodes[set_ptr[s] + col[j]] == states[j].
struct Sets {
  std::vector<int32_t> set_ptr, nodes, col;
};

inline Sets build_sets(const int32_t *state_ptr, const int32_t *states, int n_segs) {
  Sets out;
  out.set_ptr.push_back(0);
  if (n_segs <= 0) return out;
  out.col.resize(static_cast<size_t>(state_ptr[n_segs]));
  std::vector<int32_t> set;
  for (int s = 0; s < n_segs; ++s) {
    set.assign(states + state_ptr[s], states + state_ptr[s + 1]);
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    for (int32_t i = state_ptr[s]; i < state_ptr[s + 1]; ++i)
      out.col[static_cast<size_t>(i)] = static_cast<int32_t>(std::lower_bound(set.begin(), set.end(), states[i]) - set.begin());
    out.nodes.insert(out.nodes.end(), set.begin(), set.end());
    out.set_ptr.push_back(static_cast<int32_t>(out.nodes.size()));
  }
  return out;
}

// ---------------------------------------------------------------- the host restatement, over bit patterns
// One segment: rows [T] of stride ld fp32 bits (row t at rows + t * ld), col [S] (a column outside [0, ld) gives a NaN
// emission and reads nothing), node [S] and log_prior [width] under a handle (type kF32 / kF16; a node outside [0, width)
// likewise), neither with type == kScores; self_lp / next_lp [S] or null.  -> path [T], *total (bits).
inline void ref(const uint32_t *rows, int T, long long ld, const int32_t *col, const int32_t *node, int S, const float *log_prior, int width,
                float floor, int type, const float *self_lp, const float *next_lp, int32_t *path, uint32_t *total) {
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);
  const size_t wpf = (static_cast<size_t>(S) + 7) / 8;
  std::vector<uint8_t> takes(static_cast<size_t>(T) * wpf, 0);
  std::vector<float> d(static_cast<size_t>(S), ninf), nd(static_cast<size_t>(S));
  auto e = [&](int t, int j) {
    const bool ok = col[j] >= 0 && col[j] < ld && (type == kScores || (node[j] >= 0 && node[j] < width));
    const float v = ok ? float_of(rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(col[j])]) : nan;
    return emission(v, ok && type != kScores ? log_prior[node[j]] : 0.0f, floor, type);
  };
  d[0] = e(0, 0);
  for (int t = 1; t < T; ++t) {
    for (int j = 0; j < S; ++j) {
      bool take;
      nd[static_cast<size_t>(j)] = step(d[static_cast<size_t>(j)], self_lp ? self_lp[j] : 0.0f, j ? d[static_cast<size_t>(j) - 1] : ninf,
                                        j && next_lp ? next_lp[j - 1] : 0.0f, e(t, j), &take);
      if (take) takes[static_cast<size_t>(t) * wpf + static_cast<size_t>(j >> 3)] |= static_cast<uint8_t>(1u << (j & 7));
    }
    d.swap(nd);
  }
  *total = total_bits(d[static_cast<size_t>(S) - 1]);
  if (!finite_bits(*total)) {
    std::fill(path, path + T, -1);
    return;
  }
  int j = S - 1;
  for (int t = T - 1; t >= 1; --t) {
    path[t] = j;
    if (takes[static_cast<size_t>(t) * wpf + static_cast<size_t>(j >> 3)] & (1u << (j & 7))) --j;
  }
  path[0] = j;
}

// ---------------------------------------------------------------- the launch plan
// Wave form (S <= kWaveStates): one wave per segment; lane l owns the K consecutive states [l K, l K + K), K the smallest of
// 1, 2, 4, 8, 16 with 64 K >= the LAUNCH's longest transcript; d, col, prior and transition values in registers, lane l - 1's
// last d by one DPP move, no LDS for d, no barrier.  The take bits of a frame are K 64-bit words: word k holds, at bit l, the
// bit of state l K + k -- at K = 16 sixty-four 16-bit words instead, lane l's at index l, bit k: the same 2 K 32-bit words.
// Workgroup form (any S <= kMaxStates): 256 threads per segment; thread i owns states i, i + 256, ..; d as two rows in LDS,
// one barrier per frame.  The take bits of a frame are ceil(S / 64) 64-bit words in state order.
// A segment's take words stay in LDS where they are at most kBpLdsWords 32-bit words, else they go to the call's scratch
// (read back from L2 by the back-trace).
enum Form { kWave = 0, kWorkgroup = 1 };

// mode (fdnn_debug_set_align_kernel): 0 the rule -- wave where allowed --, 1 the same, 2 always workgroup
inline Form form_for(int S, int mode) { return (mode != 2 && S <= kWaveStates) ? kWave : kWorkgroup; }
inline int states_per_lane(int S) {
  int k = 1;
  while (k * kWaveLanes < S) k *= 2;
  return k;
}
inline int take_words_per_frame(Form f, int S_or_K) { return f == kWave ? 2 * S_or_K : 2 * ((S_or_K + 63) / 64); }
// who owns state j: wave form lane and slot, workgroup form thread and round
inline void wave_owner(int j, int K, int *lane, int *slot) { *lane = j / K, *slot = j % K; }
inline void wg_owner(int j, int *thread, int *round) { *thread = j % kWgThreads, *round = j / kWgThreads; }

// One launch's segments, a kernel argument passed by value (2.6 KB): no table in device memory whose lifetime an enqueued
// call would have to manage.  Workgroup s of the launch is segment s of this table.
struct Launch {
  int form, K, n_segs, lds_bytes;  // K: the wave form's states per lane; lds_bytes: dynamic LDS of the launch
  int d_floats;                    // workgroup form: floats of ONE row of d in LDS (the longest transcript, rounded up to 64)
  int T[kMaxSegs], ld[kMaxSegs], state0[kMaxSegs], S[kMaxSegs], path_off[kMaxSegs], total_off[kMaxSegs];
  long long row_off[kMaxSegs];     // the segment's first row, in elements from the rows' base
  long long bp_off[kMaxSegs];      // the segment's take words in the scratch, in 32-bit words (even); -1: in LDS
};

struct Plan {
  std::vector<Launch> launches;
  long long scratch_words = 0;  // 32-bit words of take bits that do not fit LDS
};

// seg_T, row_off, row_ld [n_segs], state_ptr [n_segs + 1]; path offsets are the running sum of T, total offsets the segment
// numbers.  Every kMaxSegs consecutive segments give one launch per form that occurs among them.
inline Plan plan(const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr, int n_segs, int mode) {
  Plan p;
  int path_off = 0;
  for (int s0 = 0; s0 < n_segs; s0 += kMaxSegs) {
    const int s1 = std::min(n_segs, s0 + kMaxSegs);
    const int path0 = path_off;
    for (int f = kWave; f <= kWorkgroup; ++f) {
      Launch l{};
      l.form = f, l.K = 1;
      int max_s = 0;
      for (int s = s0; s < s1; ++s)
        if (form_for(state_ptr[s + 1] - state_ptr[s], mode) == f) max_s = std::max(max_s, state_ptr[s + 1] - state_ptr[s]);
      if (!max_s) continue;
      if (f == kWave) l.K = states_per_lane(max_s);
      else l.d_floats = (max_s + 63) / 64 * 64;
      int lds_bp = 0;
      path_off = path0;
      for (int s = s0; s < s1; ++s) {
        const int S = state_ptr[s + 1] - state_ptr[s], T = seg_T[s];
        if (form_for(S, mode) == f) {
          const int i = l.n_segs++;
          l.T[i] = T, l.ld[i] = row_ld[s], l.state0[i] = state_ptr[s], l.S[i] = S, l.path_off[i] = path_off, l.total_off[i] = s;
          l.row_off[i] = row_off[s];
          const long long words = static_cast<long long>(T) * take_words_per_frame(static_cast<Form>(f), f == kWave ? l.K : S);
          if (words <= kBpLdsWords) {
            l.bp_off[i] = -1;
            lds_bp = std::max(lds_bp, static_cast<int>(words));
          } else {
            l.bp_off[i] = p.scratch_words;
            p.scratch_words += words;
          }
        }
        path_off += T;
      }
      l.lds_bytes = 4 * (lds_bp + 2 * l.d_floats);
      p.launches.push_back(l);
    }
    path_off = path0;
    for (int s = s0; s < s1; ++s) path_off += seg_T[s];
  }
  return p;
}

}  // namespace align
}  // namespace fdnn
