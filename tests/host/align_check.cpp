// align_check.cpp -- fdnn_align.hpp (the emission, the step, the validator, the transcript -> node-set conversion, the launch
// plan and the host restatement of forced alignment), alone and under the sanitizers (tests/test_align_host.py builds and runs
// this).  Must be built with -ffp-contract=off and WITHOUT a flush-to-zero or fast-math flag.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "fdnn_align.hpp"

using namespace fdnn;
using align::bits_of;
using align::float_of;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

const float kInf = std::numeric_limits<float>::infinity();
const float kNaN = std::numeric_limits<float>::quiet_NaN();

struct Case {
  int T, S;
  std::vector<float> e;  // [T][S] scores
  std::vector<float> self, next;
  std::vector<int32_t> col;
};

struct Result {
  std::vector<int32_t> path;
  uint32_t total;
};

Result run_ref(const Case &c, bool trans = true) {
  Result r{std::vector<int32_t>(size_t(c.T), 77), 0};
  align::ref(reinterpret_cast<const uint32_t *>(c.e.data()), c.T, c.S, c.col.data(), nullptr, c.S, nullptr, 0, 0.0f, align::kScores,
             trans ? c.self.data() : nullptr, trans ? c.next.data() : nullptr, r.path.data(), &r.total);
  return r;
}

// a path's score in the recursion's own left-to-right fp32 order
float path_score(const Case &c, const std::vector<int32_t> &p, bool trans = true) {
  float acc = c.e[size_t(p[0])];
  for (int t = 1; t < c.T; ++t) {
    const int j = p[size_t(t)];
    const float tr = !trans ? 0.0f : (j != p[size_t(t) - 1] ? c.next[size_t(j) - 1] : c.self[size_t(j)]);
    acc = (acc + tr) + c.e[size_t(t) * c.S + j];
  }
  return acc;
}

// every monotone path 0 -> S - 1 with steps 0 or 1: the best score, and among the paths of that score the one that is in the
// higher state at the LAST frame in which two of them differ (its moves come earliest)
void brute(const Case &c, bool trans, float *best, std::vector<int32_t> *best_path, long long *count) {
  *count = 0;
  bool have = false;
  for (unsigned mask = 0; mask < (1u << (c.T - 1)); ++mask) {  // bit t - 1: a move into frame t
    if (__builtin_popcount(mask) != c.S - 1) continue;
    std::vector<int32_t> p(size_t(c.T), 0);
    for (int t = 1; t < c.T; ++t) p[size_t(t)] = p[size_t(t) - 1] + int((mask >> (t - 1)) & 1u);
    ++*count;
    const float s = path_score(c, p, trans);
    bool better = !have || s > *best;
    if (have && s == *best)
      for (int t = c.T - 1; t >= 0; --t)
        if (p[size_t(t)] != (*best_path)[size_t(t)]) {
          better = p[size_t(t)] > (*best_path)[size_t(t)];
          break;
        }
    if (better) *best = s, *best_path = p, have = true;
  }
}

Case random_case(int T, int S, std::mt19937 &rng, bool integers) {
  Case c{T, S, std::vector<float>(size_t(T) * S), std::vector<float>(size_t(S)), std::vector<float>(size_t(S)), std::vector<int32_t>(size_t(S))};
  std::normal_distribution<float> n(0.0f, 1.0f);
  std::uniform_real_distribution<float> u(0.05f, 0.95f);
  std::uniform_int_distribution<int> k(-3, 3);
  for (float &v : c.e) v = integers ? float(k(rng)) : 3.0f * n(rng) - 5.0f;
  for (int j = 0; j < S; ++j) {
    const float a = u(rng);
    c.self[size_t(j)] = integers ? 0.0f : std::log(a);
    c.next[size_t(j)] = integers ? 0.0f : std::log(1.0f - a);
    c.col[size_t(j)] = j;
  }
  c.next[size_t(S) - 1] = kNaN;  // never read
  return c;
}

void check_ref_against_brute_force() {
  std::mt19937 rng(1);
  long long cases = 0, paths = 0, ties = 0;
  for (int T = 1; T <= 10; ++T)
    for (int S = 1; S <= std::min(T, 5); ++S)
      for (int rep = 0; rep < 8; ++rep) {
        const bool integers = rep >= 4;
        const Case c = random_case(T, S, rng, integers);
        const Result r = run_ref(c);
        float best = 0;
        std::vector<int32_t> bp;
        long long n = 0;
        brute(c, true, &best, &bp, &n);
        CHECK(n > 0 && align::finite_bits(r.total));
        CHECK(r.total == bits_of(best));                         // rounded addition is monotone: the maxima coincide
        CHECK(bits_of(path_score(c, r.path)) == r.total);        // the returned path has the returned score
        CHECK(r.path[0] == 0 && r.path[size_t(T) - 1] == S - 1);
        for (int t = 1; t < T; ++t) CHECK(r.path[size_t(t)] - r.path[size_t(t) - 1] == 0 || r.path[size_t(t)] - r.path[size_t(t) - 1] == 1);
        if (integers) {  // exact arithmetic: the tie rule picks the path whose moves come earliest
          CHECK(r.path == bp);
          const Result z = run_ref(c, false);  // null transitions: the bytes of passing zeros
          CHECK(z.total == r.total && z.path == r.path);
          ++ties;
        }
        ++cases, paths += n;
      }
  std::printf("ref against brute force: %lld cases, %lld paths, %lld with integer ties\n", cases, paths, ties);
}

void check_ties_and_nans() {
  bool take = true;
  CHECK(align::step(1.0f, 0.0f, 1.0f, 0.0f, 2.0f, &take) == 3.0f && !take);         // a tie: stay
  CHECK(align::step(1.0f, 0.0f, 2.0f, 0.0f, 2.0f, &take) == 4.0f && take);
  CHECK(align::step(1.0f, 0.0f, kNaN, 0.0f, 2.0f, &take) == 3.0f && !take);         // a NaN on the move side is not taken
  const float s = align::step(kNaN, 0.0f, 5.0f, 0.0f, 2.0f, &take);
  CHECK(s != s && !take);                                                            // a NaN on the stay side: stay, a NaN
  CHECK(align::step(-kInf, 0.0f, -kInf, 0.0f, 1.0f, &take) == -kInf && !take);
  CHECK(align::total_bits(float_of(0xffc12345u)) == align::kQuietNaN && align::total_bits(-kInf) == align::kMinusInf);
  CHECK(align::total_bits(1.5f) == bits_of(1.5f));

  std::mt19937 rng(2);
  {  // all-zero scores: 0, 1, .., S - 1, S - 1, ..
    Case c = random_case(12, 5, rng, true);
    std::fill(c.e.begin(), c.e.end(), 0.0f);
    const Result r = run_ref(c, false);
    CHECK(r.total == 0u);
    for (int t = 0; t < 12; ++t) CHECK(r.path[size_t(t)] == std::min(t, 4));
  }
  auto all_minus_one = [](const Result &r) {
    for (int32_t v : r.path)
      if (v != -1) return false;
    return true;
  };
  {  // T < S
    const Result r = run_ref(random_case(3, 5, rng, false));
    CHECK(r.total == align::kMinusInf && all_minus_one(r));
  }
  {  // no path with a finite score
    Case c = random_case(9, 4, rng, false);
    std::fill(c.e.begin(), c.e.end(), -kInf);
    const Result r = run_ref(c);
    CHECK(r.total == align::kMinusInf && all_minus_one(r));
  }
  {  // +inf
    Case c = random_case(9, 4, rng, false);
    for (int j = 0; j < 4; ++j) c.e[size_t(4) * 4 + j] = kInf;
    const Result r = run_ref(c);
    CHECK(r.total == bits_of(kInf) && all_minus_one(r));
  }
  {  // a NaN on every path reaches the total, as THE quiet NaN
    Case c = random_case(9, 4, rng, false);
    for (int j = 0; j < 4; ++j) c.e[size_t(4) * 4 + j] = float_of(0xffc00001u);
    const Result r = run_ref(c);
    CHECK(r.total == align::kQuietNaN && all_minus_one(r));
  }
  {  // state 2 is a NaN from frame 20 on: the move out of it is not taken from then on, a path that has left stays finite
    Case c = random_case(30, 6, rng, false);
    for (int t = 20; t < 30; ++t) c.e[size_t(t) * 6 + 2] = kNaN;
    const Result r = run_ref(c);
    CHECK(align::finite_bits(r.total));
    for (int t = 20; t < 30; ++t) CHECK(r.path[size_t(t)] > 2);
    CHECK(bits_of(path_score(c, r.path)) == r.total);
  }
  {  // a column out of range: a NaN emission, nothing read.  The move out of a NaN is never taken, so the states above it
     // are never entered: -inf -- unless it is the last state, whose NaN is the total
    Case c = random_case(9, 4, rng, false);
    c.col[2] = 4;
    Result r = run_ref(c);
    CHECK(r.total == align::kMinusInf && all_minus_one(r));
    c.col[2] = 2, c.col[3] = -1;
    r = run_ref(c);
    CHECK(r.total == align::kQuietNaN && all_minus_one(r));
  }
  {  // under a handle: the emission is loglik::score, an F16 handle's rounded to fp16 and widened; a node out of range is a NaN
    const float lp[3] = {-1.0f, -2.0f, -0.5f};
    const float rows[4] = {0.5f, 0.25f, 0.125f, 0.75f};  // [2][2]
    const int32_t col[2] = {1, 0}, node[2] = {2, 0};
    int32_t path[2];
    uint32_t total;
    for (int type : {loglik::kF32, loglik::kF16}) {
      align::ref(reinterpret_cast<const uint32_t *>(rows), 2, 2, col, node, 2, lp, 3, -20.0f, type, nullptr, nullptr, path, &total);
      float e0 = loglik::score(0.25f, -0.5f, -20.0f), e1 = loglik::score(0.125f, -1.0f, -20.0f);
      if (type == loglik::kF16) e0 = align::widen_half(loglik::half_bits(e0)), e1 = align::widen_half(loglik::half_bits(e1));
      CHECK(total == bits_of((e0 + 0.0f) + e1) && path[0] == 0 && path[1] == 1);
    }
    const int32_t bad[2] = {2, 3};  // (the last state's node)
    align::ref(reinterpret_cast<const uint32_t *>(rows), 2, 2, col, bad, 2, lp, 3, -20.0f, loglik::kF32, nullptr, nullptr, path, &total);
    CHECK(total == align::kQuietNaN && path[0] == -1 && path[1] == -1);
  }
  // the widening is exact: every fp16 value comes back from the conversion
  for (uint32_t h = 0; h < 0x10000u; ++h) {
    const float w = align::widen_half(uint16_t(h));
    if ((h & 0x7c00u) == 0x7c00u && (h & 0x3ffu)) CHECK(w != w);
    else CHECK(loglik::half_bits(w) == h);
#if defined(__FLT16_MAX__)
    _Float16 f;
    const uint16_t hb = uint16_t(h);
    std::memcpy(&f, &hb, 2);
    if (w == w) CHECK(bits_of(float(f)) == bits_of(w));
#endif
  }
  std::printf("ties, NaNs, non-finite totals, handles and the fp16 widening ok\n");
}

void check_build_sets() {
  const int32_t state_ptr[4] = {0, 7, 7 + 3, 7 + 3 + 1};
  const int32_t states[11] = {9, 7, 7, 3, 9, 0, 3, /**/ 5, 5, 5, /**/ 2};
  const align::Sets s = align::build_sets(state_ptr, states, 3);
  CHECK((s.set_ptr == std::vector<int32_t>{0, 4, 5, 6}));
  CHECK((s.nodes == std::vector<int32_t>{0, 3, 7, 9, 5, 2}));
  for (int g = 0; g < 3; ++g)
    for (int i = state_ptr[g]; i < state_ptr[g + 1]; ++i) {
      CHECK(s.col[size_t(i)] >= 0 && s.col[size_t(i)] < s.set_ptr[size_t(g) + 1] - s.set_ptr[size_t(g)]);
      CHECK(s.nodes[size_t(s.set_ptr[size_t(g)] + s.col[size_t(i)])] == states[i]);
    }
  CHECK(align::build_sets(state_ptr, states, 0).set_ptr.size() == 1);
  std::printf("build_sets ok\n");
}

void check_validator() {
  const int32_t rows[4] = {0, 10, 20, 35}, sp[4] = {0, 3, 7, 9};
  int32_t st[9] = {1, 2, 3, 4, 4, 4, 0, 7, 7};
  float self[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, next[9] = {0, 0, kNaN, 0, 0, 0, kInf, 0, -kInf};  // (next of a last state is never read)
  align::Why w;
  CHECK(align::check(rows, sp, st, self, next, 3, 8, 35, true, &w) == 0 && w == align::kOk);
  CHECK(align::check(rows, sp, st, nullptr, nullptr, 3, 8, 35, true, &w) == 0);
  CHECK(align::check(rows, sp, st, self, next, 3, 8, 34, true, &w) == -3 && w == align::kBadRows);   // past the context
  CHECK(align::check(rows, sp, st, self, next, 3, 7, 35, true, &w) == -3 && w == align::kBadNode);
  CHECK(align::check(nullptr, sp, st, self, next, 3, 8, 35, true, &w) == -1 && w == align::kBadRows);
  const int32_t flat[4] = {0, 10, 10, 35};
  CHECK(align::check(flat, sp, st, self, next, 3, 8, 35, true, &w) == -2 && w == align::kBadRows);   // a segment without rows
  const int32_t empty[4] = {0, 3, 3, 9};
  CHECK(align::check(rows, empty, st, self, next, 3, 8, 35, true, &w) == -2 && w == align::kBadStates);
  const int32_t off[4] = {1, 3, 7, 9};
  CHECK(align::check(rows, off, st, self, next, 3, 8, 35, true, &w) == -1);
  const int32_t tight[4] = {0, 2, 20, 35};
  CHECK(align::check(tight, sp, st, self, next, 3, 8, 35, true, &w) == -1 && w == align::kShort);     // T < S
  CHECK(align::check(tight, sp, st, self, next, 3, 8, 35, false, &w) == 0);
  next[4] = kInf;
  CHECK(align::check(rows, sp, st, self, next, 3, 8, 35, true, &w) == -2 && w == align::kBadTransition);
  next[4] = 0, self[8] = kNaN;
  CHECK(align::check(rows, sp, st, self, next, 3, 8, 35, true, &w) == -3 && w == align::kBadTransition);
  st[0] = -1;
  CHECK(align::check(rows, sp, st, nullptr, nullptr, 3, 8, 35, true, &w) == -1 && w == align::kBadNode);
  std::vector<int32_t> big(size_t(align::kMaxStates) + 1, 0);
  const int32_t one_rows[2] = {0, 20000}, ok_sp[2] = {0, align::kMaxStates}, long_sp[2] = {0, align::kMaxStates + 1};
  CHECK(align::check(one_rows, ok_sp, big.data(), nullptr, nullptr, 1, 8, 20000, true, &w) == 0);
  CHECK(align::check(one_rows, long_sp, big.data(), nullptr, nullptr, 1, 8, 20000, true, &w) == -1 && w == align::kBadStates);
  std::printf("validator ok\n");
}

void check_plan() {
  // every state has exactly one owner and one take bit, in both forms and at every K
  for (int K : {1, 2, 4, 8, 16}) {
    std::set<std::pair<int, int>> owners, bits;
    for (int j = 0; j < K * align::kWaveLanes; ++j) {
      int lane, slot;
      align::wave_owner(j, K, &lane, &slot);
      CHECK(lane >= 0 && lane < align::kWaveLanes && slot >= 0 && slot < K && lane * K + slot == j);
      CHECK(owners.insert({lane, slot}).second && bits.insert({slot, lane}).second);  // word `slot`, bit `lane`
    }
    CHECK(align::take_words_per_frame(align::kWave, K) == 2 * K);
  }
  {
    std::set<std::pair<int, int>> owners;
    for (int j = 0; j < align::kMaxStates; ++j) {
      int thread, round;
      align::wg_owner(j, &thread, &round);
      CHECK(thread >= 0 && thread < align::kWgThreads && round * align::kWgThreads + thread == j && owners.insert({thread, round}).second);
    }
  }
  const int edges[][2] = {{1, 1}, {64, 1}, {65, 2}, {128, 2}, {129, 4}, {256, 4}, {257, 8}, {512, 8}, {513, 16}, {1023, 16}, {1024, 16}};
  for (const auto &e : edges) CHECK(align::states_per_lane(e[0]) == e[1] && e[1] * align::kWaveLanes >= e[0]);
  CHECK(align::form_for(1024, 0) == align::kWave && align::form_for(1025, 0) == align::kWorkgroup && align::form_for(1, 2) == align::kWorkgroup);
  CHECK(align::form_for(40, 1) == align::kWave && align::form_for(align::kMaxStates, 1) == align::kWorkgroup);
  CHECK(align::take_words_per_frame(align::kWorkgroup, 1) == 2 && align::take_words_per_frame(align::kWorkgroup, 65) == 4);
  CHECK(align::frames_in_flight(1) == align::kFramesInFlight && align::frames_in_flight(16) == 2);

  std::mt19937 rng(3);
  for (int n_segs : {1, 2, 64, 65, 130})
    for (int mode : {0, 2})
      for (int mix : {0, 1}) {
        const size_t ns = static_cast<size_t>(n_segs);
        std::vector<int32_t> T(ns), ld(ns), sp(ns + 1, 0);
        std::vector<long long> off(ns);
        long long at = 0;
        for (int s = 0; s < n_segs; ++s) {
          const int S = (mix && s % 7 == 3) ? 1025 + int(rng() % 2000) : 1 + int(rng() % 1024);
          T[size_t(s)] = S + int(rng() % 300), ld[size_t(s)] = 1 + int(rng() % 50), off[size_t(s)] = at;
          at += static_cast<long long>(T[size_t(s)]) * ld[size_t(s)];
          sp[size_t(s) + 1] = sp[size_t(s)] + S;
        }
        const align::Plan p = align::plan(T.data(), off.data(), ld.data(), sp.data(), n_segs, mode);
        const int batches = (n_segs + align::kMaxSegs - 1) / align::kMaxSegs;
        if (mode == 2 || !mix) CHECK(int(p.launches.size()) == batches);
        else CHECK(int(p.launches.size()) <= 2 * batches && int(p.launches.size()) >= batches);
        std::vector<int> seen(size_t(n_segs), 0);
        long long scratch = 0;
        for (const align::Launch &l : p.launches) {
          CHECK(l.n_segs >= 1 && l.n_segs <= align::kMaxSegs);
          CHECK(l.lds_bytes <= 160 * 1024 - 8 * 1024);
          int lds_words = 0;
          for (int i = 0; i < l.n_segs; ++i) {
            const int s = l.total_off[i];
            CHECK(s >= 0 && s < n_segs && !seen[size_t(s)]++);
            const int S = sp[size_t(s) + 1] - sp[size_t(s)];
            CHECK(l.T[i] == T[size_t(s)] && l.S[i] == S && l.ld[i] == ld[size_t(s)] && l.state0[i] == sp[size_t(s)] && l.row_off[i] == off[size_t(s)]);
            long long before = 0;
            for (int q = 0; q < s; ++q) before += T[size_t(q)];
            CHECK(l.path_off[i] == before);
            CHECK(align::form_for(S, mode) == l.form);
            if (l.form == align::kWave) CHECK(l.K * align::kWaveLanes >= S && l.K <= 16);
            else CHECK(l.d_floats >= S && l.d_floats % 64 == 0 && l.d_floats <= align::kMaxStates);
            const long long words = static_cast<long long>(l.T[i]) * align::take_words_per_frame(align::Form(l.form), l.form == align::kWave ? l.K : S);
            if (words <= align::kBpLdsWords) {
              CHECK(l.bp_off[i] == -1);
              lds_words = std::max(lds_words, int(words));
            } else {
              CHECK(l.bp_off[i] == scratch && scratch % 2 == 0);  // one after the other, on 8-byte boundaries
              scratch += words;
            }
          }
          CHECK(l.lds_bytes == 4 * (lds_words + 2 * l.d_floats));
        }
        for (int v : seen) CHECK(v == 1);
        CHECK(p.scratch_words == scratch);
      }
  {  // the flagship shape: 64 utterances x 100 frames x 40 states is one launch, one state a lane, nothing in the scratch
    std::vector<int32_t> T(64, 100), ld(64, 40), sp(65);
    std::vector<long long> off(64);
    for (int s = 0; s <= 64; ++s) sp[size_t(s)] = 40 * s;
    for (int s = 0; s < 64; ++s) off[size_t(s)] = 4000ll * s;
    const align::Plan p = align::plan(T.data(), off.data(), ld.data(), sp.data(), 64, 0);
    CHECK(p.launches.size() == 1 && p.launches[0].K == 1 && p.scratch_words == 0 && p.launches[0].lds_bytes == 800);
  }
  {  // the cap: 2^27 frames of a 1024-state transcript are 2^32 words
    const int32_t T[1] = {1 << 27}, ld[1] = {1}, sp[2] = {0, 1024};
    const long long off[1] = {0};
    const align::Plan p = align::plan(T, off, ld, sp, 1, 0);
    CHECK(p.scratch_words == (1ll << 32) && p.scratch_words * 4 > align::kMaxScratchBytes);
    const int32_t T2[1] = {1 << 20};
    CHECK(align::plan(T2, off, ld, sp, 1, 0).scratch_words * 4 <= align::kMaxScratchBytes);
  }
  std::printf("plan ok\n");
}

}  // namespace

int main() {
  check_ref_against_brute_force();
  check_ties_and_nans();
  check_build_sets();
  check_validator();
  check_plan();
  std::printf("the band is not used: nothing to hold to the unbanded statement\n");
  std::printf("align ok\n");
  return 0;
}
