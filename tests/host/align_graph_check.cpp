// align_graph_check.cpp -- fdnn_align_graph.hpp (the candidate step, the final selection, the validator, the launch plan and
// the host restatement of alignment graphs), alone and under the sanitizers (tests/test_align_graph_host.py builds and runs
// this).  Must be built with -ffp-contract=off and WITHOUT a flush-to-zero or fast-math flag.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "fdnn_align_graph.hpp"

using namespace fdnn;
using align::bits_of;
using align::float_of;
namespace ag = fdnn::align_graph;

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

struct Graph {
  int T, S;
  std::vector<float> e;  // [T][S] scores
  std::vector<int32_t> ptr, src, col;
  std::vector<float> lp, start, fin;  // start / fin empty: the defaults
};

struct Result {
  std::vector<int32_t> path;
  uint32_t total;
};

Result run_ref(const Graph &g) {
  Result r{std::vector<int32_t>(size_t(g.T), 77), 0};
  ag::ref(reinterpret_cast<const uint32_t *>(g.e.data()), g.T, g.S, g.col.data(), nullptr, g.S, nullptr, 0, 0.0f, align::kScores, g.ptr.data(), g.src.data(),
          g.lp.data(), g.start.empty() ? nullptr : g.start.data(), g.fin.empty() ? nullptr : g.fin.data(), r.path.data(), &r.total);
  return r;
}

// a state sequence's score in the recursion's own order: ((start + e) ... (best arc p[t-1] -> p[t] added, then e) ...) + final;
// -inf where a step has no arc.  Parallel arcs: the best of them (rounding is monotone)
float seq_score(const Graph &g, const std::vector<int32_t> &p) {
  float acc = ag::start_of(g.start.empty() ? nullptr : g.start.data(), p[0]) + g.e[size_t(p[0])];
  for (int t = 1; t < g.T; ++t) {
    const int j = p[size_t(t)];
    float best = -kInf;
    for (int a = g.ptr[size_t(j)]; a < g.ptr[size_t(j) + 1]; ++a)
      if (g.src[size_t(a)] == p[size_t(t) - 1] && acc + g.lp[size_t(a)] > best) best = acc + g.lp[size_t(a)];
    acc = best + g.e[size_t(t) * g.S + j];
  }
  return acc + ag::final_of(g.fin.empty() ? nullptr : g.fin.data(), p[size_t(g.T) - 1], g.S);
}

// every state sequence: the best score (never a NaN: a NaN is not above anything)
float brute(const Graph &g, long long *count) {
  float best = -kInf;
  std::vector<int32_t> p(size_t(g.T), 0);
  long long n = 1;
  for (int t = 0; t < g.T; ++t) n *= g.S;
  *count = n;
  for (long long code = 0; code < n; ++code) {
    long long c = code;
    for (int t = 0; t < g.T; ++t) p[size_t(t)] = int32_t(c % g.S), c /= g.S;
    const float s = seq_score(g, p);
    if (s > best) best = s;
  }
  return best;
}

// in-degree 0 .. 3 from any state (self-loops, forward, skip and backward arcs, parallel arcs), several start and final states
Graph random_graph(int T, int S, std::mt19937 &rng, bool integers) {
  Graph g{T, S, std::vector<float>(size_t(T) * S), {0}, {}, std::vector<int32_t>(size_t(S)), {}, std::vector<float>(size_t(S)), std::vector<float>(size_t(S))};
  std::normal_distribution<float> n(0.0f, 1.0f);
  std::uniform_real_distribution<float> u(0.05f, 0.95f);
  std::uniform_int_distribution<int> k(-3, 3), deg(0, 3), any(0, S - 1), coin(0, 1);
  for (float &v : g.e) v = integers ? float(k(rng)) : 3.0f * n(rng) - 5.0f;
  for (int j = 0; j < S; ++j) {
    g.col[size_t(j)] = j;
    for (int d = deg(rng); d > 0; --d) g.src.push_back(any(rng)), g.lp.push_back(integers ? float(k(rng)) : std::log(u(rng)));
    g.ptr.push_back(int32_t(g.src.size()));
    g.start[size_t(j)] = coin(rng) ? (integers ? 0.0f : std::log(u(rng))) : -kInf;
    g.fin[size_t(j)] = coin(rng) ? (integers ? 0.0f : std::log(u(rng))) : -kInf;
  }
  g.start[size_t(any(rng))] = 0.0f, g.fin[size_t(any(rng))] = 0.0f;
  return g;
}

void check_ref_against_brute_force() {
  std::mt19937 rng(1);
  long long cases = 0, seqs = 0, no_path = 0, backward = 0, no_arcs = 0;
  for (int T = 1; T <= 5; ++T)
    for (int S = 1; S <= 4; ++S)
      for (int rep = 0; rep < 40; ++rep) {
        const Graph g = random_graph(T, S, rng, rep >= 20);
        const Result r = run_ref(g);
        long long n = 0;
        const float best = brute(g, &n);
        CHECK(r.total == bits_of(best));  // rounded addition is monotone: the best sequentially rounded sum is the total
        if (align::finite_bits(r.total)) {
          for (int t = 0; t < T; ++t) CHECK(r.path[size_t(t)] >= 0 && r.path[size_t(t)] < S);
          CHECK(bits_of(seq_score(g, r.path)) == r.total);  // the returned path has the returned score
        } else {
          CHECK(best == -kInf);
          for (int t = 0; t < T; ++t) CHECK(r.path[size_t(t)] == -1);
          ++no_path;
        }
        for (int j = 0; j < S; ++j) {
          no_arcs += g.ptr[size_t(j)] == g.ptr[size_t(j) + 1];
          for (int a = g.ptr[size_t(j)]; a < g.ptr[size_t(j) + 1]; ++a) backward += g.src[size_t(a)] > j;
        }
        ++cases, seqs += n;
      }
  CHECK(no_path > 0 && no_path < cases / 2 && backward > 100 && no_arcs > 100);
  std::printf("ref against brute force: %lld graphs, %lld sequences, %lld without a path, %lld backward arcs, %lld states without arcs\n", cases, seqs,
              no_path, backward, no_arcs);
}

Graph reversed(const Graph &g) {
  Graph r = g;
  for (int j = 0; j < g.S; ++j)
    for (int a = g.ptr[size_t(j)], b = g.ptr[size_t(j) + 1] - 1; a < b; ++a, --b) std::swap(r.src[size_t(a)], r.src[size_t(b)]), std::swap(r.lp[size_t(a)], r.lp[size_t(b)]);
  return r;
}

void check_ties_nans_and_no_path() {
  // two start states into one final state over equal arcs: the earlier arc wins, reversed the other, the total the same
  Graph g{2, 3, std::vector<float>(6, 0.0f), {0, 0, 0, 2}, {0, 1}, {0, 1, 2}, {0.0f, 0.0f}, {0.0f, 0.0f, -kInf}, {}};
  Result a = run_ref(g), b = run_ref(reversed(g));
  CHECK(a.total == 0 && b.total == 0 && a.path == (std::vector<int32_t>{0, 2}) && b.path == (std::vector<int32_t>{1, 2}));
  // equal final states: the lowest
  Graph f{1, 3, {1.0f, 1.0f, 1.0f}, {0, 0, 0, 0}, {}, {0, 1, 2}, {}, {-kInf, 0.0f, 0.0f}, {-kInf, 0.0f, 0.0f}};
  a = run_ref(f);
  CHECK(a.total == bits_of(1.0f) && a.path == (std::vector<int32_t>{1}));
  // integer scores: reversing every state's arc order keeps the total
  std::mt19937 rng(3);
  long long differ = 0;
  for (int rep = 0; rep < 200; ++rep) {
    Graph r = random_graph(5, 4, rng, true);
    for (float &v : r.lp) v = 0.0f;
    a = run_ref(r), b = run_ref(reversed(r));
    CHECK(a.total == b.total);
    differ += a.path != b.path;
  }
  CHECK(differ > 10);
  // a NaN candidate is never taken: state 1's emission is a NaN in frame 1, the path goes round it over the worse state 2
  Graph n{3, 4, {0, 0, 0, 0, /**/ 0, kNaN, -9.0f, 0, /**/ 0, 0, 0, 0}, {0, 0, 1, 2, 4}, {0, 0, 1, 2}, {0, 1, 2, 3}, {0, 0, 0, 0}, {}, {}};
  a = run_ref(n);
  CHECK(a.total == bits_of(-9.0f) && a.path == (std::vector<int32_t>{0, 2, 3}));
  n.e[6] = kNaN;  // ... and with both ways a NaN there is no path: -inf, not a NaN
  a = run_ref(n);
  CHECK(a.total == align::kMinusInf && a.path == (std::vector<int32_t>{-1, -1, -1}));
  // a NaN start, a NaN final, a source outside [0, S): never taken
  Graph s{2, 2, {0, 0, 0, 0}, {0, 1, 3}, {0, 0, 7}, {0, 1}, {0, 1.0f, 5.0f}, {0.0f, kNaN}, {kNaN, 0.0f}};
  a = run_ref(s);
  CHECK(a.total == bits_of(1.0f) && a.path == (std::vector<int32_t>{0, 1}));
  s.src[2] = -1;
  CHECK(run_ref(s).total == bits_of(1.0f));
  // +inf: -1 everywhere
  Graph p{2, 1, {kInf, 0}, {0, 1}, {0}, {0}, {0}, {}, {}};
  a = run_ref(p);
  CHECK(a.total == bits_of(kInf) && a.path == (std::vector<int32_t>{-1, -1}));
  // a final state that cannot be reached; a state without arcs is reachable at t = 0 only
  Graph u{3, 2, std::vector<float>(6, 0.0f), {0, 1, 1}, {0}, {0, 1}, {0}, {}, {}};
  a = run_ref(u);
  CHECK(a.total == align::kMinusInf && a.path == (std::vector<int32_t>{-1, -1, -1}));
  u.T = 1, u.start = {-kInf, 0.0f};
  a = run_ref(u);
  CHECK(a.total == 0 && a.path == (std::vector<int32_t>{1}));
  std::printf("ties, NaNs and missing paths ok (%lld of 200 integer graphs change their path with the arc order)\n", differ);
}

// the chain as a graph: state j's arcs are (j with self_lp[j], then j - 1 with next_lp[j - 1])
Graph chain(int T, int S, const std::vector<float> &e, const std::vector<float> &self, const std::vector<float> &next) {
  Graph g{T, S, e, {0}, {}, std::vector<int32_t>(size_t(S)), {}, {}, {}};
  for (int j = 0; j < S; ++j) {
    g.col[size_t(j)] = j;
    g.src.push_back(j), g.lp.push_back(self[size_t(j)]);
    if (j) g.src.push_back(j - 1), g.lp.push_back(next[size_t(j) - 1]);
    g.ptr.push_back(int32_t(g.src.size()));
  }
  return g;
}

void check_chain_equivalence() {
  std::mt19937 rng(1);
  std::normal_distribution<float> n(0.0f, 1.0f);
  std::uniform_real_distribution<float> u(0.05f, 0.95f);
  std::uniform_int_distribution<int> k(-3, 3), ten(0, 9);
  long long cases = 0, shorts = 0, both_inf = 0;
  for (int T = 1; T <= 10; ++T)
    for (int S = 1; S <= 6; ++S)
      for (int rep = 0; rep < 12; ++rep) {
        const bool integers = rep >= 4;  // planted ties
        std::vector<float> e(size_t(T) * size_t(S)), self(e.size() / size_t(T)), next(self.size());
        for (float &v : e) v = integers ? float(k(rng)) : 3.0f * n(rng) - 5.0f;
        if (rep >= 8)
          for (float &v : e)
            if (ten(rng) == 0) v = -kInf, ++both_inf;  // a state that cannot be held: stay and move both -inf behind it
        for (int j = 0; j < S; ++j) {
          const float a = u(rng);
          self[size_t(j)] = integers ? 0.0f : std::log(a), next[size_t(j)] = integers ? 0.0f : std::log(1.0f - a);
        }
        const Graph g = chain(T, S, e, self, next);
        const Result r = run_ref(g);
        Result want{std::vector<int32_t>(size_t(T), 77), 0};
        align::ref(reinterpret_cast<const uint32_t *>(e.data()), T, S, g.col.data(), nullptr, S, nullptr, 0, 0.0f, align::kScores, self.data(), next.data(),
                   want.path.data(), &want.total);
        CHECK(r.total == want.total && r.path == want.path);  // T < S included: -inf and -1 everywhere (stay -inf, move finite on the way up)
        shorts += T < S, ++cases;
      }
  CHECK(shorts > 0 && both_inf > 0);
  std::printf("chain graphs against align::ref: %lld cases, %lld with T < S, %lld -inf emissions planted\n", cases, shorts, both_inf);
}

void check_validator() {
  const int32_t rows[3] = {0, 4, 9}, sp[3] = {0, 2, 5}, st[5] = {3, 3, 0, 7, 1}, ap[6] = {0, 1, 3, 4, 4, 6}, src[6] = {0, 1, 0, 0, 2, 1};
  const float lp[6] = {0, -1, -2, 0, 0.5f, 0}, start[5] = {0, -kInf, -kInf, 0, 0}, fin[5] = {-kInf, 0, 0, -kInf, 0};
  ag::Tables t;
  t.seg_rows = rows, t.state_ptr = sp, t.states = st, t.arc_ptr = ap, t.arc_src = src, t.arc_lp = lp, t.start_lp = start, t.final_lp = fin, t.n_segs = 2;
  ag::Why w;
  CHECK(ag::check(t, 8, 9, &w) == 0 && w == ag::kOk);
  ag::Tables d = t;
  d.start_lp = d.final_lp = nullptr;
  CHECK(ag::check(d, 8, 9, &w) == 0);
  d.n_segs = 0, d.seg_rows = nullptr;
  CHECK(ag::check(d, 8, 9, &w) == 0);
  auto bad = [&](const ag::Tables &x, int out_dim, int ctx_rows, int seg, ag::Why why) {
    ag::Why got;
    CHECK(ag::check(x, out_dim, ctx_rows, &got) == -(seg + 1) && got == why && ag::why_text(got)[0] != 0);
  };
  bad(t, 8, 8, 1, ag::kBadRows);   // past the context
  bad(t, 7, 9, 1, ag::kBadNode);   // node 7
  { const int32_t r2[3] = {0, 4, 4}; d = t, d.seg_rows = r2; bad(d, 8, 9, 1, ag::kBadRows); }
  { d = t, d.seg_rows = nullptr; bad(d, 8, 9, 0, ag::kBadRows); }
  { const int32_t s2[3] = {0, 0, 5}; d = t, d.state_ptr = s2; bad(d, 8, 9, 0, ag::kBadStates); }
  { d = t, d.arc_ptr = nullptr; bad(d, 8, 9, 0, ag::kBadArcPtr); }
  { const int32_t a2[6] = {1, 1, 3, 4, 4, 6}; d = t, d.arc_ptr = a2; bad(d, 8, 9, 0, ag::kBadArcPtr); }
  { const int32_t a2[6] = {0, 1, 3, 4, 3, 6}; d = t, d.arc_ptr = a2; bad(d, 8, 9, 1, ag::kBadArcPtr); }
  { const int32_t c2[6] = {0, 2, 0, 0, 2, 1}; d = t, d.arc_src = c2; bad(d, 8, 9, 0, ag::kBadSource); }  // S = 2
  { const int32_t c2[6] = {0, 1, 0, 0, -1, 1}; d = t, d.arc_src = c2; bad(d, 8, 9, 1, ag::kBadSource); }
  for (float v : {kNaN, kInf, -kInf}) { float l2[6] = {0, -1, -2, 0, v, 0}; d = t, d.arc_lp = l2; bad(d, 8, 9, 1, ag::kBadArcScore); }
  for (float v : {kNaN, kInf}) {
    float s2[5] = {0, -kInf, v, 0, 0};
    d = t, d.start_lp = s2, bad(d, 8, 9, 1, ag::kBadStartFinal);
    d = t, d.final_lp = s2, bad(d, 8, 9, 1, ag::kBadStartFinal);
  }
  { const float s2[5] = {-kInf, -kInf, 0, 0, 0}; d = t, d.start_lp = s2; bad(d, 8, 9, 0, ag::kNoStart); }
  { const float f2[5] = {-kInf, 0, -kInf, -kInf, -kInf}; d = t, d.final_lp = f2; bad(d, 8, 9, 1, ag::kNoFinal); }
  {  // one arc above the most: a single state with kMaxArcs + 1 self-loops
    const int32_t r1[2] = {0, 1}, s1[2] = {0, 1}, n1[1] = {0}, a1[2] = {0, ag::kMaxArcs + 1};
    const std::vector<int32_t> many(size_t(ag::kMaxArcs) + 1, 0);
    const std::vector<float> zeros(size_t(ag::kMaxArcs) + 1, 0.0f);
    ag::Tables m;
    m.seg_rows = r1, m.state_ptr = s1, m.states = n1, m.arc_ptr = a1, m.arc_src = many.data(), m.arc_lp = zeros.data(), m.n_segs = 1;
    bad(m, 8, 9, 0, ag::kTooManyArcs);
    const int32_t a0[2] = {0, ag::kMaxArcs};
    m.arc_ptr = a0;
    CHECK(ag::check(m, 8, 9, &w) == 0);
  }
  std::printf("validator ok\n");
}

void check_plan() {
  CHECK(ag::kWaveStates == 256 && ag::kWaveRuleStates == 64 && ag::form_for(64, 0) == ag::kWave && ag::form_for(65, 0) == ag::kWorkgroup);
  CHECK(ag::form_for(256, 1) == ag::kWave && ag::form_for(257, 1) == ag::kWorkgroup && ag::form_for(5, 2) == ag::kWorkgroup);
  CHECK(ag::wave_slots(1) == 1 && ag::wave_slots(64) == 1 && ag::wave_slots(65) == 2 && ag::wave_slots(128) == 2 && ag::wave_slots(129) == 4 && ag::wave_slots(256) == 4);
  for (int K : {1, 2, 4}) CHECK(ag::frames_in_flight(K) * K * ag::kWaveLanes == ag::kEmissionRing);
  // segments per launch; forms; offsets
  const int n = 130;
  std::vector<int32_t> T(n), ld(n, 3), sp(n + 1, 0), ap;
  std::vector<long long> off(n, 0);
  for (int s = 0; s < n; ++s) T[size_t(s)] = 2 + s % 3, sp[size_t(s) + 1] = sp[size_t(s)] + (s % 7 == 3 ? 1500 : 10 + s);
  ap.assign(size_t(sp[n]) + 1, 0);
  for (int i = 1; i <= sp[n]; ++i) ap[size_t(i)] = ap[size_t(i) - 1] + 2;
  ag::Plan p = ag::plan(T.data(), off.data(), ld.data(), sp.data(), ap.data(), n, 0);
  CHECK(p.launches.size() == 4);  // 64 + 64 + 2 segments; the rule's wave form (up to 64 states) occurs among the first 64 only
  CHECK(ag::plan(T.data(), off.data(), ld.data(), sp.data(), ap.data(), n, 1).launches.size() == 6);  // forced: both forms among each
  std::vector<int> seen(n, 0);
  for (const ag::Launch &l : p.launches) {
    CHECK(l.n_segs >= 1 && l.n_segs <= ag::kMaxSegs && l.d_floats % 64 == 0);
    int bpw = 0;
    for (int i = 0; i < l.n_segs; ++i) {
      const int s = l.total_off[i];
      CHECK(seen[size_t(s)]++ == 0 && l.S[i] == sp[size_t(s) + 1] - sp[size_t(s)] && l.T[i] == T[size_t(s)] && l.state0[i] == sp[size_t(s)]);
      CHECK(ag::form_for(l.S[i], 0) == l.form && l.S[i] <= l.d_floats && l.arc0[i] == 2 * sp[size_t(s)] && l.n_arcs[i] == 2 * l.S[i]);
      int po = 0;
      for (int q = 0; q < s; ++q) po += T[size_t(q)];
      CHECK(l.path_off[i] == po);
      if (l.bp_off[i] < 0) bpw = std::max<int>(bpw, int(ag::bp_words(l.T[i], l.S[i])));
      if (l.form == ag::kWave) CHECK(l.n_arcs[i] <= l.arc_cap && l.arc_cap % 2 == 0 && l.S[i] <= l.K * ag::kWaveLanes && l.d_floats == l.K * ag::kWaveLanes);
    }
    CHECK(l.bp_words == bpw && bpw <= ag::kBpLdsWords);
    CHECK(l.lds_bytes == 4 * (l.form == ag::kWave ? ag::wave_lds_words(l.d_floats, l.arc_cap, l.bp_words) : ag::wg_lds_words(l.d_floats, l.bp_words)));
    CHECK(l.lds_bytes <= (l.form == ag::kWave ? 64 * 1024 : 160 * 1024));
  }
  for (int s = 0; s < n; ++s) CHECK(seen[size_t(s)] == 1);
  CHECK(p.scratch_words == 0);
  p = ag::plan(T.data(), off.data(), ld.data(), sp.data(), ap.data(), n, 2);
  CHECK(p.launches.size() == 3);
  // the largest LDS of either form is inside what a launch can get
  CHECK(4 * ag::wave_lds_words(ag::kWaveStates, ag::kArcLdsArcs, ag::kBpLdsWords) <= 64 * 1024);
  CHECK(4 * ag::wg_lds_words(ag::kMaxStates, ag::kBpLdsWords) <= 160 * 1024);
  // back-pointers: at the LDS cap, one word above it, the scratch offsets and the cap of a call
  {
    const int32_t T3[3] = {128, 4097, 130}, ld3[3] = {1, 1, 1}, sp3[4] = {0, 64, 66, 129};
    const long long off3[3] = {0, 0, 0};
    ag::Plan q = ag::plan(T3, off3, ld3, sp3, nullptr, 3, 0);
    CHECK(ag::bp_words(128, 64) == ag::kBpLdsWords && ag::bp_words(4097, 2) == ag::kBpLdsWords + 1 && ag::bp_words(130, 63) == ag::kBpLdsWords - 1);
    CHECK(q.launches.size() == 1 && q.launches[0].bp_off[0] == -1 && q.launches[0].bp_off[1] == 0 && q.launches[0].bp_off[2] == -1);
    CHECK(q.scratch_words == ag::kBpLdsWords + 1 && q.launches[0].bp_words == ag::kBpLdsWords && q.launches[0].arc_cap == 0);
    const int32_t Tb[1] = {40000}, spb[2] = {0, ag::kMaxStates};
    q = ag::plan(Tb, off3, ld3, spb, nullptr, 1, 0);
    CHECK(q.scratch_words == 40000ll * ag::kMaxStates / 2 && q.scratch_words * 4 > ag::kMaxScratchBytes);
  }
  // the arc-staging cap at its edge: one below, at, one above
  {
    const int32_t T3[3] = {2, 2, 2}, ld3[3] = {1, 1, 1}, sp3[4] = {0, 1, 2, 3}, ap3[4] = {0, ag::kArcLdsArcs - 1, 2 * ag::kArcLdsArcs - 1, 3 * ag::kArcLdsArcs};
    const long long off3[3] = {0, 0, 0};
    const ag::Plan q = ag::plan(T3, off3, ld3, sp3, ap3, 3, 0);
    CHECK(q.launches.size() == 1 && q.launches[0].arc_cap == ag::kArcLdsArcs && q.launches[0].n_arcs[2] == ag::kArcLdsArcs + 1);
    CHECK(ag::arcs_staged(ag::kWave, ag::kArcLdsArcs) && !ag::arcs_staged(ag::kWave, ag::kArcLdsArcs + 1) && !ag::arcs_staged(ag::kWorkgroup, 1));
    const ag::Plan w = ag::plan(T3, off3, ld3, sp3, ap3, 3, 2);
    CHECK(w.launches.size() == 1 && w.launches[0].arc_cap == 0);
  }
  std::printf("plan ok\n");
}

}  // namespace

int main() {
  check_ref_against_brute_force();
  check_ties_nans_and_no_path();
  check_chain_equivalence();
  check_validator();
  check_plan();
  std::printf("align graph ok\n");
  return 0;
}
