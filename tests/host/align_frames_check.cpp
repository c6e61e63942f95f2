// align_frames_check.cpp -- fdnn_align_frames.hpp (the frames form of the best path over alignment graphs: the restatement, the
// contract's consequences (a) to (f) and the tie rule), alone and under the sanitizers (tests/test_align_frames_host.py builds
// and runs this).  Must be built with -ffp-contract=off and WITHOUT a flush-to-zero or fast-math flag.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fdnn_align_frames.hpp"

using namespace fdnn;
using align::bits_of;
using align::float_of;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

namespace {

struct Graph {
  int S;
  std::vector<float> e;  // [T][S] scores
  std::vector<int32_t> ptr, src, col;
  std::vector<float> lp, start, fin;
};

struct Result {
  std::vector<uint32_t> best, d;
  std::vector<int32_t> end, begin, b;
  Result(int n, int S) : best(size_t(n), 0x12345678u), d(size_t(S)), end(size_t(n), -7), begin(size_t(n), -7), b(size_t(S)) {}
};

// rows [t0, t1) of g, numbered from base + t0
Result run(const Graph &g, bool free_start, int t0, int t1, int base = 0, const Result *in = nullptr) {
  Result r(t1 - t0, g.S);
  align_frames::ref(reinterpret_cast<const uint32_t *>(g.e.data()) + size_t(t0) * g.S, t1 - t0, g.S, g.col.data(), nullptr, g.S, nullptr, 0, 0.0f,
                    align::kScores, g.ptr.data(), g.src.data(), g.lp.data(), g.start.data(), g.fin.data(), free_start, base + t0, in ? in->d.data() : nullptr,
                    in ? in->b.data() : nullptr, r.d.data(), r.b.data(), r.best.data(), r.end.data(), r.begin.data());
  return r;
}

// align_graph::ref, anchored, on rows [t0, t1) -> the total's bits and the path's last state
uint32_t graph_ref(const Graph &g, int t0, int t1, int32_t *last) {
  std::vector<int32_t> path(size_t(t1 - t0));
  uint32_t total;
  align_graph::ref(reinterpret_cast<const uint32_t *>(g.e.data()) + size_t(t0) * g.S, t1 - t0, g.S, g.col.data(), nullptr, g.S, nullptr, 0, 0.0f,
                   align::kScores, g.ptr.data(), g.src.data(), g.lp.data(), g.start.data(), g.fin.data(), path.data(), &total);
  *last = path.back();
  return total;
}

// A keyword: a chain entered in state 0 and left in state S - 1, state j from j (a loop that costs `loop`), j - 1, j - 2 (a skip that costs
// `skip`) and one state drawn from all (backward and parallel arcs, dearer than a loop).  With loops dearer than a frame's emission makes up
// for, the best path ending at t is short, so it begins late.  wide: besides, by a coin each, any state is a start and a final state at ln U
Graph keyword(int T, int S, float loop, float skip, bool wide, std::mt19937 &rng) {
  Graph g{S, std::vector<float>(size_t(T) * S), {0}, {}, std::vector<int32_t>(size_t(S)), {}, std::vector<float>(size_t(S), -INFINITY), std::vector<float>(size_t(S), -INFINITY)};
  std::normal_distribution<float> n(0.0f, 1.0f);
  std::uniform_real_distribution<float> u(0.05f, 0.95f);
  std::uniform_int_distribution<int> any(0, S - 1), coin(0, 1);
  for (float &v : g.e) v = n(rng) - 1.0f;
  for (int j = 0; j < S; ++j) {
    g.col[size_t(j)] = j;
    g.src.push_back(j), g.lp.push_back(loop);
    if (j >= 1) g.src.push_back(j - 1), g.lp.push_back(-0.1f);
    if (j >= 2) g.src.push_back(j - 2), g.lp.push_back(skip);
    g.src.push_back(any(rng)), g.lp.push_back(loop + std::log(u(rng)));
    if (wide && j == 0 && S > 1 && coin(rng)) g.src.clear(), g.lp.clear();  // the first state without arcs: dead after frame 0 unless the start is free
    g.ptr.push_back(int32_t(g.src.size()));
    if (wide && coin(rng)) g.start[size_t(j)] = std::log(u(rng));
    if (wide && coin(rng)) g.fin[size_t(j)] = std::log(u(rng));
  }
  g.start[0] = 0.0f, g.fin[size_t(S) - 1] = 0.0f;
  return g;
}

// the contract's pseudo-code on the first T rows, transcribed with + and > alone
Result literal(const Graph &g, int T, bool free_start, int base) {
  const int S = g.S;
  Result r(T, S);
  std::vector<float> d = g.start, nd = d;  // (sized S)
  std::vector<int32_t> b = g.col, nb = b;
  for (int t = 0; t < T; ++t) {
    float sel = -INFINITY;
    int end = -1;
    for (int j = 0; j < S; ++j) {
      float best = -INFINITY;
      int32_t bg = -1;
      if (t == 0) {
        best = g.start[size_t(j)], bg = g.start[size_t(j)] > -INFINITY ? base : -1;
      } else {
        int from = -1;
        for (int a = g.ptr[size_t(j)]; a < g.ptr[size_t(j) + 1]; ++a) {
          const float cand = d[size_t(g.src[size_t(a)])] + g.lp[size_t(a)];
          if (cand > best) best = cand, from = g.src[size_t(a)];
        }
        bg = from >= 0 ? b[size_t(from)] : -1;
        if (free_start && g.start[size_t(j)] > best) best = g.start[size_t(j)], bg = base + t;
      }
      nd[size_t(j)] = best + g.e[size_t(t) * S + size_t(g.col[size_t(j)])], nb[size_t(j)] = bg;
      if (nd[size_t(j)] + g.fin[size_t(j)] > sel) sel = nd[size_t(j)] + g.fin[size_t(j)], end = j;
    }
    d = nd, b = nb;
    r.best[size_t(t)] = bits_of(sel), r.end[size_t(t)] = end, r.begin[size_t(t)] = end >= 0 ? b[size_t(end)] : -1;
  }
  for (int j = 0; j < S; ++j) r.d[size_t(j)] = bits_of(d[size_t(j)]), r.b[size_t(j)] = b[size_t(j)];
  return r;
}

// float64 over ALL state sequences that begin at a frame in [b0, b1] and end at t -> the best; *big: the largest finite partial sum
double brute(const Graph &g, int b0, int b1, int t, double *big) {
  double best = -INFINITY;
  auto seen = [&](double v) { return *big = std::isfinite(v) ? std::max(*big, std::fabs(v)) : *big, v; };
  for (int b = b0; b <= b1; ++b) {
    const int L = t - b + 1;
    std::vector<int> seq(size_t(L), 0);
    for (bool more = true; more;) {
      double v = seen(double(g.start[size_t(seq[0])]) + g.e[size_t(b) * g.S + size_t(seq[0])]);
      for (int i = 1; i < L && v > -INFINITY; ++i) {
        double arc = -INFINITY;  // (parallel arcs: the best of them)
        for (int a = g.ptr[size_t(seq[size_t(i)])]; a < g.ptr[size_t(seq[size_t(i)]) + 1]; ++a)
          if (g.src[size_t(a)] == seq[size_t(i) - 1]) arc = std::max(arc, double(g.lp[size_t(a)]));
        v = seen(seen(v + arc) + g.e[size_t(b + i) * g.S + size_t(seq[size_t(i)])]);
      }
      best = std::max(best, seen(v + g.fin[size_t(seq.back())]));
      more = false;  // the next sequence, an odometer
      for (int i = 0; i < L && !more; ++i) more = ++seq[size_t(i)] < g.S || (seq[size_t(i)] = 0, false);
    }
  }
  return best;
}

// The restatement against the literal transcription, (f) against float64 over all state sequences (frames 0 .. 4 of the graphs of
// S <= 4), and (a) to (e).  Every fixture has T >= S + 2 rows: a path that begins after the first frame can still reach the last state
void check_the_contract() {
  std::mt19937 rng(1);
  long long cuts = 0, above = 0, frames = 0, late = 0, brutes = 0, finite = 0;
  for (int S = 1; S <= 5; ++S)
    for (int T = S + 2; T <= 12; T += 2)
      for (int rep = 0; rep < 8; ++rep) {
        Graph g = keyword(T, S, -1.5f - 0.25f * rep, -0.3f, rep % 2 == 0, rng);
        const int base = 1000 * rep - 3000;
        const Result anchored = run(g, false, 0, T, base), fre = run(g, true, 0, T, base);
        CHECK(fre.best != anchored.best);  // not blind: the free and the anchored frame_best differ in a frame of EVERY fixture
        for (int f = 0; f < 4; ++f) {  // (one row: the start row is the last)
          const Result r = run(g, f % 2 != 0, 0, f < 2 ? T : 1, base), lit = literal(g, f < 2 ? T : 1, f % 2 != 0, base);
          CHECK(r.best == lit.best && r.end == lit.end && r.begin == lit.begin && r.d == lit.d && r.b == lit.b);
        }
        for (int t = 0; t < T; ++t, ++frames) {
          for (int f = 0; f < 2 && S <= 4 && t < 5; ++f, ++brutes) {  // (f)
            double big = 0.0;
            const double want = brute(g, 0, f ? t : 0, t, &big), got = float_of((f ? fre : anchored).best[size_t(t)]);
            CHECK(std::isfinite(want) ? std::fabs(got - want) <= align_frames::best_bound(t + 1, big * 1.000001) : got == want);
            finite += std::isfinite(want);
          }
          int32_t last;
          const uint32_t total = graph_ref(g, 0, t + 1, &last);  // (a) every prefix against align_graph::ref
          CHECK(anchored.best[size_t(t)] == total);
          if (align::finite_bits(total)) CHECK(anchored.end[size_t(t)] == last && anchored.begin[size_t(t)] == base);
          CHECK(float_of(fre.best[size_t(t)]) >= float_of(anchored.best[size_t(t)]));  // (d) free >= anchored, as floats
          above += float_of(fre.best[size_t(t)]) > float_of(anchored.best[size_t(t)]);
          if (align::finite_bits(fre.best[size_t(t)])) {  // (e) the begin frame is true
            const int b = fre.begin[size_t(t)] - base;
            CHECK(b >= 0 && b <= t && graph_ref(g, b, t + 1, &last) == fre.best[size_t(t)] && last == fre.end[size_t(t)]);
            late += b > 0;
          }
        }
        // (b) every cut, either start, and (c); then both again with a NaN, +inf or -inf in the emissions, a column out of
        // range (a NaN emission) and, uncut, a NaN, +inf or -inf in d_in
        for (int pass = 0; pass < 2; ++pass) {
          for (int f = 0; f < 2; ++f) {
            Result in(0, S);
            for (int j = 0; j < S; ++j) in.d[size_t(j)] = bits_of(j == rep % S ? (rep % 3 == 0 ? NAN : (rep % 3 == 1 ? INFINITY : -INFINITY)) : -1.0f), in.b[size_t(j)] = 42;
            const Result whole = run(g, f != 0, 0, T, base), carried = run(g, f != 0, 0, T, base, &in);
            for (int t = 0; t < T; ++t) CHECK(!std::isnan(float_of(whole.best[size_t(t)])) && !std::isnan(float_of(carried.best[size_t(t)])));  // (c)
            for (int c = 1; c < T; ++c, ++cuts) {
              const Result a = run(g, f != 0, 0, c, base), b = run(g, f != 0, c, T, base, &a);
              for (int t = 0; t < T; ++t) {
                const Result &h = t < c ? a : b;
                const size_t i = size_t(t < c ? t : t - c);
                CHECK(h.best[i] == whole.best[size_t(t)] && h.end[i] == whole.end[size_t(t)] && h.begin[i] == whole.begin[size_t(t)]);
              }
              CHECK(b.b == whole.b);
              for (size_t j = 0; j < size_t(S); ++j) CHECK(std::isnan(float_of(whole.d[j])) ? std::isnan(float_of(b.d[j])) : b.d[j] == whole.d[j]);  // (the NaN rule)
            }
          }
          g.e[size_t(rep) % g.e.size()] = rep % 3 == 0 ? NAN : (rep % 3 == 1 ? INFINITY : -INFINITY);
          g.col[size_t(rep % S)] = rep % 5 == 0 ? 9 : g.col[size_t(rep % S)];
        }
      }
  CHECK(above > 0 && finite * 2 > brutes);
  CHECK(late * 2 >= frames);  // not blind: in at least half of the (fixture, frame) pairs frame_best is finite and the path begins after the first frame
  std::printf("contract ok: the literal transcription's bytes; brute force within bound (f) in %lld of %lld frames, the rest -inf;\n(a), (d) and (e) against "
              "align_graph::ref in %lld frames, free above anchored in %lld, a finite late begin in %lld;\n(b) and (c) at %lld cuts, half of them with non-finite input\n",
              finite, brutes, frames, above, late, cuts);
}

}  // namespace

int main() {
  check_the_contract();
  std::mt19937 rng(3);  // the tie rule: a start equal to the running best keeps the earlier begin; one above it restarts
  Graph g = keyword(3, 1, 0.0f, 0.0f, false, rng);  // one state with a free loop (and a dearer one); start = final = 0
  g.e = {-1.0f, 1.0f, -2.0f};                       // d[0] = -1; frame 1: best = -1 < start 0: restart; d[1] = 1; frame 2: best = 1 > 0: keeps 1
  CHECK(run(g, true, 0, 3, 10).begin == (std::vector<int32_t>{10, 11, 11}));
  g.e = {0.0f, 0.0f, 0.0f};  // every frame a tie of the running path (0) with the start term (0): the path that is already running
  CHECK(run(g, true, 0, 3, 10).begin == (std::vector<int32_t>{10, 10, 10}));
  std::printf("tie rule ok\nalign frames ok\n");
}
