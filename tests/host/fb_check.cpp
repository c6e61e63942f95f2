// fb_check.cpp -- fdnn_fb.hpp (the two stated functions, the summing recursion, the total's order, the transposer, the launch
// plan and the host restatement of forward-backward over alignment graphs), alone and under the sanitizers
// (tests/test_fb_host.py builds and runs this).  Must be built with -ffp-contract=off and WITHOUT a flush-to-zero or
// fast-math flag.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "fdnn_fb.hpp"

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
  const float *start_p() const { return start.empty() ? nullptr : start.data(); }
  const float *fin_p() const { return fin.empty() ? nullptr : fin.data(); }
};

struct Result {
  uint32_t total;
  std::vector<float> gamma;
};

Result run_ref(const Graph &g, bool want_gamma = true) {
  Result r{0, std::vector<float>(want_gamma ? size_t(g.T) * g.S : 0, 77.0f)};
  std::vector<int32_t> tp(size_t(g.S) + 1, 0), ts(g.src.size());
  std::vector<float> tl(g.src.size());
  const int32_t sp[2] = {0, g.S};
  if (want_gamma) CHECK(fb::transpose(sp, 1, g.ptr.data(), g.src.data(), g.lp.data(), tp.data(), ts.data(), tl.data()) == 0);
  fb::ref(reinterpret_cast<const uint32_t *>(g.e.data()), g.T, g.S, g.col.data(), nullptr, g.S, nullptr, 0, 0.0f, align::kScores, g.ptr.data(), g.src.data(),
          g.lp.data(), g.start_p(), g.fin_p(), want_gamma ? tp.data() : nullptr, ts.data(), tl.data(), &r.total,
          want_gamma ? reinterpret_cast<uint32_t *>(r.gamma.data()) : nullptr);
  return r;
}

uint32_t best_total(const Graph &g) {
  std::vector<int32_t> path(size_t(g.T));
  uint32_t total;
  ag::ref(reinterpret_cast<const uint32_t *>(g.e.data()), g.T, g.S, g.col.data(), nullptr, g.S, nullptr, 0, 0.0f, align::kScores, g.ptr.data(), g.src.data(),
          g.lp.data(), g.start_p(), g.fin_p(), path.data(), &total);
  return total;
}

// in-degree 0 .. 3 from any state (self-loops, forward, skip and backward arcs, parallel arcs), several start and final states
Graph random_graph(int T, int S, std::mt19937 &rng, bool soft) {
  Graph g{T, S, std::vector<float>(size_t(T) * S), {0}, {}, std::vector<int32_t>(size_t(S)), {}, std::vector<float>(size_t(S)), std::vector<float>(size_t(S))};
  std::normal_distribution<float> n(0.0f, 1.0f);
  std::uniform_real_distribution<float> u(0.05f, 0.95f);
  std::uniform_int_distribution<int> deg(0, 3), any(0, S - 1), coin(0, 1);
  for (float &v : g.e) v = soft ? n(rng) - 2.0f : 3.0f * n(rng) - 5.0f;
  for (int j = 0; j < S; ++j) {
    g.col[size_t(j)] = j;
    for (int d = deg(rng); d > 0; --d) g.src.push_back(any(rng)), g.lp.push_back(std::log(u(rng)));
    g.ptr.push_back(int32_t(g.src.size()));
    g.start[size_t(j)] = coin(rng) ? std::log(u(rng)) : -kInf;
    g.fin[size_t(j)] = coin(rng) ? std::log(u(rng)) : -kInf;
  }
  g.start[size_t(any(rng))] = 0.0f, g.fin[size_t(any(rng))] = 0.0f;
  return g;
}

// every state sequence in float64: the sum of exp(score) over all sequences and all choices of parallel arcs, and per
// (t, j) the same over the sequences through j at t
void brute(const Graph &g, double *sum, std::vector<double> *through, long long *count, double *max_abs) {
  std::vector<int32_t> p(size_t(g.T), 0);
  long long n = 1;
  for (int t = 0; t < g.T; ++t) n *= g.S;
  *count = n, *sum = 0.0;
  through->assign(size_t(g.T) * g.S, 0.0);
  for (long long code = 0; code < n; ++code) {
    long long c = code;
    for (int t = 0; t < g.T; ++t) p[size_t(t)] = int32_t(c % g.S), c /= g.S;
    double w = std::exp(double(ag::start_of(g.start_p(), p[0])) + double(g.e[size_t(p[0])]));
    for (int t = 1; t < g.T && w > 0; ++t) {
      const int j = p[size_t(t)];
      double arcs = 0.0;
      for (int a = g.ptr[size_t(j)]; a < g.ptr[size_t(j) + 1]; ++a)
        if (g.src[size_t(a)] == p[size_t(t) - 1]) arcs += std::exp(double(g.lp[size_t(a)]));
      w *= arcs * std::exp(double(g.e[size_t(t) * g.S + j]));
    }
    w *= std::exp(double(ag::final_of(g.fin_p(), p[size_t(g.T) - 1], g.S)));
    *sum += w;
    for (int t = 0; t < g.T; ++t) (*through)[size_t(t) * g.S + p[size_t(t)]] += w;
  }
  *max_abs = 0.0;
}

// the header's M and A of a case, from the case: forward-backward in float64 -> the largest finite |alpha| or |bb| plus the
// largest |arc_lp| or finite |final_lp|, and the largest in- or out-degree
void case_bound(const Graph &g, double *max_abs, int *degree) {
  const size_t S = size_t(g.S), T = size_t(g.T);
  auto lse = [](double a, double b) {
    const double hi = std::max(a, b), lo = std::min(a, b);
    return lo == -HUGE_VAL ? hi : hi + std::log1p(std::exp(lo - hi));
  };
  std::vector<double> alpha(T * S, -HUGE_VAL), bb(T * S, -HUGE_VAL);
  for (size_t j = 0; j < S; ++j) {
    alpha[j] = double(ag::start_of(g.start_p(), int(j))) + double(g.e[j]);
    bb[(T - 1) * S + j] = double(ag::final_of(g.fin_p(), int(j), g.S)) + double(g.e[(T - 1) * S + j]);
  }
  for (size_t t = 1; t < T; ++t) {
    std::vector<double> acc(S, -HUGE_VAL), back(S, -HUGE_VAL);
    for (size_t j = 0; j < S; ++j)
      for (int a = g.ptr[j]; a < g.ptr[j + 1]; ++a) {
        const size_t i = size_t(g.src[size_t(a)]);
        acc[j] = lse(acc[j], alpha[(t - 1) * S + i] + double(g.lp[size_t(a)]));
        back[i] = lse(back[i], bb[(T - t) * S + j] + double(g.lp[size_t(a)]));
      }
    for (size_t j = 0; j < S; ++j) alpha[t * S + j] = acc[j] + double(g.e[t * S + j]), bb[(T - 1 - t) * S + j] = back[j] + double(g.e[(T - 1 - t) * S + j]);
  }
  double m = 0, step = 0;
  for (double v : alpha) m = std::isfinite(v) ? std::max(m, std::fabs(v)) : m;
  for (double v : bb) m = std::isfinite(v) ? std::max(m, std::fabs(v)) : m;
  for (float v : g.lp) step = std::max(step, std::fabs(double(v)));
  for (size_t j = 0; j < S; ++j) {
    const double f = double(ag::final_of(g.fin_p(), int(j), g.S));
    if (std::isfinite(f)) step = std::max(step, std::fabs(f));
  }
  *max_abs = m + step;
  std::vector<int> out(S, 0);
  int d = 0;
  for (size_t j = 0; j < S; ++j) {
    d = std::max(d, g.ptr[j + 1] - g.ptr[j]);
    for (int a = g.ptr[j]; a < g.ptr[j + 1]; ++a) d = std::max(d, ++out[size_t(g.src[size_t(a)])]);
  }
  *degree = d;
}

void check_ref_against_brute_force() {
  std::mt19937 rng(1);
  long long cases = 0, seqs = 0, no_path = 0, backward = 0, no_arcs = 0, multi = 0;
  double worst_total = 0, worst_gamma = 0;
  for (int T = 1; T <= 5; ++T)
    for (int S = 1; S <= 4; ++S)
      for (int rep = 0; rep < 20; ++rep) {
        const Graph g = random_graph(T, S, rng, rep >= 10);
        const Result r = run_ref(g);
        const Result f = run_ref(g, false);
        CHECK(f.total == r.total);  // forward only: the same total
        long long n = 0;
        double sum, max_abs;
        std::vector<double> through;
        brute(g, &sum, &through, &n, &max_abs);
        int degree = 0;
        case_bound(g, &max_abs, &degree);
        const float total = float_of(r.total);
        CHECK(total == total);  // never a NaN
        const uint32_t best = best_total(g);
        CHECK(total >= float_of(best));  // total >= the best path's, as floats
        const double delta = fb::delta_bound(T, S, degree, max_abs);  // M and A are the case's own
        if (sum > 0) {
          const double err = std::fabs(double(total) - std::log(sum));
          CHECK(err <= delta);
          worst_total = std::max(worst_total, err);
          double row = 0;
          for (int t = 0; t < T; ++t) {
            row = 0;
            for (int j = 0; j < S; ++j) {
              const size_t at = size_t(t) * S + j;
              const double want = through[at] / sum, err_g = std::fabs(double(r.gamma[at]) - want);
              CHECK(r.gamma[at] >= 0.0f && r.gamma[at] <= 1.0f);
              CHECK(err_g <= fb::gamma_bound(delta, max_abs));
              worst_gamma = std::max(worst_gamma, err_g);
              row += r.gamma[at];
            }
            CHECK(std::fabs(row - 1.0) <= fb::gamma_bound(delta, max_abs) + S * 1.2e-38);  // (the bound is relative where gamma <= 1, and the exact row sums to 1)
          }
          int finite_starts = 0;
          for (int j = 0; j < S; ++j) finite_starts += g.start[size_t(j)] > -kInf;
          multi += finite_starts > 1;
        } else {
          CHECK(r.total == align::kMinusInf && best == align::kMinusInf);  // no path: -inf, and gamma +0 everywhere
          for (float v : r.gamma) CHECK(bits_of(v) == 0u);
          ++no_path;
        }
        for (int j = 0; j < S; ++j) {
          no_arcs += g.ptr[size_t(j)] == g.ptr[size_t(j) + 1];
          for (int a = g.ptr[size_t(j)]; a < g.ptr[size_t(j) + 1]; ++a) backward += g.src[size_t(a)] > j;
        }
        ++cases, seqs += n;
      }
  CHECK(cases >= 400 && no_path > 0 && backward > 0 && no_arcs > 0 && multi > 0);
  std::printf("ref against brute force: %lld graphs, %lld sequences, %lld without a path, %lld backward arcs, %lld states without arcs, %lld with several starts; "
              "worst |total - ln sum| %.3g, worst |gamma - gamma64| %.3g\n", cases, seqs, no_path, backward, no_arcs, multi, worst_total, worst_gamma);
}

// exactly one path of finite score: a strict left-to-right chain without self-loops at T = S, and a single state with a loop
void check_one_path_gives_the_best_paths_bits() {
  std::mt19937 rng(2);
  std::normal_distribution<float> n(0.0f, 1.0f);
  std::uniform_real_distribution<float> u(0.05f, 0.95f);
  int cases = 0;
  for (int S : {1, 2, 3, 7, 40, 300}) {
    Graph g{S, S, std::vector<float>(size_t(S) * S), {0}, {}, std::vector<int32_t>(size_t(S)), {}, {}, {}};
    for (float &v : g.e) v = 3.0f * n(rng) - 5.0f;
    for (int j = 0; j < S; ++j) {
      g.col[size_t(j)] = j;
      if (j) g.src.push_back(j - 1), g.lp.push_back(std::log(u(rng)));
      g.ptr.push_back(int32_t(g.src.size()));
    }
    const Result r = run_ref(g);
    CHECK(align::finite_bits(r.total) && r.total == best_total(g));
    for (int t = 0; t < S; ++t)
      for (int j = 0; j < S; ++j) CHECK(bits_of(r.gamma[size_t(t) * S + j]) == (t == j ? 0x3f800000u : 0u) || (t == j && r.gamma[size_t(t) * S + j] > 0.998f));
    ++cases;
  }
  for (int T : {1, 2, 9, 200}) {  // one state looping
    Graph g{T, 1, std::vector<float>(size_t(T)), {0, 1}, {0}, {0}, {-0.25f}, {}, {}};
    for (float &v : g.e) v = 3.0f * n(rng) - 5.0f;
    const Result r = run_ref(g);
    CHECK(align::finite_bits(r.total) && r.total == best_total(g));
    ++cases;
  }
  std::printf("one path: %d graphs give the best path's bits\n", cases);
}

void check_the_stated_functions() {
  // exp_neg's edges
  CHECK(bits_of(fb::exp_neg(0.0f)) == 0x3f800000u && bits_of(fb::exp_neg(-0.0f)) == 0x3f800000u && bits_of(fb::exp_neg(3.0f)) == 0x3f800000u);
  CHECK(bits_of(fb::exp_neg(kNaN)) == 0u && bits_of(fb::exp_neg(-kInf)) == 0u && bits_of(fb::exp_neg(std::nextafter(-87.0f, -kInf))) == 0u);
  CHECK(fb::exp_neg(-87.0f) >= std::numeric_limits<float>::min());
  std::mt19937 rng(3);
  std::uniform_real_distribution<float> u(-87.0f, 0.0f), w(-200.0f, 200.0f);
  for (int i = 0; i < 200000; ++i) {
    const float x = u(rng), got = fb::exp_neg(x);
    const double want = std::exp(double(x));
    CHECK(std::fabs(double(got) - want) <= fb::kExpMaxUlp * std::ldexp(1.0, std::ilogb(want) - 23) && got >= std::numeric_limits<float>::min());
  }
  // ladd: the stated cases, commutative in its bytes, >= max, within kLse1MaxAbs + one rounding of float64
  CHECK(bits_of(fb::ladd(-kInf, -3.5f)) == bits_of(-3.5f) && bits_of(fb::ladd(-3.5f, -kInf)) == bits_of(-3.5f));
  CHECK(bits_of(fb::ladd(-kInf, -kInf)) == align::kMinusInf && bits_of(fb::ladd(-kInf, -0.0f)) == 0x80000000u);
  CHECK(fb::ladd(kInf, 1.0f) == kInf && fb::ladd(1.0f, kInf) == kInf && fb::ladd(kInf, kInf) == kInf && fb::ladd(kInf, -kInf) == kInf);
  CHECK(bits_of(fb::ladd(kNaN, 1.0f)) == align::kQuietNaN && bits_of(fb::ladd(1.0f, kNaN)) == align::kQuietNaN);
  CHECK(bits_of(fb::ladd(2.0f, 2.0f)) == bits_of(2.0f + loglik::ln(2.0f)));
  for (int i = 0; i < 200000; ++i) {
    const float a = w(rng), b = i % 7 ? w(rng) : a + 1e-3f * w(rng);
    const float s = fb::ladd(a, b);
    CHECK(bits_of(s) == bits_of(fb::ladd(b, a)) && s >= std::max(a, b));
    const double want = std::max(double(a), double(b)) + std::log1p(std::exp(-std::fabs(double(a) - double(b))));
    CHECK(std::fabs(double(s) - want) <= fb::kLse1MaxAbs + 2.0 * std::ldexp(1.0, std::ilogb(std::fabs(want) + 1.0) - 23));
  }
  // a NaN candidate is never added; a NaN emission makes no total a NaN
  CHECK(bits_of(fb::accumulate(-2.0f, kNaN, 1.0f)) == bits_of(-2.0f) && bits_of(fb::accumulate(-kInf, kInf, -kInf)) == align::kMinusInf);
  std::mt19937 r2(4);
  for (int rep = 0; rep < 50; ++rep) {
    Graph g = random_graph(4, 4, r2, true);
    g.e[size_t(rep % 16)] = rep % 3 == 0 ? kNaN : (rep % 3 == 1 ? kInf : -kInf);
    g.col[size_t(rep % 4)] = rep % 5 == 0 ? 9 : g.col[size_t(rep % 4)];  // a column out of range: a NaN emission
    const Result r = run_ref(g);
    const float t = float_of(r.total);
    CHECK(t == t && t >= float_of(best_total(g)));
    for (float v : r.gamma) CHECK(v >= 0.0f && v <= 1.0f);
    if (!align::finite_bits(r.total))
      for (float v : r.gamma) CHECK(bits_of(v) == 0u);
  }
  // gamma's element
  CHECK(bits_of(fb::gamma_of(-1.0f, -2.0f, -0.5f, -kInf)) == 0u && bits_of(fb::gamma_of(-1.0f, -2.0f, -0.5f, kInf)) == 0u);
  CHECK(bits_of(fb::gamma_of(kNaN, -2.0f, -0.5f, -3.0f)) == 0u && bits_of(fb::gamma_of(-1.0f, -1.0f, -1.0f, -2.0f)) == 0x3f800000u);  // x > 0 -> 0
  CHECK(bits_of(fb::gamma_of(-kInf, -kInf, -kInf, -3.0f)) == 0u);
  std::printf("stated functions ok\n");
}

void check_transpose() {
  std::mt19937 rng(5);
  int cases = 0;
  for (int rep = 0; rep < 200; ++rep) {
    const int n_segs = 1 + rep % 4;
    std::vector<int32_t> sp{0}, ptr{0}, src;
    std::vector<float> lp;
    for (int s = 0; s < n_segs; ++s) {
      const int S = 1 + int(rng() % 9);
      for (int j = 0; j < S; ++j) {
        for (int d = int(rng() % 4); d > 0; --d) src.push_back(int32_t(rng() % S)), lp.push_back(float(src.size()));
        ptr.push_back(int32_t(src.size()));
      }
      sp.push_back(sp.back() + S);
    }
    std::vector<int32_t> tp(ptr.size(), -1), ts(src.size(), -1);
    std::vector<float> tl(src.size(), -1.0f);
    CHECK(fb::transpose(sp.data(), n_segs, ptr.data(), src.data(), lp.data(), tp.data(), ts.data(), tl.data()) == 0);
    // the literal double loop: for every source i ascending, every arc ascending whose source is i
    size_t at = 0;
    for (int s = 0; s < n_segs; ++s)
      for (int i = 0; i < sp[size_t(s) + 1] - sp[size_t(s)]; ++i) {
        CHECK(tp[size_t(sp[size_t(s)] + i)] == int32_t(at));
        for (int j = 0; j < sp[size_t(s) + 1] - sp[size_t(s)]; ++j)
          for (int a = ptr[size_t(sp[size_t(s)] + j)]; a < ptr[size_t(sp[size_t(s)] + j) + 1]; ++a)
            if (src[size_t(a)] == i) {
              CHECK(ts[at] == j && tl[at] == lp[size_t(a)]);
              ++at;
            }
      }
    CHECK(at == src.size() && tp.back() == int32_t(src.size()));
    ++cases;
  }
  const int32_t sp[2] = {0, 2}, ptr[3] = {0, 1, 2}, bad[2] = {0, 2};
  const float lp[2] = {0, 0};
  int32_t tp[3], ts[2];
  float tl[2];
  CHECK(fb::transpose(sp, 1, ptr, bad, lp, tp, ts, tl) == -1);  // a source outside [0, S)
  std::printf("transpose ok: %d calls against the double loop\n", cases);
}

// the total's order, transcribed literally from the contract
float literal_total(const std::vector<float> &last, const std::vector<float> &fin) {
  const int S = int(last.size());
  float partial[256];
  for (int i = 0; i < 256; ++i) partial[i] = -kInf;
  for (int j = 0; j < S; ++j) {
    const float term = last[size_t(j)] + fin[size_t(j)];
    if (term != term) continue;
    partial[j % 256] = fb::ladd(partial[j % 256], term);
  }
  for (int step = 128; step >= 1; step /= 2)
    for (int i = 0; i < step; ++i) partial[i] = fb::ladd(partial[i], partial[i + step]);
  return partial[0];
}

void check_total_order() {
  std::mt19937 rng(6);
  std::normal_distribution<float> n(0.0f, 1.0f);
  int differ_from_sequential = 0;
  for (int S : {1, 2, 255, 256, 257, 511, 512, 513, 2000}) {
    std::vector<float> last(static_cast<size_t>(S)), fin(static_cast<size_t>(S));
    for (int j = 0; j < S; ++j) last[size_t(j)] = 2.0f * n(rng) - 30.0f, fin[size_t(j)] = rng() % 3 ? -0.5f * float(rng() % 5) : -kInf;
    fin[size_t(S) / 2] = 0.0f;
    if (S > 2) last[1] = kNaN;  // skipped
    const float got = fb::total_of(last.data(), fin.data(), S);
    CHECK(bits_of(got) == bits_of(literal_total(last, fin)) && got == got);
    float seq = -kInf;
    for (int j = 0; j < S; ++j)
      if (last[size_t(j)] + fin[size_t(j)] == last[size_t(j)] + fin[size_t(j)]) seq = fb::ladd(seq, last[size_t(j)] + fin[size_t(j)]);
    differ_from_sequential += bits_of(seq) != bits_of(got);
    CHECK(std::fabs(seq - got) < 1e-3f);
  }
  // through ref: T = 1, every state final
  for (int S : {255, 256, 257, 511, 512, 513}) {
    Graph g{1, S, std::vector<float>(size_t(S)), std::vector<int32_t>(size_t(S) + 1, 0), {}, std::vector<int32_t>(size_t(S)), {}, std::vector<float>(size_t(S), 0.0f),
            std::vector<float>(size_t(S), -1.0f)};
    for (int j = 0; j < S; ++j) g.e[size_t(j)] = n(rng) - 3.0f, g.col[size_t(j)] = j;
    std::vector<float> last(static_cast<size_t>(S));
    for (int j = 0; j < S; ++j) last[size_t(j)] = 0.0f + g.e[size_t(j)];
    CHECK(run_ref(g).total == bits_of(literal_total(last, g.fin)));
  }
  std::printf("total order ok (%d of 9 differ from the sequential sum's bits)\n", differ_from_sequential);
}

void check_plan() {
  const int32_t T[5] = {10, 1, 7, 300, 2};
  const int32_t sp[6] = {0, 5, 69, 134, 390, 1390};  // S = 5, 64, 65, 256, 1000
  const long long off[5] = {0, 100, 200, 300, 400};
  const int32_t ld[5] = {3, 4, 5, 6, 7};
  std::vector<int32_t> ap(1391);
  for (int i = 0; i <= 1390; ++i) ap[size_t(i)] = 2 * i;
  for (int want = 0; want < 2; ++want) {
    const fb::Plan p = fb::plan(T, off, ld, sp, ap.data(), 5, want != 0, 0);
    const long long words = 10 * 5 + 64 + 7 * 65 + 300 * 256 + 2 * 1000;
    CHECK(p.gamma_words == words && p.scratch_words == (want ? words : 0));
    CHECK(p.launches.size() == 2 && p.launches[0].form == fb::kWave && p.launches[0].n_segs == 2 && p.launches[1].form == fb::kWorkgroup &&
          p.launches[1].n_segs == 3);
    const fb::Launch &w = p.launches[0], &g = p.launches[1];
    CHECK(w.K == 1 && w.d_floats == 64 && w.arc_cap == 128 && w.lds_bytes == 4 * fb::wave_lds_words(64, 128));
    CHECK(w.S[0] == 5 && w.S[1] == 64 && w.out_off[0] == 0 && w.out_off[1] == 50 && w.total_off[1] == 1 && w.arc0[1] == 10 && w.n_arcs[1] == 128);
    CHECK(g.d_floats == 1024 && g.lds_bytes == 4 * fb::wg_lds_words(1024) && g.out_off[0] == 114 && g.out_off[1] == 114 + 455 && g.out_off[2] == 114 + 455 + 76800);
    CHECK(g.row_off[2] == 400 && g.ld[2] == 7 && g.state0[2] == 390 && g.total_off[2] == 4);
  }
  const fb::Plan forced = fb::plan(T, off, ld, sp, ap.data(), 5, true, 1);
  CHECK(forced.launches.size() == 2 && forced.launches[0].n_segs == 4 && forced.launches[0].K == 4 && forced.launches[0].d_floats == 256);
  CHECK(fb::plan(T, off, ld, sp, ap.data(), 5, true, 2).launches.size() == 1);
  CHECK(fb::form_for(64, 0) == fb::kWave && fb::form_for(65, 0) == fb::kWorkgroup && fb::form_for(256, 1) == fb::kWave && fb::form_for(257, 1) == fb::kWorkgroup);
  // 65 segments: two launches of one form; the LDS of the largest graph inside 160 KiB
  std::vector<int32_t> t65(65, 3), sp65(66);
  std::vector<long long> off65(65, 0);
  std::vector<int32_t> ld65(65, 1);
  for (int i = 0; i <= 65; ++i) sp65[size_t(i)] = 4 * i;
  const fb::Plan many = fb::plan(t65.data(), off65.data(), ld65.data(), sp65.data(), nullptr, 65, true, 0);
  CHECK(many.launches.size() == 2 && many.launches[0].n_segs == 64 && many.launches[1].n_segs == 1 && many.launches[1].out_off[0] == 64 * 12);
  CHECK(4 * fb::wg_lds_words(fb::kMaxStates) <= 160 * 1024 && 4 * fb::wave_lds_words(256, fb::kArcLdsArcs) <= 64 * 1024);
  // the cap at its edge: T S = 2^28 words is 2^30 bytes, allowed; one more row is above it
  const int32_t sp1[2] = {0, 16384};
  const long long off1[1] = {0};
  const int32_t ld1[1] = {1};
  int32_t tcap[1] = {16384};
  CHECK(fb::plan(tcap, off1, ld1, sp1, nullptr, 1, true, 0).scratch_words * 4 == fb::kMaxScratchBytes);
  tcap[0] = 16385;
  CHECK(fb::plan(tcap, off1, ld1, sp1, nullptr, 1, true, 0).scratch_words * 4 > fb::kMaxScratchBytes);
  CHECK(fb::plan(tcap, off1, ld1, sp1, nullptr, 1, false, 0).scratch_words == 0);
  std::printf("plan ok\n");
}

}  // namespace

int main() {
  check_the_stated_functions();
  check_ref_against_brute_force();
  check_one_path_gives_the_best_paths_bits();
  check_transpose();
  check_total_order();
  check_plan();
  std::printf("fb ok\n");
  return 0;
}
