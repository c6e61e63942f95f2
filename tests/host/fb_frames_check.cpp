// fb_frames_check.cpp -- fdnn_fb_frames.hpp (the frames form of the summed alignment graphs: the contract's consequences, the
// plan and the scratch cap), alone and under the sanitizers (tests/test_fb_frames_host.py builds and runs this).  Must be
// built with -ffp-contract=off and WITHOUT a flush-to-zero or fast-math flag.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "fdnn_fb_frames.hpp"

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

struct Graph {
  int T, S;
  std::vector<float> e;  // [T][S] scores
  std::vector<int32_t> ptr, src, col;
  std::vector<float> lp, start, fin;
};

struct Result {
  std::vector<uint32_t> total, out;
};

// rows [t0, t1) of g
Result run(const Graph &g, bool free_start, int t0, int t1, const std::vector<uint32_t> *in = nullptr) {
  Result r{std::vector<uint32_t>(size_t(t1 - t0), 0x12345678u), std::vector<uint32_t>(size_t(g.S), 0x12345678u)};
  fb_frames::ref(reinterpret_cast<const uint32_t *>(g.e.data()) + size_t(t0) * g.S, t1 - t0, g.S, g.col.data(), nullptr, g.S, nullptr, 0, 0.0f, align::kScores,
                 g.ptr.data(), g.src.data(), g.lp.data(), g.start.data(), g.fin.data(), free_start, in ? in->data() : nullptr, r.out.data(), r.total.data());
  return r;
}

// in-degree 0 .. 3 from any state (loops, backward and parallel arcs, states without arcs), several start and final states
Graph random_graph(int T, int S, std::mt19937 &rng) {
  Graph g{T, S, std::vector<float>(size_t(T) * S), {0}, {}, std::vector<int32_t>(size_t(S)), {}, std::vector<float>(size_t(S)), std::vector<float>(size_t(S))};
  std::normal_distribution<float> n(0.0f, 1.0f);
  std::uniform_real_distribution<float> u(0.05f, 0.95f);
  std::uniform_int_distribution<int> deg(0, 3), any(0, S - 1), coin(0, 1);
  for (float &v : g.e) v = n(rng) - 2.0f;
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

void check_consequences() {
  std::mt19937 rng(1);
  long long prefixes = 0, cuts = 0, planted = 0, above = 0, frames = 0;
  for (int T = 1; T <= 6; ++T)
    for (int S = 1; S <= 5; ++S)
      for (int rep = 0; rep < 12; ++rep) {
        Graph g = random_graph(T, S, rng);
        const Result anchored = run(g, false, 0, T), free_start = run(g, true, 0, T);
        // (a) every prefix against fb::ref
        for (int t = 0; t < T; ++t, ++prefixes) {
          uint32_t total;
          fb::ref(reinterpret_cast<const uint32_t *>(g.e.data()), t + 1, g.S, g.col.data(), nullptr, S, nullptr, 0, 0.0f, align::kScores, g.ptr.data(),
                  g.src.data(), g.lp.data(), g.start.data(), g.fin.data(), nullptr, nullptr, nullptr, &total, nullptr);
          CHECK(anchored.total[size_t(t)] == total);
        }
        // (d) free >= anchored, as floats
        for (int t = 0; t < T; ++t, ++frames) {
          CHECK(float_of(free_start.total[size_t(t)]) >= float_of(anchored.total[size_t(t)]));
          above += float_of(free_start.total[size_t(t)]) > float_of(anchored.total[size_t(t)]);
        }
        // (b) every cut, either start; then (c) with NaN, +inf and -inf planted in the emissions and in alpha_in
        for (int pass = 0; pass < 2; ++pass) {
          for (int f = 0; f < 2; ++f) {
            const Result whole = f ? run(g, true, 0, T) : run(g, false, 0, T);
            for (uint32_t v : whole.total) CHECK(float_of(v) == float_of(v));  // (c)
            for (int c = 1; c < T; ++c, ++cuts) {
              const Result a = run(g, f != 0, 0, c), b = run(g, f != 0, c, T, &a.out);
              for (int t = 0; t < T; ++t) CHECK((t < c ? a.total[size_t(t)] : b.total[size_t(t - c)]) == whole.total[size_t(t)]);
              CHECK(b.out == whole.out);
            }
            if (pass) {
              std::vector<uint32_t> in(size_t(S), bits_of(-1.0f));
              in[size_t(rep % S)] = bits_of(rep % 3 == 0 ? kNaN : (rep % 3 == 1 ? kInf : -kInf));
              const Result r = run(g, f != 0, 0, T, &in);
              for (uint32_t v : r.total) CHECK(float_of(v) == float_of(v));
              ++planted;
            }
          }
          g.e[size_t(rep) % g.e.size()] = rep % 3 == 0 ? kNaN : (rep % 3 == 1 ? kInf : -kInf);
          g.col[size_t(rep % S)] = rep % 5 == 0 ? 9 : g.col[size_t(rep % S)];  // a column out of range: a NaN emission
        }
      }
  CHECK(prefixes > 1000 && cuts > 2000 && above * 2 > frames);
  std::printf("prefixes ok: %lld prefixes have fb::ref's total\n", prefixes);
  std::printf("every cut ok: %lld cuts give the uncut bytes\n", cuts);
  std::printf("never a NaN: %lld calls with a NaN, +inf or -inf planted in alpha_in, as many in the emissions\n", planted);
  std::printf("free start ok: >= the anchored total in %lld frames, above it in %lld\n", frames, above);
}

void check_plan() {
  const int32_t T[5] = {10, 1, 7, 300, 2};
  const int32_t sp[6] = {0, 5, 69, 134, 390, 1390};  // S = 5, 64, 65, 256, 1000
  const long long off[5] = {0, 100, 200, 300, 400};
  const int32_t ld[5] = {3, 4, 5, 6, 7};
  std::vector<int32_t> ap(1391);
  for (int i = 0; i <= 1390; ++i) ap[size_t(i)] = 2 * i;
  const fb_frames::Plan p = fb_frames::plan(T, off, ld, sp, ap.data(), 5, 0);
  const fb::Plan q = fb::plan(T, off, ld, sp, ap.data(), 5, true, 0);
  CHECK(p.scratch_words == 10 * 5 + 64 + 7 * 65 + 300 * 256 + 2 * 1000 && p.total_rows == 320);
  CHECK(p.sweep.launches.size() == q.launches.size() && p.rows.size() == p.sweep.launches.size() && p.rows.size() == 2);  // fb's launches + a row launch each
  for (size_t i = 0; i < q.launches.size(); ++i) CHECK(p.sweep.launches[i].form == q.launches[i].form && p.sweep.launches[i].n_segs == q.launches[i].n_segs);
  const fb_frames::RowLaunch &w = p.rows[0], &g = p.rows[1];
  CHECK(w.n_segs == 2 && w.max_T == 10 && w.frame_off[0] == 0 && w.frame_off[1] == 10 && w.lat_off[1] == 50 && w.S[1] == 64);
  CHECK(g.n_segs == 3 && g.max_T == 300 && g.frame_off[0] == 11 && g.frame_off[1] == 18 && g.frame_off[2] == 318 && g.state0[2] == 390 && g.T[1] == 300);
  CHECK(p.sweep.launches[0].lds_bytes == 4 * fb_frames::wave_lds_words(64, 128) && p.sweep.launches[1].lds_bytes == 8 * 1024);
  CHECK(fb_frames::plan(T, off, ld, sp, ap.data(), 5, 1).rows[0].n_segs == 4 && fb_frames::plan(T, off, ld, sp, ap.data(), 5, 2).rows.size() == 1);
  CHECK(8 * fb::kMaxStates <= 160 * 1024 && 4 * fb_frames::wave_lds_words(256, fb::kArcLdsArcs) <= 64 * 1024);
  // the cap at its edge: the lattice is always needed
  const int32_t sp1[2] = {0, 16384};
  const long long off1[1] = {0};
  const int32_t ld1[1] = {1};
  int32_t tcap[1] = {16384};
  CHECK(fb_frames::plan(tcap, off1, ld1, sp1, nullptr, 1, 0).scratch_words * 4 == fb_frames::kMaxScratchBytes);
  tcap[0] = 16385;
  CHECK(fb_frames::plan(tcap, off1, ld1, sp1, nullptr, 1, 0).scratch_words * 4 > fb_frames::kMaxScratchBytes);
  std::printf("plan ok\n");
}

}  // namespace

int main() {
  check_consequences();
  check_plan();
  std::printf("fb frames ok\n");
  return 0;
}
