// topk_check.cpp -- the HIP-free half of the top-k return (fdnn_topk.hpp) and the top-k arm of the scoring loop's batch plan
// (fdnn_server_plan.hpp), checked without a GPU.  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_topk_host.py; exit status 0 = all cases hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

#include "fdnn_server_plan.hpp"
#include "fdnn_topk.hpp"

using namespace fdnn;

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

namespace {

float as_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// The order the key must reproduce, stated without it: sign first, then magnitude bits (NaNs past the infinities on both
// sides, -0 below +0): the total order of IEEE 754-2008 5.10 on fp32 bit patterns.
bool total_less(uint32_t a, uint32_t b) {
  const bool na = a >> 31, nb = b >> 31;
  if (na != nb) return na;                      // negative below positive
  const uint32_t ma = a & 0x7fffffffu, mb = b & 0x7fffffffu;
  return na ? ma > mb : ma < mb;
}

void key_is_monotone() {
  // every special value in ascending order
  const uint32_t table[] = {0xffffffffu, 0xffc00000u, 0xff800001u, 0xff800000u, 0xff7fffffu, 0xbf800000u, 0x80800000u, 0x807fffffu, 0x80000001u,
                            0x80000000u, 0x00000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x3f800000u, 0x7f7fffffu, 0x7f800000u, 0x7f800001u,
                            0x7fc00000u, 0x7fffffffu};
  const int T = int(sizeof(table) / sizeof(table[0]));
  for (int i = 0; i + 1 < T; ++i) {
    CHECK(total_less(table[i], table[i + 1]));
    CHECK(topk::key(table[i]) < topk::key(table[i + 1]));
  }
  for (int i = 0; i < T; ++i) CHECK(topk::unkey(topk::key(table[i])) == table[i]);
  // ordinary floats: the key orders as < does
  CHECK(as_float(0x3f800000u) == 1.0f && topk::key(0x3f800000u) > topk::key(0x3f000000u));
  std::mt19937 rng(12345);
  std::vector<uint32_t> v(100000);
  for (uint32_t &u : v) u = rng();
  for (int i = 0; i < T; ++i) v[size_t(i) * 37] = table[i];
  for (size_t i = 0; i + 1 < v.size(); ++i) {
    const uint32_t a = v[i], b = v[i + 1];
    CHECK((topk::key(a) < topk::key(b)) == total_less(a, b));
    CHECK((topk::key(a) == topk::key(b)) == (a == b));
    CHECK(topk::unkey(topk::key(a)) == a);
    const float fa = as_float(a), fb = as_float(b);
    if (fa < fb) CHECK(topk::key(a) < topk::key(b));  // (false for NaNs and for -0 < +0, which only the total order separates)
  }
  CHECK(topk::ranks_before(5, 9, 4, 0) && topk::ranks_before(5, 3, 5, 4) && !topk::ranks_before(5, 4, 5, 3) && !topk::ranks_before(4, 0, 5, 9));
  CHECK(topk::pair_word(5, 3) > topk::pair_word(5, 4) && topk::pair_word(6, 100) > topk::pair_word(5, 0));
}

// full stable sort by descending key: the k first are the contract's answer
std::vector<int32_t> by_full_sort(const uint32_t *row, int width) {
  std::vector<int32_t> idx(static_cast<size_t>(width));
  for (int i = 0; i < width; ++i) idx[size_t(i)] = i;
  std::stable_sort(idx.begin(), idx.end(), [row](int32_t a, int32_t b) { return topk::key(row[a]) > topk::key(row[b]); });
  return idx;
}

void ref_against_full_sort_and_prefix() {
  std::mt19937 rng(777);
  const uint32_t few[] = {0x3f800000u, 0x3f000000u, 0x00000000u, 0x80000000u, 0x7fc00000u, 0xffc00000u, 0x7f800000u, 0x38d1b717u};
  for (int width : {1, 2, 63, 64, 65, 251, 300, 1001}) {
    const int n = 3;
    std::vector<uint32_t> rows(size_t(n) * width);
    for (int r = 0; r < n; ++r)
      for (int i = 0; i < width; ++i)  // row 0: two values; row 1: eight values with both zeros and NaNs; row 2: all equal
        rows[size_t(r) * width + i] = r == 2 ? few[0] : few[rng() % (r == 0 ? 2 : 8)];
    const int kmax = std::min(width, topk::kTopkMaxK);
    std::vector<std::vector<int32_t>> full;
    for (int r = 0; r < n; ++r) full.push_back(by_full_sort(rows.data() + size_t(r) * width, width));
    std::vector<int32_t> prev_nodes;
    std::vector<uint32_t> prev_vals;
    for (int k = 1; k <= kmax; ++k) {  // every k: the answer is the full sort's head, and the top k - 1 is its prefix
      CHECK(topk::args_ok(width, k));
      std::vector<int32_t> nodes(size_t(n) * k);
      std::vector<uint32_t> vals(size_t(n) * k);
      topk::ref(rows.data(), n, width, k, nodes.data(), vals.data());
      for (int r = 0; r < n; ++r)
        for (int j = 0; j < k; ++j) {
          CHECK(nodes[size_t(r) * k + j] == full[size_t(r)][size_t(j)]);
          CHECK(vals[size_t(r) * k + j] == rows[size_t(r) * width + nodes[size_t(r) * k + j]]);
          if (j < k - 1) {
            CHECK(prev_nodes[size_t(r) * (k - 1) + j] == nodes[size_t(r) * k + j]);
            CHECK(prev_vals[size_t(r) * (k - 1) + j] == vals[size_t(r) * k + j]);
          }
        }
      if (width > 2) CHECK(nodes[size_t(2) * k + (k - 1)] == k - 1);  // all equal: nodes 0 .. k - 1
      prev_nodes = nodes, prev_vals = vals;
    }
    CHECK(!topk::args_ok(width, 0) && !topk::args_ok(width, kmax + 1));
  }
  CHECK(!topk::args_ok(0, 1) && topk::args_ok(100000, 256) && !topk::args_ok(100000, 257));
}

void plan_forms_and_lds() {
  const int RW = topk::kTopkResidentWidth;
  CHECK(RW >= 16384 && topk::kTopkMaxK == 256);
  CHECK(topk::plan(5, RW, 0).form == topk::kResident && topk::plan(5, RW + 1, 0).form == topk::kStreaming);
  CHECK(topk::plan(5, RW, 1).form == topk::kResident && topk::plan(5, RW + 1, 1).form == topk::kStreaming);
  CHECK(topk::plan(5, 64, 2).form == topk::kStreaming && topk::plan(5, 64, 0).form == topk::kResident);
  for (int mode = 0; mode <= 2; ++mode)
    for (int width : {1, 2, 63, 64, 65, 251, 1001, 8000, RW - 1, RW, RW + 1, 100000, 1 << 24}) {
      const topk::Plan p = topk::plan(130, width, mode);
      CHECK(p.lds_bytes > 0 && p.lds_bytes <= topk::kLdsLimit && p.lds_bytes <= 160 * 1024);
      if (p.form == topk::kResident) CHECK(p.lds_bytes >= 4 * (width + 3) + 4 * topk::kKeysAt);  // the keys behind any misalignment
      CHECK(p.rows_per_launch == 130 && p.launches == 1);
    }
  const topk::Plan big = topk::plan(topk::kMaxRowsPerLaunch * 2 + 1, 8000, 0);
  CHECK(big.rows_per_launch == topk::kMaxRowsPerLaunch && big.launches == 3);
  CHECK(topk::plan(0, 8000, 0).launches == 0);
}

// ---- the top-k arm of plan_batch
constexpr size_t O = 70;
struct Caller {
  std::vector<float> out, probs;
  std::vector<int32_t> nodes;
  float x = 0;
};

plan::Request dense_req(Caller &c, uint64_t ticket, int n) {
  c.out.resize(size_t(n) * O);
  plan::Request r(plan::Frames::rows(&c.x), plan::Want::rows_to(c.out.data()), n);
  r.ticket = ticket;
  return r;
}
plan::Request topk_req(Caller &c, uint64_t ticket, int n, int k) {
  c.nodes.resize(size_t(n) * k), c.probs.resize(size_t(n) * k);
  plan::Request r(plan::Frames::rows(&c.x), plan::Want::topk_to(k, c.nodes.data(), c.probs.data()), n);
  r.ticket = ticket;
  return r;
}

void plan_arithmetic() {
  using namespace plan;
  {  // k = 3, 32 and 7 behind a dense request: one dense batch, then one top-k batch with k_b = 32
    Caller c[4];
    std::deque<Request> q{dense_req(c[0], 1, 10), topk_req(c[1], 2, 7, 3), topk_req(c[2], 3, 20, 32), topk_req(c[3], 4, 5, 7)};
    CHECK(q[0].want.kind == Want::rows && q[1].want.kind == Want::topk);
    BatchPlan b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::rows && b.pieces.size() == 1 && b.rows == 10 && b.topk_k == 0 && q.size() == 3);
    b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::topk && b.pieces.size() == 3 && b.rows == 32 && b.topk_k == 32 && b.stride == 0 && !b.any_mask && q.empty());
    const int ks[3] = {3, 32, 7}, row0[3] = {0, 7, 27};
    for (int i = 0; i < 3; ++i) {
      const Piece &p = b.pieces[size_t(i)];
      CHECK(p.want.k == ks[i] && p.row0 == row0[i] && p.want.out == nullptr && p.last && !p.want.nodes && p.want.bits == nullptr);
      CHECK(p.want.topk_nodes == c[i + 1].nodes.data() && p.want.topk_probs == c[i + 1].probs.data());
    }
  }
  {  // a dense request behind top-k ones does not join them either
    Caller c[2];
    std::deque<Request> q{topk_req(c[0], 1, 4, 5), dense_req(c[1], 2, 4)};
    BatchPlan b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::topk && b.pieces.size() == 1 && b.topk_k == 5 && q.size() == 1);
    b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::rows && b.topk_k == 0 && b.pieces[0].want.k == 0);
  }
  {  // a request cut by max_frames continues at taken * k of the caller's arrays
    Caller c[2];
    std::deque<Request> q{topk_req(c[0], 1, 25, 9), topk_req(c[1], 2, 3, 200)};
    BatchPlan b = plan_batch(q, 10, O);
    CHECK(b.kind == Want::topk && b.rows == 10 && b.topk_k == 9 && b.pieces.size() == 1 && !b.pieces[0].last && q.front().taken == 10);
    CHECK(b.pieces[0].want.topk_nodes == c[0].nodes.data() && b.pieces[0].want.topk_probs == c[0].probs.data());
    b = plan_batch(q, 10, O);
    CHECK(b.rows == 10 && b.pieces.size() == 1 && b.pieces[0].want.topk_nodes == c[0].nodes.data() + 10 * 9 && b.pieces[0].want.topk_probs == c[0].probs.data() + 10 * 9);
    b = plan_batch(q, 10, O);  // the last 5 rows, and the next request's 3 with the larger k
    CHECK(b.rows == 8 && b.pieces.size() == 2 && b.topk_k == 200 && b.pieces[0].last && b.pieces[0].rows == 5);
    CHECK(b.pieces[0].want.topk_nodes == c[0].nodes.data() + 20 * 9 && b.pieces[0].want.k == 9);
    CHECK(b.pieces[1].want.topk_nodes == c[1].nodes.data() && b.pieces[1].row0 == 5 && b.pieces[1].want.k == 200);
    // every destination the scatter writes is inside the caller's block: touch it
    for (const Piece &p : b.pieces)
      for (int r = 0; r < p.rows; ++r)
        for (int j = 0; j < p.want.k; ++j) p.want.topk_nodes[size_t(r) * p.want.k + j] = 1, p.want.topk_probs[size_t(r) * p.want.k + j] = 1.0f;
    CHECK(q.empty());
  }
  {  // raw and plain top-k requests do not share a batch
    Caller c[2];
    auto sp = std::make_shared<SpliceSpec>();
    sp->offsets = {-1, 0, 1}, sp->raw_dim = 39, sp->left = 1, sp->right = 1;
    Request raw = topk_req(c[0], 1, 6, 4);
    raw.frames = Frames::raw_rows(&c[0].x, sp, 6, 0);
    std::deque<Request> q{raw, topk_req(c[1], 2, 6, 4)};
    BatchPlan b = plan_batch(q, 100, O);
    CHECK(b.kind == Want::topk && b.raw && b.pieces.size() == 1 && b.raw_frames == 6 && q.size() == 1);
    b = plan_batch(q, 100, O);
    CHECK(b.kind == Want::topk && !b.raw && b.pieces.size() == 1);
  }
}

}  // namespace

int main() {
  key_is_monotone();
  ref_against_full_sort_and_prefix();
  plan_forms_and_lds();
  plan_arithmetic();
  std::printf("topk ok\n");
  return 0;
}
