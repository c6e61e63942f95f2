// pool_check.cpp -- fdnn_pool.hpp (the map and its CSR, the order of the additions, the plan, the host restatement) and the
// pool arm of the scoring loop's batch plan (fdnn_server_plan.hpp), alone and under the sanitizers
// (tests/test_pool_host.py builds and runs this).  Must NOT be built with a flush-to-zero or fast-math flag.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <vector>

#include "fdnn_pool.hpp"
#include "fdnn_server_plan.hpp"

using namespace fdnn;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
float float_of(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

void map_validation() {
  const int32_t ok[6] = {0, 2, -1, 1, 2, 0};
  CHECK(pool::check_map(ok, 6, 3) == 0);
  CHECK(pool::check_map(ok, 6, 6) == 0);  // C = W, empty classes
  int32_t bad[6] = {0, 2, -2, 1, 2, 0};
  CHECK(pool::check_map(bad, 6, 3) == 3);  // -2 at index 2
  bad[2] = 3;
  CHECK(pool::check_map(bad, 6, 3) == 3);  // C at index 2
  CHECK(pool::check_map(ok, 6, 7) == -1);  // C > W
  CHECK(pool::check_map(ok, 6, 0) == -1 && pool::check_map(ok, 6, -1) == -1);  // C < 1
  CHECK(pool::check_map(ok, 0, 1) == -1 && pool::check_map(nullptr, 6, 3) == -1);
  CHECK(pool::check_map(ok, 6, 2) == 2);  // 2 is no class of two
  const int32_t none[4] = {-1, -1, -1, -1};
  CHECK(pool::check_map(none, 4, 2) == 0);  // an all -1 map is valid
  const pool::Csr c = pool::build_csr(none, 4, 2);
  CHECK(c.class_ptr == std::vector<int32_t>({0, 0, 0}) && c.member.empty());
}

void csr_is_sorted_and_covers() {
  std::mt19937 rng(5);
  for (int width : {1, 2, 17, 250, 1001}) {
    for (int C : {1, 2, 7, width}) {
      if (C > width) continue;
      std::vector<int32_t> co(static_cast<size_t>(width));
      for (auto &v : co) v = static_cast<int32_t>(rng() % static_cast<unsigned>(C + 1)) - 1;
      CHECK(pool::check_map(co.data(), width, C) == 0);
      const pool::Csr c = pool::build_csr(co.data(), width, C);
      CHECK(c.class_ptr.size() == static_cast<size_t>(C) + 1 && c.class_ptr[0] == 0);
      std::vector<int> seen(static_cast<size_t>(width), 0);
      for (int k = 0; k < C; ++k) {
        CHECK(c.class_ptr[size_t(k) + 1] >= c.class_ptr[size_t(k)]);
        for (int i = c.class_ptr[size_t(k)]; i < c.class_ptr[size_t(k) + 1]; ++i) {
          const int32_t m = c.member[size_t(i)];
          CHECK(m >= 0 && m < width && co[size_t(m)] == k);
          if (i > c.class_ptr[size_t(k)]) CHECK(c.member[size_t(i) - 1] < m);  // ascending inside a class
          ++seen[size_t(m)];
        }
      }
      size_t mapped = 0;
      for (int i = 0; i < width; ++i) {
        CHECK(seen[size_t(i)] == (co[size_t(i)] >= 0 ? 1 : 0));  // exactly the mapped nodes, once
        mapped += co[size_t(i)] >= 0;
      }
      CHECK(c.member.size() == mapped && size_t(c.class_ptr[size_t(C)]) == mapped);
    }
  }
}

// The rule, transcribed literally with float arithmetic (volatile: one rounding to fp32 per +)
float literal(const std::vector<float> &p, const std::vector<int32_t> &m) {
  volatile float s[16];
  const int L = static_cast<int>(m.size());
  for (int j = 0; j < 16; ++j) {
    s[j] = +0.0f;
    for (int t = j; t < L; t += 16) s[j] = s[j] + p[size_t(m[size_t(t)])];
  }
  volatile float a01 = s[0] + s[1], a23 = s[2] + s[3], a45 = s[4] + s[5], a67 = s[6] + s[7];
  volatile float a89 = s[8] + s[9], aab = s[10] + s[11], acd = s[12] + s[13], aef = s[14] + s[15];
  volatile float b0 = a01 + a23, b1 = a45 + a67, b2 = a89 + aab, b3 = acd + aef;
  volatile float c0 = b0 + b1, c1 = b2 + b3;
  volatile float q = c0 + c1;
  return q;
}

void ref_against_literal_and_float64() {
  CHECK(pool::kPoolLanes == 16);
  std::mt19937 rng(11);
  std::normal_distribution<float> nd(0.0f, 3.0f);
  const int sizes[] = {0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257};
  const int C = int(sizeof(sizes) / sizeof(sizes[0]));
  int width = 100;  // (some nodes in no class)
  for (int s : sizes) width += s;
  for (int round = 0; round < 4; ++round) {
    // a soft-max row (rounds 0, 1), signed values (2), values with denormals among them (3)
    std::vector<float> p(static_cast<size_t>(width));
    double tot = 0;
    for (auto &v : p) v = std::exp(nd(rng)), tot += v;
    for (auto &v : p) v = static_cast<float>(v / tot);
    if (round == 2) for (auto &v : p) v = nd(rng);
    if (round == 3) for (size_t i = 0; i < p.size(); i += 3) p[i] = float_of(static_cast<uint32_t>(rng() & 0x7fffffu));
    // classes of the listed sizes, members scattered
    std::vector<int32_t> order(static_cast<size_t>(width)), co(static_cast<size_t>(width), -1);
    for (int i = 0; i < width; ++i) order[size_t(i)] = i;
    std::shuffle(order.begin(), order.end(), rng);
    size_t at = 0;
    for (int c = 0; c < C; ++c)
      for (int k = 0; k < sizes[c]; ++k) co[size_t(order[at++])] = c;
    CHECK(pool::check_map(co.data(), width, C) == 0);
    const pool::Csr csr = pool::build_csr(co.data(), width, C);
    std::vector<uint32_t> rows(p.size()), out(static_cast<size_t>(C));
    for (size_t i = 0; i < p.size(); ++i) rows[i] = bits_of(p[i]);
    pool::ref(rows.data(), 1, width, csr.class_ptr.data(), csr.member.data(), C, out.data());
    for (int c = 0; c < C; ++c) {
      const std::vector<int32_t> m(csr.member.begin() + csr.class_ptr[size_t(c)], csr.member.begin() + csr.class_ptr[size_t(c) + 1]);
      CHECK(int(m.size()) == sizes[c]);
      CHECK(out[size_t(c)] == bits_of(literal(p, m)));
      // float64 (sums of < 2^9 fp32 values: exact enough by 2^-29 relative) and the derived bound
      double sum = 0, mag = 0;
      for (int32_t i : m) sum += double(p[size_t(i)]), mag += std::fabs(double(p[size_t(i)]));
      const double d = pool::depth(sizes[c]), u = std::ldexp(1.0, -24), bound = d * u / (1 - d * u) * mag;
      CHECK(pool::depth(sizes[c]) == (sizes[c] + 15) / 16 + 4);
      CHECK(std::fabs(double(float_of(out[size_t(c)])) - sum) <= bound + mag * std::ldexp(1.0, -40));
      if (sizes[c] == 0) CHECK(out[size_t(c)] == 0u);                           // +0.0f
      if (sizes[c] == 1) CHECK(out[size_t(c)] == rows[size_t(m[0])]);           // a singleton's own bits
    }
  }
  // singletons: own bits for every pattern but -0, which becomes +0; NaN stays a NaN
  const uint32_t pats[] = {0x00000000u, 0x00000001u, 0x807fffffu, 0x00800000u, 0x3f800000u, 0xbf800000u, 0x7f7fffffu, 0x7f800000u, 0xff800000u};
  for (uint32_t u : pats) {
    const int32_t member = 0;
    CHECK(pool::ref_class(&u, &member, 1) == u);
  }
  const uint32_t neg0 = 0x80000000u, nan = 0x7fc00000u;
  const int32_t m0 = 0;
  CHECK(pool::ref_class(&neg0, &m0, 1) == 0u);
  CHECK(std::isnan(float_of(pool::ref_class(&nan, &m0, 1))));
  const uint32_t infs[2] = {0x7f800000u, 0xff800000u};
  const int32_t m01[2] = {0, 1};
  CHECK(std::isnan(float_of(pool::ref_class(infs, m01, 2))));
  CHECK(pool::ref_class(infs, m01, 0) == 0u);
  // denormals are kept: two halves of the smallest normal
  const uint32_t den[2] = {0x00400000u, 0x00400000u};
  CHECK(pool::ref_class(den, m01, 2) == 0x00800000u);
  const uint32_t tiny[2] = {0x00000001u, 0x00000002u};
  CHECK(pool::ref_class(tiny, m01, 2) == 0x00000003u);
}

void plan_forms_and_lds() {
  CHECK(pool::plan(10, pool::kPoolResidentWidth, 0).form == pool::kResident && pool::plan(10, pool::kPoolResidentWidth + 1, 0).form == pool::kStreaming);
  CHECK(pool::plan(10, pool::kPoolResidentWidth, 1).form == pool::kResident && pool::plan(10, pool::kPoolResidentWidth + 1, 1).form == pool::kStreaming);
  CHECK(pool::plan(10, 64, 2).form == pool::kStreaming && pool::plan(10, 1 << 19, 0).form == pool::kStreaming);
  for (int w : {1, 64, 8000, pool::kPoolResidentWidth, pool::kPoolResidentWidth + 1, 1 << 19})
    for (int mode = 0; mode < 3; ++mode) {
      const pool::Plan p = pool::plan(130, w, mode);
      CHECK(p.lds_bytes <= pool::kLdsLimit && p.rows_per_launch == 130 && p.launches == 1);
      CHECK(p.form == pool::kStreaming ? p.lds_bytes == 0 : p.lds_bytes >= 4 * (w + 3));  // the row and its misalignment
    }
  CHECK(pool::kMaxWidth == 1 << 19);
  const pool::Plan big = pool::plan(pool::kMaxRowsPerLaunch + 5, 100, 0);
  CHECK(big.rows_per_launch == pool::kMaxRowsPerLaunch && big.launches == 2);
  CHECK(pool::plan(0, 8000, 0).launches == 0);
}

// ---- the pool arm of plan_batch
constexpr size_t O = 70;
struct Caller {
  std::vector<float> out, pooled;
  float x = 0;
};
const fdnn_pool *handle(int i) { return reinterpret_cast<const fdnn_pool *>(static_cast<uintptr_t>(0x1000 + 0x100 * i)); }  // (never dereferenced by the plan)

plan::Request dense_req(Caller &c, uint64_t ticket, int n) {
  c.out.resize(size_t(n) * O);
  plan::Request r(plan::Frames::rows(&c.x), plan::Want::rows_to(c.out.data()), n);
  r.ticket = ticket;
  return r;
}
plan::Request pool_req(Caller &c, uint64_t ticket, int n, int h, int classes) {
  c.pooled.resize(size_t(n) * size_t(classes));
  plan::Request r(plan::Frames::rows(&c.x), plan::Want::pool_to(handle(h), classes, c.pooled.data()), n);
  r.ticket = ticket;
  return r;
}

void plan_arithmetic() {
  using namespace plan;
  {  // two requests of one handle behind a dense one, then another handle: dense, pool (2 pieces), pool
    Caller c[4];
    std::deque<Request> q{dense_req(c[0], 1, 10), pool_req(c[1], 2, 7, 0, 48), pool_req(c[2], 3, 20, 0, 48), pool_req(c[3], 4, 5, 1, 48)};
    CHECK(q[0].want.kind == Want::rows && q[1].want.kind == Want::pool && Want::pool == 5 && Want::topk == 4);
    BatchPlan b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::rows && b.pieces.size() == 1 && b.rows == 10 && b.pool == nullptr && q.size() == 3);
    b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::pool && b.pieces.size() == 2 && b.rows == 27 && b.pool == handle(0) && b.pool_classes == 48 && b.stride == 0 && !b.any_mask);
    CHECK(b.pieces[0].want.pooled == c[1].pooled.data() && b.pieces[1].want.pooled == c[2].pooled.data() && b.pieces[1].row0 == 7);
    CHECK(b.pieces[0].want.out == nullptr && b.pieces[0].want.k == 0 && !b.pieces[0].want.nodes && b.pieces[0].last);
    b = plan_batch(q, 1000, O);  // different handles are never coalesced, whatever their class counts
    CHECK(b.kind == Want::pool && b.pieces.size() == 1 && b.pool == handle(1) && b.rows == 5 && q.empty());
  }
  {  // a dense or top-k request behind pool ones does not join them, nor the other way round
    Caller c[3];
    Request tk = dense_req(c[2], 3, 4);
    std::vector<int32_t> nodes(4 * 3);
    std::vector<float> probs(4 * 3);
    tk.want = Want::topk_to(3, nodes.data(), probs.data());
    std::deque<Request> q{pool_req(c[0], 1, 4, 0, 2), dense_req(c[1], 2, 4), tk, pool_req(c[0], 4, 4, 0, 2)};
    BatchPlan b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::pool && b.pieces.size() == 1 && q.size() == 3);
    b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::rows && b.pieces.size() == 1 && b.pool == nullptr && b.pieces[0].want.pooled == nullptr);
    b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::topk && b.pieces.size() == 1 && b.pool == nullptr);
    b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::pool && b.pieces.size() == 1 && q.empty());
  }
  {  // a request cut by max_frames continues at taken * C of the caller's array
    Caller c[2];
    std::deque<Request> q{pool_req(c[0], 1, 25, 0, 9), pool_req(c[1], 2, 3, 0, 9)};
    BatchPlan b = plan_batch(q, 10, O);
    CHECK(b.kind == Want::pool && b.rows == 10 && b.pieces.size() == 1 && !b.pieces[0].last && q.front().taken == 10);
    CHECK(b.pieces[0].want.pooled == c[0].pooled.data());
    b = plan_batch(q, 10, O);
    CHECK(b.rows == 10 && b.pieces.size() == 1 && b.pieces[0].want.pooled == c[0].pooled.data() + 10 * 9);
    b = plan_batch(q, 10, O);  // the last 5 rows, and the next request's 3
    CHECK(b.rows == 8 && b.pieces.size() == 2 && b.pieces[0].last && b.pieces[0].rows == 5 && b.pool_classes == 9);
    CHECK(b.pieces[0].want.pooled == c[0].pooled.data() + 20 * 9 && b.pieces[1].want.pooled == c[1].pooled.data() && b.pieces[1].row0 == 5);
    for (const Piece &p : b.pieces)  // every destination the scatter writes is inside the caller's block: touch it
      for (int r = 0; r < p.rows; ++r)
        for (int j = 0; j < b.pool_classes; ++j) p.want.pooled[size_t(r) * size_t(b.pool_classes) + size_t(j)] = 1.0f;
    CHECK(q.empty());
  }
  {  // raw and plain pool requests of one handle do not share a batch
    Caller c[2];
    auto sp = std::make_shared<SpliceSpec>();
    sp->offsets = {-1, 0, 1}, sp->raw_dim = 39, sp->left = 1, sp->right = 1;
    Request raw = pool_req(c[0], 1, 6, 0, 4);
    raw.frames = Frames::raw_rows(&c[0].x, sp, 6, 0);
    std::deque<Request> q{raw, pool_req(c[1], 2, 6, 0, 4)};
    BatchPlan b = plan_batch(q, 100, O);
    CHECK(b.kind == Want::pool && b.raw && b.pieces.size() == 1 && b.raw_frames == 6 && q.size() == 1);
    b = plan_batch(q, 100, O);
    CHECK(b.kind == Want::pool && !b.raw && b.pieces.size() == 1);
  }
}

}  // namespace

int main() {
  map_validation();
  csr_is_sorted_and_covers();
  ref_against_literal_and_float64();
  plan_forms_and_lds();
  plan_arithmetic();
  std::printf("pool ok\n");
  return 0;
}
