// loglik_check.cpp -- fdnn_loglik.hpp (the logarithm, the score, the fp16 conversion, the handle's checks, the plan, the host
// restatement) and the loglik arm of the scoring loop's batch plan (fdnn_server_plan.hpp), alone and under the sanitizers
// (tests/test_loglik_host.py builds and runs this).  Must be built with -ffp-contract=off and WITHOUT a flush-to-zero or
// fast-math flag.  The exhaustive run over every positive float is tools/ln_sweep.cpp (profiles/ln_sweep.log).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <limits>
#include <vector>

#include "fdnn_loglik.hpp"
#include "fdnn_server_plan.hpp"

using namespace fdnn;
using loglik::bits_of;
using loglik::float_of;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

const float kInf = std::numeric_limits<float>::infinity();
bool is_nan(float x) { return x != x; }

// |got - exact| in ulps of the fp32 binade that holds exact (the denormal spacing below 2^-126)
double ulp_err(float got, double exact) {
  int ex;
  std::frexp(exact, &ex);
  return std::fabs(double(got) - exact) / std::ldexp(1.0, std::max(ex - 24, -149));
}

// bit patterns lo, lo + step, ... < hi: against float64 log within kLnMaxUlp, and monotone along the sweep
double sweep(uint32_t lo, uint32_t hi, uint32_t step) {
  double worst = 0;
  float prev = -kInf;
  for (uint64_t b = lo; b < hi; b += step) {
    const float x = float_of(uint32_t(b)), got = loglik::ln(x);
    const double exact = std::log(double(x));
    CHECK(got >= prev);
    prev = got;
    if (exact == 0.0) {
      CHECK(bits_of(got) == 0u);  // ln(1) = +0
      continue;
    }
    const double e = ulp_err(got, exact);
    if (e > worst) worst = e;
    if (!(e <= loglik::kLnMaxUlp)) {
      std::printf("ln(0x%08x) = %.9g, float64 log %.17g: %.4f ulp\n", unsigned(b), double(got), exact, e);
      CHECK(e <= loglik::kLnMaxUlp);
    }
  }
  return worst;
}

void ln_against_float64() {
  const double a = sweep(0x3f000000u, 0x3f800000u, 1);  // every mantissa of [1/2, 1)
  const double b = sweep(0x3f800000u, 0x40000000u, 1);  // ... and of [1, 2)
  const double c = sweep(1u, 0x00800000u, 3);           // every third denormal
  const double d = sweep(1u, 0x7f800000u, 4099);        // a stride through all positive floats
  std::printf("worst ulp: [1/2,1) %.4f, [1,2) %.4f, denormals %.4f, stride %.4f (bound %.2f)\n", a, b, c, d, loglik::kLnMaxUlp);
  CHECK(loglik::kLnMaxUlp == 0.85);  // (profiles/ln_sweep.log: 0.8265 rounded up to the next 0.05)
  CHECK(a > 0.5 && b > 0.5);         // (it is NOT the correctly rounded logarithm: the byte comparisons are not blind)
}

void ln_specials() {
  CHECK(bits_of(loglik::ln(0.0f)) == 0xff800000u && bits_of(loglik::ln(-0.0f)) == 0xff800000u);
  CHECK(bits_of(loglik::ln(kInf)) == 0x7f800000u);
  CHECK(is_nan(loglik::ln(std::numeric_limits<float>::quiet_NaN())));
  CHECK(is_nan(loglik::ln(float_of(0x7f800001u))) && is_nan(loglik::ln(float_of(0xffc12345u))));
  CHECK(is_nan(loglik::ln(-1.0f)) && is_nan(loglik::ln(-kInf)));
  CHECK(is_nan(loglik::ln(float_of(0x80000001u))) && is_nan(loglik::ln(float_of(0x807fffffu))));  // negative denormals
  CHECK(bits_of(loglik::ln(1.0f)) == 0u);
  CHECK(loglik::ln(float_of(1u)) < -103.0f && loglik::ln(float_of(1u)) > -104.0f);  // 2^-149: -103.28
  CHECK(loglik::ln(float_of(0x7f7fffffu)) > 88.7f && loglik::ln(float_of(0x7f7fffffu)) < 88.8f);
  // around the denormal border and the mantissa split the steps meet without a fold
  for (uint32_t c : {0x00800000u, 0x3f3504f3u, 0x3f800000u})
    for (uint32_t b = c - 4096; b < c + 4096; ++b) CHECK(loglik::ln(float_of(b + 1)) >= loglik::ln(float_of(b)));
}

// ---- ref against a literal transcription
float ln_literal(float x) {  // the header's steps once more, written from its comment
  uint32_t b = bits_of(x);
  if (b == 0u || b == 0x80000000u) return -kInf;
  if (x != x || (b >> 31)) return std::numeric_limits<float>::quiet_NaN();
  if (x == kInf) return x;
  int e = 0;
  if (b < 0x00800000u) {
    volatile float s = x * 16777216.0f;
    x = s, b = bits_of(x), e = -24;
  }
  const uint32_t t = b - 0x3f3504f3u;
  e += int32_t(t) >> 23;
  const float m = float_of((t & 0x007fffffu) + 0x3f3504f3u);
  volatile float f = m - 1.0f;
  volatile float z = f * f;
  const float k[9] = {7.0376836292e-2f, -1.1514610310e-1f, 1.1676998740e-1f, -1.2420140846e-1f, 1.4249322787e-1f,
                      -1.6668057665e-1f, 2.0000714765e-1f, -2.4999993993e-1f, 3.3333331174e-1f};
  float p = k[0];
  for (int i = 1; i < 9; ++i) p = std::fmaf(p, f, k[i]);
  volatile float y = f * z;
  y = y * p;
  y = std::fmaf(float(e), -2.12194440e-4f, y);
  y = std::fmaf(-0.5f, z, y);
  volatile float r = f + y;
  return std::fmaf(float(e), 0.693359375f, r);
}

void ref_is_the_literal_rule() {
  const int W = 37, n = 5;
  std::vector<uint32_t> rows(size_t(n) * W);
  std::vector<float> lp(W);
  uint32_t s = 12345u;
  for (auto &v : rows) {
    s = s * 1664525u + 1013904223u;
    v = (s >> 2) % 0x3f800001u;  // (0, 1] and +0
  }
  rows[3] = 0u, rows[4] = 0x80000000u, rows[5] = 0x7fc00000u, rows[6] = 0xbf800000u, rows[7] = 0x7f800000u, rows[8] = 1u, rows[9] = 0x80000001u;
  for (int i = 0; i < W; ++i) lp[size_t(i)] = -0.5f * float(i) - 1.25f;
  for (float floor : {-kInf, -20.0f, -3.0f}) {
    std::vector<uint32_t> o32(rows.size());
    std::vector<uint16_t> o16(rows.size());
    loglik::ref(rows.data(), n, W, lp.data(), floor, loglik::kF32, o32.data());
    loglik::ref(rows.data(), n, W, lp.data(), floor, loglik::kF16, o16.data());
    for (size_t j = 0; j < rows.size(); ++j) {
      volatile float want = ln_literal(float_of(rows[j])) - lp[j % W];
      float w = want;
      if (w < floor) w = floor;
      if (is_nan(w)) {
        CHECK(is_nan(float_of(o32[j])) && (o16[j] & 0x7c00u) == 0x7c00u && (o16[j] & 0x3ffu));
      } else {
        CHECK(o32[j] == bits_of(w) && o16[j] == loglik::half_bits(w));
        if (floor != -kInf) CHECK(w >= floor && float_of(o32[j]) != -kInf);  // with a finite floor no -inf leaves
      }
    }
  }
  // entries: the node's prior; a node outside [0, W) gives a NaN and reads nothing
  const int32_t nodes[6] = {0, 36, -1, 37, std::numeric_limits<int32_t>::min(), 5};
  const uint32_t p[6] = {rows[10], rows[11], rows[12], rows[13], rows[14], rows[15]};
  uint32_t out[6];
  loglik::ref_entries(nodes, p, 6, W, lp.data(), -20.0f, loglik::kF32, out);
  for (int j : {0, 1, 5}) CHECK(out[j] == bits_of(loglik::score(float_of(p[j]), lp[size_t(nodes[j])], -20.0f)));
  for (int j : {2, 3, 4}) CHECK(is_nan(float_of(out[j])));
}

void floor_at_and_around_a_score() {
  const float lp = -2.5f, p = 0.0123f;
  const float s = loglik::score(p, lp, -kInf);
  const float above = std::nextafterf(s, kInf), below = std::nextafterf(s, -kInf);
  CHECK(bits_of(loglik::score(p, lp, s)) == bits_of(s));          // floor == score: the score
  CHECK(bits_of(loglik::score(p, lp, above)) == bits_of(above));  // one ulp above: the floor
  CHECK(bits_of(loglik::score(p, lp, below)) == bits_of(s));      // one ulp below: the score
  CHECK(bits_of(loglik::score(0.0f, lp, -kInf)) == 0xff800000u);  // no floor: -inf leaves
  CHECK(bits_of(loglik::score(0.0f, lp, -30.0f)) == bits_of(-30.0f));
  CHECK(is_nan(loglik::score(-1.0f, lp, -30.0f)));                // a NaN stays a NaN
  CHECK(bits_of(loglik::score(kInf, lp, -30.0f)) == 0x7f800000u);
}

void half_conversion() {
  CHECK(loglik::half_bits(65504.0f) == 0x7bffu && loglik::half_bits(-65504.0f) == 0xfbffu);
  CHECK(loglik::half_bits(65519.9f) == 0x7bffu && loglik::half_bits(65520.0f) == 0x7c00u && loglik::half_bits(-65520.0f) == 0xfc00u);
  CHECK(loglik::half_bits(kInf) == 0x7c00u && loglik::half_bits(-kInf) == 0xfc00u);
  CHECK((loglik::half_bits(float_of(0x7fc00000u)) & 0x7fffu) > 0x7c00u);
  CHECK(loglik::half_bits(0.0f) == 0u && loglik::half_bits(-0.0f) == 0x8000u);
  CHECK(loglik::half_bits(1.0f + 0x1p-11f) == 0x3c00u);  // a tie goes to the even neighbour, 1.0 ...
  CHECK(loglik::half_bits(1.0f + 3 * 0x1p-11f) == 0x3c02u);  // ... and 1 + 2^-9
  CHECK(loglik::half_bits(0x1p-24f) == 1u && loglik::half_bits(0x1p-25f) == 0u && loglik::half_bits(0x1.8p-24f) == 2u);
  CHECK(loglik::half_bits(std::nextafterf(0x1p-25f, 1.0f)) == 1u);
  CHECK(loglik::half_bits(0x1p-14f) == 0x0400u && loglik::half_bits(std::nextafterf(0x1p-14f, 0.0f)) == 0x0400u);  // rounds up into the smallest normal
  CHECK(loglik::half_bits(-20.7232658f) == loglik::half_bits(-20.71875f));  // ln(1e-9): an ordinary fp16 number
#ifdef __FLT16_MANT_DIG__
  const auto hw = [](float s) {
    const _Float16 h = static_cast<_Float16>(s);
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
  };
  unsigned long long checked = 0;
  const auto both = [&](uint32_t b) {
    for (uint32_t sign : {0u, 0x80000000u}) {
      const float s = float_of(b | sign);
      const uint16_t mine = loglik::half_bits(s), theirs = hw(s);
      if (is_nan(s)) CHECK((mine & 0x7c00u) == 0x7c00u && (mine & 0x3ffu) && (theirs & 0x7c00u) == 0x7c00u && (theirs & 0x3ffu));
      else CHECK(mine == theirs);
      ++checked;
    }
  };
  for (uint32_t h = 0; h < 0x7c00u; ++h) {  // every fp16 value's neighbourhood: itself, the ties to both sides, one ulp off them
    const uint16_t hb = uint16_t(h);
    _Float16 hv;
    std::memcpy(&hv, &hb, 2);
    const uint32_t b = bits_of(static_cast<float>(hv));
    const uint32_t half_step = h >= 0x0400u ? 0x1000u : 0u;  // (normals: the tie is 2^12 fp32 ulps up)
    for (uint32_t d : {0u, 1u, half_step - 1u, half_step, half_step + 1u, 2u * half_step - 1u})
      if (b + d < 0x7f800000u) both(b + d);
  }
  for (uint32_t b = 0x33000000u - 64; b < 0x33000000u + 64; ++b) both(b);    // around 2^-25
  for (uint32_t b = 0x38800000u - 8192; b < 0x38800000u + 8192; ++b) both(b);  // around 2^-14, the fp16 denormal border
  for (uint32_t b = 0x33000000u; b < 0x38800000u; b += 1021) both(b);        // through the fp16 denormals (ties included below)
  for (uint32_t q = 1; q < 0x400u; ++q) {  // the ties between fp16 denormals: (q + 1/2) 2^-24
    const float tie = (float(q) + 0.5f) * 0x1p-24f;
    both(bits_of(tie)), both(bits_of(tie) - 1), both(bits_of(tie) + 1);
  }
  for (uint32_t b = 0x477fe000u - 64; b < 0x477ff000u + 64; ++b) both(b);    // 65504 .. 65520 and beyond
  for (uint32_t b = 1; b < 0x7f800000u; b += 65521) both(b);
  both(0x7f800000u), both(0x7fc00000u), both(0x7f800001u);
  std::printf("half conversion against _Float16: %llu values\n", checked);
#endif
}

void handle_checks() {
  const float ok[3] = {-1.0f, -2.0f, 0.0f};
  CHECK(loglik::check_handle(ok, 3, -kInf, loglik::kF32) == 0 && loglik::check_handle(ok, 3, -20.0f, loglik::kF16) == 0);
  CHECK(loglik::check_handle(ok, 3, -65504.0f, loglik::kF16) == 0 && loglik::check_handle(ok, 3, -kInf, loglik::kF16) == 0);
  CHECK(loglik::check_handle(ok, 3, -65505.0f, loglik::kF16) == -2 && loglik::check_handle(ok, 3, -65505.0f, loglik::kF32) == 0);
  CHECK(loglik::check_handle(ok, 3, kInf, loglik::kF32) == -2 && loglik::check_handle(ok, 3, std::nanf(""), loglik::kF32) == -2);
  CHECK(loglik::check_handle(ok, 3, 5.0f, loglik::kF32) == 0);  // a finite floor of either sign
  CHECK(loglik::check_handle(ok, 0, -kInf, 0) == -1 && loglik::check_handle(nullptr, 3, -kInf, 0) == -1 && loglik::check_handle(ok, 3, -kInf, 2) == -1);
  CHECK(loglik::check_handle(ok, loglik::kMaxWidth + 1, -kInf, 0) == -1);
  float bad[3] = {-1.0f, -kInf, 0.0f};
  CHECK(loglik::check_handle(bad, 3, -kInf, 0) == 2);
  bad[1] = -1.0f, bad[2] = std::nanf("");
  CHECK(loglik::check_handle(bad, 3, -kInf, 0) == 3);
  bad[2] = kInf;
  CHECK(loglik::check_handle(bad, 3, -kInf, 0) == 3);
}

void plan_rules() {
  using namespace loglik;
  const auto at = [](uintptr_t a) { return reinterpret_cast<const void *>(a); };
  CHECK(form_for(8000, at(0x1000), at(0x2000), 0) == kVector && form_for(8000, at(0x1000), at(0x2000), 1) == kVector);
  CHECK(form_for(8000, at(0x1000), at(0x2000), 2) == kScalar);
  CHECK(form_for(8000, at(0x1004), at(0x2000), 0) == kScalar && form_for(8000, at(0x1000), at(0x2008), 0) == kScalar);
  CHECK(form_for(8001, at(0x1000), at(0x2000), 0) == kScalar && form_for(8002, at(0x1000), at(0x2000), 1) == kScalar);
  CHECK(form_for(4, at(0x1000), at(0x2000), 0) == kVector && form_for(1, at(0x1000), at(0x2000), 0) == kScalar);
  Plan p = loglik::plan(10000, 8000, kF32, at(0x1000), at(0x2000), 0);
  CHECK(p.form == kVector && p.cols == 4 && p.launches == 1 && p.rows_per_launch == 10000 && p.rows_per_block == 16 && p.grid_x == 625 && p.grid_y == 8 && p.lds_bytes == 0);
  p = loglik::plan(10000, 8000, kF16, at(0x1000), at(0x2000), 0);
  CHECK(p.form == kVector && p.cols == 8 && p.grid_y == 4);
  p = loglik::plan(5, 8004, kF16, at(0x1000), at(0x2000), 0);  // the last thread of a row owns four columns
  CHECK(p.form == kVector && p.rows_per_block == kRowsInFlight && p.grid_x == 2 && p.grid_y == 4 && p.grid_y * kThreads * p.cols >= 8004);
  p = loglik::plan(130, 1001, kF16, at(0x1000), at(0x2000), 0);
  CHECK(p.form == kScalar && p.cols == 1 && p.rows_per_block == 4 && p.grid_x == 33 && p.grid_y == 4);
  p = loglik::plan(100, 8000, kF32, at(0x1000), at(0x2000), 0);  // a 100-frame utterance: 200 workgroups of 4 rows, not 56 of 16
  CHECK(p.rows_per_block == 4 && p.grid_x == 25 && p.grid_y == 8);
  p = loglik::plan(2048, 8000, kF16, at(0x1000), at(0x2000), 0);  // 128 x 4 = 512 < kMinBlocks at 16 rows
  CHECK(p.rows_per_block == 4 && p.grid_x == 512);
  p = loglik::plan(4096, 8000, kF16, at(0x1000), at(0x2000), 0);  // 256 x 4 = kMinBlocks
  CHECK(p.rows_per_block == 16 && p.grid_x == 256);
  p = loglik::plan(kMaxRowsPerLaunch + 1, kMaxWidth, kF32, at(0x1000), at(0x2000), 0);
  CHECK(p.launches == 2 && p.rows_per_launch == kMaxRowsPerLaunch && p.rows_per_block == 16 && p.grid_x == 65536 && p.grid_y == 512);
  CHECK(loglik::plan(0, 8000, kF32, at(0x1000), at(0x2000), 0).launches == 0);
  // every column has exactly one owner, inside the row
  for (int width : {1, 3, 4, 5, 8, 12, 63, 64, 65, 251, 1001, 1004, 8000}) {
    for (int type : {kF32, kF16}) {
      const Plan q = loglik::plan(3, width, type, at(0x1000), at(0x2000), 0);
      long long covered = 0;
      for (int t = 0; t < q.grid_y * kThreads; ++t) {
        const int c0 = t * q.cols;
        if (c0 >= width) continue;
        const int cols = std::min(q.cols, width - c0);
        CHECK(q.form == kScalar || cols == q.cols || (type == kF16 && cols == 4));
        covered += cols;
      }
      CHECK(covered == width);
    }
  }
  CHECK(elem_bytes(kF32) == 4 && elem_bytes(kF16) == 2);
}

// ---- the loglik arm of plan_batch
constexpr size_t O = 70;
struct Caller {
  std::vector<float> out;
  std::vector<uint16_t> scores;  // (sized for either type)
  float x = 0;
};
const fdnn_loglik *handle(int i) { return reinterpret_cast<const fdnn_loglik *>(static_cast<uintptr_t>(0x1000 + 0x100 * i)); }  // (never dereferenced by the plan)

plan::Request dense_req(Caller &c, uint64_t ticket, int n) {
  c.out.resize(size_t(n) * O);
  plan::Request r(plan::Frames::rows(&c.x), plan::Want::rows_to(c.out.data()), n);
  r.ticket = ticket;
  return r;
}
plan::Request ll_req(Caller &c, uint64_t ticket, int n, int h, size_t bytes) {
  c.scores.resize(size_t(n) * O * bytes / 2);
  plan::Request r(plan::Frames::rows(&c.x), plan::Want::loglik_to(handle(h), bytes, c.scores.data()), n);
  r.ticket = ticket;
  return r;
}

void plan_arithmetic() {
  using namespace plan;
  {  // an F32 and an F16 handle never share a batch; requests of one handle do
    Caller c[5];
    std::deque<Request> q{dense_req(c[0], 1, 10), ll_req(c[1], 2, 7, 0, 4), ll_req(c[2], 3, 20, 0, 4), ll_req(c[3], 4, 5, 1, 2), ll_req(c[4], 5, 3, 1, 2)};
    CHECK(q[1].want.kind == Want::loglik && Want::loglik == 6 && Want::pool == 5);
    BatchPlan b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::rows && b.pieces.size() == 1 && b.score == nullptr);
    b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::loglik && b.pieces.size() == 2 && b.rows == 27 && b.score == handle(0) && b.score_bytes == 4 && b.stride == 0 && !b.any_mask);
    CHECK(b.form.leave == Form::scores && b.form.behind == Form::loglik_scores && b.form.words == 27 * O && b.form.upload == Form::no_upload && b.form.pass == Form::loop_rows);
    CHECK(b.pieces[0].want.scores == c[1].scores.data() && b.pieces[1].want.scores == c[2].scores.data() && b.pieces[1].row0 == 7);
    CHECK(b.pieces[0].want.out == nullptr && b.pieces[0].want.pooled == nullptr);
    b = plan_batch(q, 1000, O);
    CHECK(b.kind == Want::loglik && b.pieces.size() == 2 && b.score == handle(1) && b.score_bytes == 2 && b.rows == 8 && q.empty());
    CHECK(b.form.words == 8 * O / 2);  // half the dense batch's bytes
  }
  {  // an odd number of fp16 scores: the transfer is rounded up to whole words
    Caller c[1];
    std::deque<Request> q{ll_req(c[0], 1, 3, 1, 2)};
    BatchPlan b = plan_batch(q, 1000, 5);
    CHECK(b.form.words == 8);  // 3 x 5 x 2 = 30 bytes
  }
  {  // dense, pool and top-k requests in between do not join, nor the other way round
    Caller c[3];
    Request tk = dense_req(c[2], 3, 4);
    std::vector<int32_t> nodes(4 * 3);
    std::vector<float> probs(4 * 3);
    tk.want = Want::topk_to(3, nodes.data(), probs.data());
    Request pl = dense_req(c[2], 4, 4);
    std::vector<float> pooled(4 * 2);
    pl.want = Want::pool_to(reinterpret_cast<const fdnn_pool *>(uintptr_t(0x9000)), 2, pooled.data());
    std::deque<Request> q{ll_req(c[0], 1, 4, 0, 2), dense_req(c[1], 2, 4), tk, pl, ll_req(c[0], 5, 4, 0, 2)};
    for (Want::Kind k : {Want::loglik, Want::rows, Want::topk, Want::pool, Want::loglik}) {
      BatchPlan b = plan_batch(q, 1000, O);
      CHECK(b.kind == k && b.pieces.size() == 1);
    }
    CHECK(q.empty());
  }
  for (size_t bytes : {size_t(4), size_t(2)}) {  // a request cut by max_frames continues at taken x O scores of the caller's array
    Caller c[2];
    std::deque<Request> q{ll_req(c[0], 1, 25, 0, bytes), ll_req(c[1], 2, 3, 0, bytes)};
    char *base = reinterpret_cast<char *>(c[0].scores.data());
    BatchPlan b = plan_batch(q, 10, O);
    CHECK(b.kind == Want::loglik && b.rows == 10 && b.pieces.size() == 1 && !b.pieces[0].last && q.front().taken == 10 && b.pieces[0].want.scores == base);
    b = plan_batch(q, 10, O);
    CHECK(b.rows == 10 && b.pieces.size() == 1 && b.pieces[0].want.scores == base + 10 * O * bytes);
    b = plan_batch(q, 10, O);  // the last 5 rows, and the next request's 3
    CHECK(b.rows == 8 && b.pieces.size() == 2 && b.pieces[0].last && b.pieces[0].rows == 5);
    CHECK(b.pieces[0].want.scores == base + 20 * O * bytes && b.pieces[1].want.scores == c[1].scores.data() && b.pieces[1].row0 == 5);
    // the scatter moves each piece's rows from its byte offset of the landing buffer, inside the caller's block
    std::vector<uint32_t> landing(b.form.words);
    unsigned char *lb = reinterpret_cast<unsigned char *>(landing.data());
    for (size_t i = 0; i < size_t(b.rows) * O * bytes; ++i) lb[i] = static_cast<unsigned char>(i * 7 + 3);
    for (const Piece &p : b.pieces) scatter(b, p, landing.data(), O, [](float *, const float *, int, size_t, size_t, const uint64_t *) { CHECK(false); });
    const unsigned char *a0 = reinterpret_cast<const unsigned char *>(base + 20 * O * bytes), *a1 = reinterpret_cast<const unsigned char *>(c[1].scores.data());
    for (size_t i = 0; i < 5 * O * bytes; ++i) CHECK(a0[i] == lb[i]);
    for (size_t i = 0; i < 3 * O * bytes; ++i) CHECK(a1[i] == lb[5 * O * bytes + i]);
  }
  {  // raw and spliced-row requests of one handle do not share a batch
    Caller c[2];
    auto sp = std::make_shared<SpliceSpec>();
    sp->offsets = {-1, 0, 1}, sp->raw_dim = 39, sp->left = 1, sp->right = 1;
    Request raw = ll_req(c[0], 1, 6, 0, 2);
    raw.frames = Frames::raw_rows(&c[0].x, sp, 6, 0);
    std::deque<Request> q{raw, ll_req(c[1], 2, 6, 0, 2)};
    BatchPlan b = plan_batch(q, 100, O);
    CHECK(b.kind == Want::loglik && b.raw && b.pieces.size() == 1 && b.raw_frames == 6 && q.size() == 1);
    b = plan_batch(q, 100, O);
    CHECK(b.kind == Want::loglik && !b.raw && b.pieces.size() == 1);
  }
}

}  // namespace

int main() {
  ln_specials();
  ln_against_float64();
  ref_is_the_literal_rule();
  floor_at_and_around_a_score();
  half_conversion();
  handle_checks();
  plan_rules();
  plan_arithmetic();
  std::printf("loglik ok\n");
  return 0;
}
