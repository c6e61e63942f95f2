// exp_sweep.cpp -- fb::exp_neg and ln(1 + exp_neg(d)) (fast-dnn_amd/csrc/fdnn_fb.hpp) over ALL floats of their domain against
// float64, as ln_sweep.cpp does for loglik::ln:
//   exp_neg  on every float of [-87, -0] (bit patterns 0x80000000 .. 0xc2ae0000) against exp: the worst error in ulp and
//            where, that no pair of neighbouring floats is out of order, that no result is a denormal, exp_neg(-0) and
//            exp_neg(+0), and the values outside the domain (below -87, -inf, a NaN: +0)
//   lse1(d)  = ln(1.0f + exp_neg(d)), ladd's correction, on every d <= 0 (-inf included) against log1p(exp(d)): the worst
//            absolute error and where, that it is never negative and never above ln 2 rounded, and its order
// kExpMaxUlp and kLse1MaxAbs of the header are this run's worst values rounded up to the next 0.05 ulp and 0.05 x 2^-24;
// the run is recorded in profiles/exp_sweep.log.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I fast-dnn_amd/csrc tools/exp_sweep.cpp -o exp_sweep -lpthread && ./exp_sweep [threads]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "fdnn_fb.hpp"

using fdnn::fb::bits_of;
using fdnn::fb::exp_neg;
using fdnn::fb::float_of;

struct Part {
  double worst = 0, worst_lse = 0;
  uint32_t at = 0, at_lse = 0;
  unsigned long long out_of_order = 0, denormal = 0, lse_out_of_order = 0, lse_out_of_range = 0, outside_not_zero = 0;
};

static double ulp_err(float got, double exact) {
  int ex;
  std::frexp(exact, &ex);
  const int unit = std::max(ex - 24, -149);
  return std::fabs(static_cast<double>(got) - exact) / std::ldexp(1.0, unit);
}

static float lse1(float d) { return fdnn::loglik::ln(1.0f + exp_neg(d)); }

// bit patterns [lo, hi) of negative floats: a larger pattern is a smaller value
static void sweep(uint32_t lo, uint32_t hi, Part *p) {
  const uint32_t edge = bits_of(-87.0f);
  float prev = lo > 0x80000000u ? exp_neg(float_of(lo - 1)) : INFINITY;
  float prev_lse = lo > 0x80000000u ? lse1(float_of(lo - 1)) : INFINITY;
  const float ln2 = fdnn::loglik::ln(2.0f);
  for (uint32_t b = lo; b < hi; ++b) {
    const float x = float_of(b), got = exp_neg(x);
    if (b <= edge) {
      const double exact = std::exp(static_cast<double>(x));
      const double e = ulp_err(got, exact);
      if (e > p->worst) p->worst = e, p->at = b;
      if (!(got <= prev)) ++p->out_of_order;
      if (!(got >= 1.17549435e-38f)) ++p->denormal;
    } else if (bits_of(got) != 0u) {
      ++p->outside_not_zero;
    }
    prev = got;
    const float l = lse1(x);
    const double exact_l = std::log1p(std::exp(static_cast<double>(x)));
    const double el = std::fabs(static_cast<double>(l) - exact_l);
    if (el > p->worst_lse) p->worst_lse = el, p->at_lse = b;
    if (!(l <= prev_lse)) ++p->lse_out_of_order;
    if (!(l >= 0.0f && l <= ln2) || bits_of(l) == 0x80000000u) ++p->lse_out_of_range;
    prev_lse = l;
  }
}

int main(int argc, char **argv) {
  const int threads = argc > 1 ? std::max(1, std::atoi(argv[1])) : 8;
  const uint32_t first = 0x80000000u, end = 0xff800001u;  // -0 .. -inf
  const uint32_t pieces = 64u * static_cast<uint32_t>(threads);
  std::vector<Part> parts(pieces);
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t] {
      for (uint32_t k = static_cast<uint32_t>(t); k < pieces; k += static_cast<uint32_t>(threads)) {
        const uint64_t span = end - first;
        sweep(first + static_cast<uint32_t>(span * k / pieces), first + static_cast<uint32_t>(span * (k + 1) / pieces), &parts[k]);
      }
    });
  for (auto &th : pool) th.join();
  Part all;
  for (const Part &p : parts) {
    if (p.worst > all.worst) all.worst = p.worst, all.at = p.at;
    if (p.worst_lse > all.worst_lse) all.worst_lse = p.worst_lse, all.at_lse = p.at_lse;
    all.out_of_order += p.out_of_order, all.denormal += p.denormal, all.lse_out_of_order += p.lse_out_of_order;
    all.lse_out_of_range += p.lse_out_of_range, all.outside_not_zero += p.outside_not_zero;
  }
  const double lse_u = all.worst_lse * 16777216.0;
  const double up = std::ceil(all.worst / 0.05 - 1e-9) * 0.05, up_lse = std::ceil(lse_u / 0.05 - 1e-9) * 0.05;
  const bool edges = bits_of(exp_neg(-0.0f)) == 0x3f800000u && bits_of(exp_neg(0.0f)) == 0x3f800000u && bits_of(exp_neg(float_of(0x7fc00000u))) == 0u &&
                     bits_of(exp_neg(float_of(0xffc00000u))) == 0u && bits_of(exp_neg(-INFINITY)) == 0u && bits_of(exp_neg(5.0f)) == 0x3f800000u;
  std::printf("exp_neg inputs                 %u (bit patterns 0x80000000 .. 0x%08x: [-87, -0])\n", bits_of(-87.0f) - 0x80000000u + 1u, bits_of(-87.0f));
  std::printf("exp_neg worst error            %.4f ulp at 0x%08x\n", all.worst, all.at);
  std::printf("exp_neg neighbours out of order %llu\n", all.out_of_order);
  std::printf("exp_neg results below the smallest normal  %llu\n", all.denormal);
  std::printf("exp_neg below -87 (to -inf) not +0         %llu\n", all.outside_not_zero);
  std::printf("exp_neg(-0), (+0), (NaN), (-inf), (5)      0x%08x 0x%08x 0x%08x 0x%08x 0x%08x\n", bits_of(exp_neg(-0.0f)), bits_of(exp_neg(0.0f)),
              bits_of(exp_neg(float_of(0x7fc00000u))), bits_of(exp_neg(-INFINITY)), bits_of(exp_neg(5.0f)));
  std::printf("lse1 inputs                    %u (every d <= 0: bit patterns 0x80000000 .. 0xff800000)\n", end - first);
  std::printf("lse1 worst absolute error      %.4f x 2^-24 at 0x%08x\n", lse_u, all.at_lse);
  std::printf("lse1 neighbours out of order   %llu\n", all.lse_out_of_order);
  std::printf("lse1 outside [+0, ln(2.0f)]    %llu\n", all.lse_out_of_range);
  std::printf("kExpMaxUlp: %.2f (the worst error rounded up to 0.05); the header has %.2f\n", up, fdnn::fb::kExpMaxUlp);
  std::printf("kLse1MaxAbs: %.2f x 2^-24 (the worst rounded up to 0.05); the header has %.2f x 2^-24\n", up_lse, fdnn::fb::kLse1MaxAbs * 16777216.0);
  const bool ok = edges && all.denormal == 0 && all.outside_not_zero == 0 && all.lse_out_of_range == 0 && std::fabs(up - fdnn::fb::kExpMaxUlp) < 1e-9 &&
                  std::fabs(up_lse - fdnn::fb::kLse1MaxAbs * 16777216.0) < 1e-9;
  std::printf(ok ? "exp sweep ok\n" : "exp sweep FAILED\n");
  return ok ? 0 : 1;
}
