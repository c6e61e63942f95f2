// ln_sweep.cpp -- loglik::ln (fast-dnn_amd/csrc/fdnn_loglik.hpp) over ALL 2 139 095 039 positive finite floats against
// float64 log, whose own error is below 2^-29 of an fp32 ulp: the worst error in ulp and where, the worst on (0, 1], that
// no pair of neighbouring floats is out of order, ln(1), and how many results on (0, 1] differ from the correctly rounded
// float64 logarithm and from the C library's logf.  kLnMaxUlp of the header is this run's worst error rounded up to the
// next 0.05 ulp; the run is recorded in profiles/ln_sweep.log.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I fast-dnn_amd/csrc tools/ln_sweep.cpp -o ln_sweep -lpthread && ./ln_sweep [threads]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "fdnn_loglik.hpp"

using fdnn::loglik::bits_of;
using fdnn::loglik::float_of;

struct Part {
  double worst = 0, worst01 = 0;
  uint32_t at = 0, at01 = 0;
  unsigned long long out_of_order = 0, not_rounded01 = 0, not_logf01 = 0;
};

// |got - exact| in ulps of the fp32 binade that holds exact (the denormal spacing below 2^-126)
static double ulp_err(float got, double exact) {
  int ex;
  std::frexp(exact, &ex);  // |exact| in [2^(ex-1), 2^ex)
  const int unit = std::max(ex - 24, -149);
  return std::fabs(static_cast<double>(got) - exact) / std::ldexp(1.0, unit);
}

static void sweep(uint32_t lo, uint32_t hi, Part *p) {  // bit patterns [lo, hi)
  float prev = lo > 1 ? fdnn::loglik::ln(float_of(lo - 1)) : -INFINITY;
  for (uint32_t b = lo; b < hi; ++b) {
    const float x = float_of(b), got = fdnn::loglik::ln(x);
    const double exact = std::log(static_cast<double>(x));
    if (!(got >= prev)) ++p->out_of_order;
    prev = got;
    if (exact != 0.0) {
      const double e = ulp_err(got, exact);
      if (e > p->worst) p->worst = e, p->at = b;
      if (b <= 0x3f800000u && e > p->worst01) p->worst01 = e, p->at01 = b;
    } else if (bits_of(got) != 0u) {
      p->worst = 1e9, p->at = b;  // ln(1) must be +0
    }
    if (b <= 0x3f800000u) {
      if (bits_of(got) != bits_of(static_cast<float>(exact))) ++p->not_rounded01;
      if (bits_of(got) != bits_of(std::log(x))) ++p->not_logf01;
    }
  }
}

int main(int argc, char **argv) {
  const int threads = argc > 1 ? std::max(1, std::atoi(argv[1])) : 8;
  const uint32_t first = 1u, end = 0x7f800000u;  // every positive finite float
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
    if (p.worst01 > all.worst01) all.worst01 = p.worst01, all.at01 = p.at01;
    all.out_of_order += p.out_of_order, all.not_rounded01 += p.not_rounded01, all.not_logf01 += p.not_logf01;
  }
  const double up = std::ceil(all.worst / 0.05 - 1e-9) * 0.05;
  std::printf("inputs                         %llu (bit patterns 0x%08x .. 0x%08x)\n", static_cast<unsigned long long>(end - first), first, end - 1);
  std::printf("worst error                    %.4f ulp at 0x%08x\n", all.worst, all.at);
  std::printf("worst error on (0, 1]          %.4f ulp at 0x%08x\n", all.worst01, all.at01);
  std::printf("neighbours out of order        %llu\n", all.out_of_order);
  std::printf("ln(1) bits                     0x%08x\n", bits_of(fdnn::loglik::ln(1.0f)));
  std::printf("on (0, 1]: differ from float64 log rounded   %llu\n", all.not_rounded01);
  std::printf("on (0, 1]: differ from the C library's logf  %llu\n", all.not_logf01);
  std::printf("kLnMaxUlp: %.2f (the worst error rounded up to 0.05); the header has %.2f\n", up, fdnn::loglik::kLnMaxUlp);
  const bool ok = all.out_of_order == 0 && bits_of(fdnn::loglik::ln(1.0f)) == 0u && std::fabs(up - fdnn::loglik::kLnMaxUlp) < 1e-9;
  std::printf(ok ? "ln sweep ok\n" : "ln sweep FAILED\n");
  return ok ? 0 : 1;
}
