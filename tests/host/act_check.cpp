// act_check.cpp -- the epilogue arithmetic every int8 kernel shares (fdnn_act.hpp), checked without a GPU: the half-step
// index against the reference's own rounding (lut_index, dnn.h:36-43) and, through the two tables the library builds
// (build_sigmoid_lut and the loader's lut2_build), byte for byte; pack4's byte order; dequant<false> against `/`.
//
// Inputs: the floats within +-64 ulps of k / 200 for k = -1300 .. 1300 (every point where the half-step index changes, the
// clamps at +-1281 included), and every 4099th float bit pattern of both signs below 0.999 * 2^31 / 200 (lut2_index's
// precondition: the conversion to int32 stays in range).  The sweep must reach all 2563 half-step indices and both
// clamps, and an index off by one must be visible in the bytes.
// Built with -fsanitize=address,undefined and run as a child process by tests/test_act_host.py; exit status 0 = all hold.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fdnn_act.hpp"
#include "fdnn_model.hpp"  // build_sigmoid_lut

using namespace fdnn;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
uint32_t bits_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

std::vector<float> sweep() {
  std::vector<float> in;
  for (int k = -1300; k <= 1300; ++k) {
    const float c = static_cast<float>(k / 200.0);
    in.push_back(c);
    float lo = c, hi = c;
    for (int i = 0; i < 64; ++i) {
      lo = std::nextafterf(lo, -INFINITY);
      hi = std::nextafterf(hi, INFINITY);
      in.push_back(lo);
      in.push_back(hi);
    }
  }
  const float limit = static_cast<float>(0.999 * 2147483648.0 / 200.0);
  for (uint32_t b = 0; from_bits(b) < limit; b += 4099) {
    in.push_back(from_bits(b));
    in.push_back(from_bits(b | 0x80000000u));
  }
  return in;
}

// QuantizedSigmoid::get's byte for k = (int)round(lin * 100) (dnn.h:38-42), as it travels: s8 = u8 - 128
uint8_t ref_byte(const uint8_t *lut1280, int index /* lut_index: k clamped, + 640 */) {
  const int k = index - kLutHalf;
  const uint8_t v = k <= -kLutHalf ? 0 : (k >= kLutHalf ? 255 : lut1280[k + kLutHalf]);
  return v ^ 0x80;
}

void half_step() {
  uint8_t lut[kLutSize];
  build_sigmoid_lut(lut);
  std::vector<uint8_t> table2(kLut2Size);
  lut2_build(lut, table2.data());

  const std::vector<float> in = sweep();
  std::vector<int> seen(kLut2Size, 0);
  long clamped_lo = 0, clamped_hi = 0, shifted_differs = 0;
  for (const float lin : in) {
    const int raw = static_cast<int>(std::trunc(lin * 200.0f));  // in range: |lin| < 0.999 * 2^31 / 200
    const int u = lut2_clamp(raw);
    CHECK(lut2_index(lin) == u + kLut2Half);
    clamped_lo += raw < -kLut2Half;
    clamped_hi += raw > kLut2Half;
    ++seen[u + kLut2Half];
    // the index: k = sign(u) * ((|u| + 1) >> 1), clamped as the reference clamps k
    const int mag = ((u < 0 ? -u : u) + 1) >> 1;
    const int k = act_clamp(u < 0 ? -mag : mag, kLutHalf);
    const int want = lut_index(lin);
    if (k != want - kLutHalf) {
      std::fprintf(stderr, "lin = %.9g (0x%08x): half-step k = %d, lut_index - 640 = %d\n", lin, bits_of(lin), k, want - kLutHalf);
      std::exit(1);
    }
    // the byte, through the two tables
    const uint8_t ref = ref_byte(lut, want);
    if (table2[lut2_index(lin)] != ref) {
      std::fprintf(stderr, "lin = %.9g (0x%08x): table2 byte %d, reference byte %d\n", lin, bits_of(lin), table2[lut2_index(lin)], ref);
      std::exit(1);
    }
    const int off = lut2_index(lin) + 1 < kLut2Size ? lut2_index(lin) + 1 : kLut2Size - 1;
    shifted_differs += table2[off] != ref;
  }
  int reached = 0;
  for (int i = 0; i < kLut2Size; ++i) reached += seen[i] > 0;
  std::printf("inputs %zu, half-step indices reached %d of %d, clamped below %ld above %ld, an index one too high changes the byte at %ld inputs\n",
              in.size(), reached, kLut2Size, clamped_lo, clamped_hi, shifted_differs);
  CHECK(reached == kLut2Size && kLut2Size == 2563);
  CHECK(clamped_lo > 0 && clamped_hi > 0);
  CHECK(shifted_differs > 0);
}

void packing() {
  const uint32_t w = pack4(0x11, 0x22, 0x33, 0xf4);
  uint8_t b[4];
  std::memcpy(b, &w, 4);  // little-endian, as the device: byte i of the word is node i of the row
  CHECK(b[0] == 0x11 && b[1] == 0x22 && b[2] == 0x33 && b[3] == 0xf4);
  CHECK(pack4(255, 255, 255, 255) == 0xffffffffu && pack4(0, 0, 0, 0x80) == 0x80000000u);
}

void division() {
  const float coefs[] = {255.0f, 127.0f * 255.0f, 3.0f * 255.0f, 1e-3f, 7.25f};
  for (const float coef : coefs) {
    const float rcp = 1.0f / coef;
    for (long a = -(1L << 29); a <= (1L << 29); a += 104729) {
      const int acc = static_cast<int>(a);
      CHECK(dequant<false>(acc, coef, rcp) == static_cast<float>(acc) / coef);
    }
    CHECK(dequant<false>(0, coef, rcp) == 0.0f && dequant<true>(0, coef, rcp) == 0.0f);
  }
  CHECK(logit_exp(0.0f) == 1.0f && logit_exp(-INFINITY) == 0.0f);
}

}  // namespace

int main() {
  half_step();
  packing();
  division();
  std::printf("act ok\n");
  return 0;
}
