// fdnn_act.hpp -- what an int8 layer's epilogue computes from an accumulator: the one definition of its arithmetic.
//
//   hidden layers  lin = sum / coef + bias (dnn.cc:298-311, :250-264), QuantizedSigmoid::get(lin) (dnn.h:36-43): dequant,
//                  then lut_index (the reference's own rounding) or lut2_index (the half-step form, one multiply, one
//                  convert, one clamp), a table byte, four bytes to a word (pack4)
//   output layer   z = sum / coef + bias, e = exp(z) (SoftMax::apply's first loop, dnn.cc:536-540): dequant, logit_exp
// Every kernel that finishes an int8 layer calls these (fdnn_gemm.hip, fdnn_chain.hip, fdnn_pp.hip, fdnn_small.hip,
// fdnn_lists.hip, fdnn_set_tile.hpp; fdnn_l0s.hip for the clamp); fdnn_ppo.hip restates dequant and logit_exp in inline
// assembly, on registers it fixes by hand.  What stays in each kernel is its SCHEDULE: which accumulators it finishes when,
// where the bias comes from, when the table gathers are issued and where the bytes are parked.
//
// Everything is compiled with -ffp-contract=off: each float operation rounds exactly where the reference's scalar / SSE
// code rounds; fused multiply-adds appear only where written as fmaf().  As in fdnn_pair.hpp, every helper is plain and
// takes and returns BY VALUE (the 256-VGPR kernels sit on a register-allocation knife edge).
//
// No HIP needed for the arithmetic: tests/host/act_check.cpp builds this header with a host compiler and holds lut_index
// and the half-step form to each other.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#include "fdnn_model.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FDNN_ACT_HD __host__ __device__ __forceinline__
#else
#define FDNN_ACT_HD inline
#endif

namespace fdnn {

// float(sum) / (multiplier * 255)   -- dnn.cc:298-299, :311.  The fast form is
// the Markstein sequence q = x*y, r = fma(-q, c, x), q' = fma(r, y, q) with
// y = RN(1/c); it is enabled per layer only after launch_fastdiv_check has
// compared it with IEEE division for every accumulator the layer can produce:
// the closed range +-(cols_pad / 2) * 32768, each adjacent pair being saturated
// to int16 (2^26 at K = 4096, 2^29 at the widest layer the loader accepts).
template <bool FAST>
FDNN_ACT_HD float dequant(int acc, float coef, float rcp) {
  const float x = static_cast<float>(acc);  // v_cvt_f32_i32, RNE like cvtsi2ss
  if (FAST) {
    const float q = x * rcp;
    const float r = fmaf(-q, coef, x);
    return fmaf(r, rcp, q);
  }
  return x / coef;
}

// clamp(v, -half, half)
FDNN_ACT_HD int act_clamp(int v, int half) {
#if defined(__HIP_DEVICE_COMPILE__)
  return max(-half, min(half, v));
#else
  return v < -half ? -half : (v > half ? half : v);
#endif
}

// QuantizedSigmoid::get -- dnn.h:36-43: k = (int)round(x*100), table index
// clamp(k,-640,640)+640 into the extended table.  round() is half away from
// zero; the x86 build turns NaN / |t| >= 2^31 into INT_MIN (-> entry 0).
FDNN_ACT_HD int lut_index(float lin) {
  const float t = lin * 100.0f;
  const float r0 = truncf(t);
  // t - r0 is exact; select, do not branch (the epilogue runs this 32*NF times per lane)
  const float r = r0 + ((fabsf(t - r0) >= 0.5f) ? copysignf(1.0f, t) : 0.0f);
  const int k = (fabsf(t) < 2147483648.0f) ? static_cast<int>(r) : INT_MIN;
  return act_clamp(k, kLutHalf) + kLutHalf;
}

// The half-step form of the same index.  k = (int)round(t) (half away from zero) equals sign(u) * ((|u| + 1) >> 1) with
// u = trunc(2t), and 2t = RN(lin*200) exactly (RN(lin*200) = 2*RN(lin*100): a power of two scales without rounding), so
// QuantizedSigmoid::get(lin) = table2[lut2_index(lin)] with table2 as lut2_build fills it: one multiply, one convert, one
// clamp, one byte gather.
// PRECONDITION, established per layer by the loader (fdnn_model.cpp: lin_bounded) -- a layer that fails it runs lut_index:
// no |lin| can reach 2^31 / 200 (the x86 build would turn such a value into INT_MIN -> entry 0, dnn.h:37) and no bias is
// NaN / inf, so the conversion to int32 is in range.
FDNN_ACT_HD int lut2_clamp(int u) { return act_clamp(u, kLut2Half); }
FDNN_ACT_HD int lut2_index(float lin) { return lut2_clamp(static_cast<int>(lin * 200.0f)) + kLut2Half; }

// table2[u + kLut2Half] for u = -kLut2Half .. kLut2Half from the QuantizedSigmoid table (build_sigmoid_lut), stored XOR 0x80
// because activations travel as s8 = u8 - 128.  Host only: the loader's.
inline void lut2_build(const uint8_t *lut1280, uint8_t *table2) {
  for (int u = -kLut2Half; u <= kLut2Half; ++u) {
    const int mag = ((u < 0 ? -u : u) + 1) >> 1;
    const int k = u < 0 ? -mag : mag;
    const uint8_t v = k <= -kLutHalf ? 0 : (k >= kLutHalf ? 255 : lut1280[k + kLutHalf]);  // dnn.h:38-42
    table2[u + kLut2Half] = v ^ 0x80;
  }
}

// four table bytes (four consecutive nodes of one frame) as they lie in an activation row: byte i = node i
FDNN_ACT_HD uint32_t pack4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) { return b0 | b1 << 8 | b2 << 16 | b3 << 24; }

// e = exp(z) of an output logit as one multiply and the hardware's 2^y (v_exp_f32)
constexpr float kLog2e = 1.44269504088896340736f;
FDNN_ACT_HD float exp2_hw(float y) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(y);
#else
  return exp2f(y);
#endif
}
FDNN_ACT_HD float logit_exp(float z) { return exp2_hw(z * kLog2e); }

#if defined(__HIPCC__)
// ... of two logits: the multiply as one packed instruction (fdnn_gemm.hip's dense production epilogues; the two steps
// are separate names for the instance that selects per element between them)
typedef float v2f_t __attribute__((ext_vector_type(2)));
FDNN_ACT_HD v2f_t logit_log2(v2f_t z) { return z * v2f_t{kLog2e, kLog2e}; }
FDNN_ACT_HD v2f_t exp2_hw(v2f_t y) { return v2f_t{exp2_hw(y.x), exp2_hw(y.y)}; }
FDNN_ACT_HD v2f_t logit_exp(v2f_t z) { return exp2_hw(logit_log2(z)); }
#endif

}  // namespace fdnn
