// fdnn_loglik.hpp -- the HIP-free half of the dense output as DECODER SCORES (fdnn_loglik.hip): the logarithm, the score of
// an element, the fp16 conversion, the launch plan and a plain host restatement.  The arithmetic is stated here and nowhere
// else: the kernels call ln() and score() of this header.  tests/host/loglik_check.cpp builds it alone, under the sanitizers.
//
// The scores extend CalculateOutput (src/cpp/dnn.cc:428-454): of a row p[0 .. W) of probabilities and a handle's
// log_prior[0 .. W), floor and type
//
//   s_i = ln(p_i) - log_prior[i]          one fp32 subtraction, round to nearest even
//   s_i = (s_i < floor) ? floor : s_i     a NaN stays a NaN; floor = -inf is no floor
//   F16: the RN-even conversion of s_i    |s_i| >= 65520 becomes +-inf, fp16 denormals are kept
//
// ln is NOT the hardware's logarithm and not the C library's: it is ONE fixed sequence of fp32 operations -- fmaf, single
// multiplications, additions and subtractions rounded on their own, integer operations on the bit pattern -- so that the
// host and the device give the same bits (both build with -ffp-contract=off and without any flush-to-zero or fast-math
// flag; denormals are kept).  It is the classic single-precision Cephes scheme:
//
//   NaN -> a NaN;  any negative value (negative denormals and -inf included) -> a NaN;  +0, -0 -> -inf;  +inf -> +inf
//   a denormal is multiplied by 2^24 first (exact);  x = 2^e m with m in [sqrt(1/2), sqrt(2)) by integer operations;
//   f = m - 1 (exact);  ln x = f - f^2/2 + f^3 P(f) + e ln 2,  ln 2 = 0.693359375 - 2.12194440e-4
//
// Measured over ALL 2 139 095 039 positive finite floats against float64 log (tools/ln_sweep.cpp,
// profiles/ln_sweep.log): the worst error is 0.8265 ulp (at 0x3fb4f239), no pair of neighbouring floats is out of order, and
// ln(1) = +0.  kLnMaxUlp is that worst error rounded up to the next 0.05 ulp.  FROZEN: results depend on every constant and
// on the order of the operations below.
//
// s is a function of the row and the handle alone: not of the row's position, the batch, the entry point or the kernel
// form.  With a finite floor no -inf leaves the device.  Note that the k best probabilities are NOT the k best scores:
// dividing by the priors reorders the nodes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FDNN_LOGLIK_HD __host__ __device__ __forceinline__
#else
#define FDNN_LOGLIK_HD inline
#endif

namespace fdnn {
namespace loglik {

constexpr double kLnMaxUlp = 0.85;           // the exhaustive sweep's worst error, 0.8265 ulp, rounded up to 0.05
constexpr int kF32 = 0, kF16 = 1;            // FDNN_LOGLIK_F32, FDNN_LOGLIK_F16
constexpr int kMaxWidth = 1 << 19;           // the loader's widest output layer
constexpr float kHalfMax = 65504.0f;         // a finite floor of an F16 handle is not below -kHalfMax

FDNN_LOGLIK_HD uint32_t bits_of(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bit_cast(uint32_t, x);
#else
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return b;
#endif
}
FDNN_LOGLIK_HD float float_of(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bit_cast(float, b);
#else
  float x;
  std::memcpy(&x, &b, 4);
  return x;
#endif
}

// ---------------------------------------------------------------- the logarithm
FDNN_LOGLIK_HD float ln(float x) {
  uint32_t b = bits_of(x);
  if ((b << 1) == 0u) return float_of(0xff800000u);  // +0, -0: -inf
  if (b > 0x7f800000u) return float_of(0x7fc00000u); // a NaN, or the sign is set: a NaN
  if (b == 0x7f800000u) return x;                    // +inf
  int e = 0;
  if (b < 0x00800000u) {  // a denormal: times 2^24, exact
    x = x * 0x1p24f;
    b = bits_of(x);
    e = -24;
  }
  const uint32_t t = b - 0x3f3504f3u;  // (0x3f3504f3: sqrt(1/2) rounded up)
  e += static_cast<int32_t>(t) >> 23;
  const float m = float_of((t & 0x007fffffu) + 0x3f3504f3u);  // in [sqrt(1/2), sqrt(2))
  const float f = m - 1.0f;                                    // exact
  const float z = f * f;
  float p = 7.0376836292e-2f;
  p = fmaf(p, f, -1.1514610310e-1f);
  p = fmaf(p, f, 1.1676998740e-1f);
  p = fmaf(p, f, -1.2420140846e-1f);
  p = fmaf(p, f, 1.4249322787e-1f);
  p = fmaf(p, f, -1.6668057665e-1f);
  p = fmaf(p, f, 2.0000714765e-1f);
  p = fmaf(p, f, -2.4999993993e-1f);
  p = fmaf(p, f, 3.3333331174e-1f);
  const float fe = static_cast<float>(e);
  float y = f * z;
  y = y * p;
  y = fmaf(fe, -2.12194440e-4f, y);
  y = fmaf(-0.5f, z, y);
  float r = f + y;
  r = fmaf(fe, 0.693359375f, r);
  return r;
}

// ---------------------------------------------------------------- one element's score
FDNN_LOGLIK_HD float score(float p, float log_prior, float floor) {
  float s = ln(p) - log_prior;
  s = (s < floor) ? floor : s;  // (false for a NaN: it stays)
  return s;
}

// fp32 -> fp16 bits, round to nearest even, denormals kept, overflow to +-inf, a NaN to a NaN: IEEE 754's conversion in
// integer operations.  The kernels use the hardware's conversion, which is this one (tests hold both to _Float16).
inline uint16_t half_bits(float s) {
  const uint32_t b = bits_of(s), sign = (b >> 16) & 0x8000u, a = b & 0x7fffffffu;
  if (a > 0x7f800000u) return static_cast<uint16_t>(sign | 0x7e00u);   // NaN
  if (a >= 0x477ff000u) return static_cast<uint16_t>(sign | 0x7c00u);  // |s| >= 65520 (inf included): +-inf
  if (a < 0x33000000u) return static_cast<uint16_t>(sign);             // |s| < 2^-25: +-0  (2^-25 itself ties to even: 0)
  uint32_t mant, shift;
  if (a < 0x38800000u) {  // below 2^-14: an fp16 denormal, unit 2^-24
    mant = (a & 0x007fffffu) | 0x00800000u;
    shift = 126u - (a >> 23);  // exponent fields 112 .. 102: 14 .. 24 bits of the 24-bit mantissa fall below the unit
    uint32_t q = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (q & 1u))) ++q;  // (may carry into the smallest normal: the right bits)
    return static_cast<uint16_t>(sign | q);
  }
  uint32_t q = (a - 0x38000000u) >> 13;  // exponent rebased by 112, ten mantissa bits
  const uint32_t rem = a & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (q & 1u))) ++q;  // (a carry moves to the next binade; 65520 and above went to inf)
  return static_cast<uint16_t>(sign | q);
}

// ---------------------------------------------------------------- the handle's arguments
// 0 when log_prior [width], floor and type make a handle, else 1 + the index of the first prior that is not finite, or
// -1 for a bad width / type / null priors, -2 for a bad floor (a NaN, +inf, or finite below -65504 with F16)
inline long long check_handle(const float *log_prior, int width, float floor, int type) {
  if (!log_prior || width < 1 || width > kMaxWidth || (type != kF32 && type != kF16)) return -1;
  if (floor != floor || bits_of(floor) == 0x7f800000u) return -2;
  if (type == kF16 && bits_of(floor) != 0xff800000u && floor < -kHalfMax) return -2;
  for (int i = 0; i < width; ++i)
    if ((bits_of(log_prior[i]) & 0x7f800000u) == 0x7f800000u) return 1 + static_cast<long long>(i);
  return 0;
}

inline size_t elem_bytes(int type) { return type == kF16 ? 2 : 4; }

// ---------------------------------------------------------------- the host restatement, over bit patterns
// rows [n][width] fp32 bits -> out [n][width] of fp32 bits (kF32) or fp16 bits (kF16)
inline void ref(const uint32_t *rows, int n, int width, const float *log_prior, float floor, int type, void *out) {
  for (size_t r = 0; r < static_cast<size_t>(n); ++r)
    for (int i = 0; i < width; ++i) {
      const float s = score(float_of(rows[r * width + i]), log_prior[i], floor);
      if (type == kF16)
        static_cast<uint16_t *>(out)[r * width + i] = half_bits(s);
      else
        static_cast<uint32_t *>(out)[r * width + i] = bits_of(s);
    }
}

// entries (node_j, p_j): s_j = score(p_j, log_prior[node_j]); a node outside [0, width) gives a NaN and reads nothing
inline void ref_entries(const int32_t *nodes, const uint32_t *p, size_t count, int width, const float *log_prior, float floor, int type, void *out) {
  for (size_t j = 0; j < count; ++j) {
    const bool in = nodes[j] >= 0 && nodes[j] < width;
    const float s = in ? score(float_of(p[j]), log_prior[nodes[j]], floor) : float_of(0x7fc00000u);
    if (type == kF16)
      static_cast<uint16_t *>(out)[j] = half_bits(s);
    else
      static_cast<uint32_t *>(out)[j] = bits_of(s);
  }
}

// ---------------------------------------------------------------- the launch plan
// Rows: a workgroup of kThreads threads takes rows_per_block rows x (kThreads x cols) columns; a thread owns `cols`
// consecutive columns, holds their priors in registers and walks down the rows, kRowsInFlight rows' loads issued before the
// first is used.  rows_per_block is kRowsPerBlock where that still makes kMinBlocks workgroups (the priors are then read
// once per 16 rows), else kRowsInFlight: a 100-frame utterance is spread over the card instead of walked by 56 workgroups.  Vector form: cols = 4 (F32) or 8 (F16), 16-byte loads and stores; it needs width % 4 == 0 and both bases
// on a 16-byte boundary (then every row of the input is, and every row of the output at least on an 8-byte one).  Scalar
// form: cols = 1, any width, element alignment.  No LDS in either.
enum Form { kVector = 0, kScalar = 1 };
constexpr int kThreads = 256;
constexpr int kRowsPerBlock = 16;
constexpr int kRowsInFlight = 4;
constexpr int kMinBlocks = 1024;                 // four workgroups per CU of a 256-CU card
constexpr int kMaxRowsPerLaunch = 1 << 20;       // a longer call goes as several launches
constexpr int kMaxEntriesPerLaunch = 1 << 30;    // entries: one per lane, kThreads a workgroup
static_assert(kRowsPerBlock % kRowsInFlight == 0, "the walk takes whole groups of rows in flight");

inline bool vector_ok(int width, const void *rows, const void *out) {
  return width % 4 == 0 && ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
}
// mode (fdnn_debug_set_loglik_kernel): 0 the rule -- vector where allowed --, 1 the same, 2 always scalar
inline Form form_for(int width, const void *rows, const void *out, int mode) {
  return (mode != 2 && vector_ok(width, rows, out)) ? kVector : kScalar;
}
inline int cols_per_thread(Form f, int type) { return f == kScalar ? 1 : (type == kF16 ? 8 : 4); }

struct Plan {
  Form form;
  int cols;             // columns a thread owns
  int rows_per_block;   // rows a workgroup walks down
  int rows_per_launch;
  int launches;
  int grid_x, grid_y;   // of a full launch: row blocks, column blocks
  int lds_bytes;        // none
};

inline Plan plan(int n, int width, int type, const void *rows, const void *out, int mode) {
  Plan p{form_for(width, rows, out, mode), 0, 0, 0, 0, 0, 0, 0};
  p.cols = cols_per_thread(p.form, type);
  p.rows_per_launch = std::min(std::max(n, 0), kMaxRowsPerLaunch);
  p.launches = p.rows_per_launch ? (n + p.rows_per_launch - 1) / p.rows_per_launch : 0;
  const int chunks = (width + p.cols - 1) / p.cols;
  p.grid_y = (chunks + kThreads - 1) / kThreads;
  const long long blocks16 = static_cast<long long>((p.rows_per_launch + kRowsPerBlock - 1) / kRowsPerBlock) * p.grid_y;
  p.rows_per_block = blocks16 >= kMinBlocks ? kRowsPerBlock : kRowsInFlight;
  p.grid_x = (p.rows_per_launch + p.rows_per_block - 1) / p.rows_per_block;
  return p;
}

}  // namespace loglik
}  // namespace fdnn
