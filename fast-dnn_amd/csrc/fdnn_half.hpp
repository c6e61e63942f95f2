// fdnn_half.hpp -- the HALF-PRECISION net: fp16 weights and activations on v_mfma_f32_32x32x16_f16, fp32 sums, fp32 sigmoid
// and soft-max.  The half that needs no HIP: the contract, the packed blob, the buffer extents of a call as pure
// functions, the fp32 <-> fp16 conversions of the host.  fdnn_half.hip holds the kernels, fdnn_half_api.cpp the C-ABI.
// What is independent of the element type (LayerDesc, DenseLayer, Shape, counts, chunk_range, the extents) is
// fdnn_float.hpp's, used as it stands.
//
// THE CONTRACT
//   weights      the .bin's fp32 weights rounded ONCE at load to fp16, round to nearest even (numpy's astype(float16)),
//                subnormal halves kept.  A weight that rounds to +-inf refuses the load (FDNN_E_FORMAT, naming layer and
//                node).  Biases, shift and scale stay fp32.
//   input step   t = RN32(x + shift), v = RN32(t * scale) -- the float net's two roundings -- then ONE rounding to fp16.
//                Whatever that gives (+-inf, a NaN) stays in its own row.
//   a layer      s = sum over k of x[k] w[k]: a product of two halves is exact in fp32 (22 significant bits), the sum is
//                accumulated in fp32 by the MFMA, 16 k per instruction, k-steps ascending, ONE accumulator chain per
//                output (no split-K, no per-wave k halves), accumulators starting at +0.  Then z = RN32(s + bias).
//                A row's bytes are a function of the row and the model alone: not of n, its position, the tile, the chunk.
//                The order of the additions INSIDE one instruction is the hardware's and is not documented, so there is NO
//                byte-for-byte host restatement of a sum here (the float net has one: its instruction adds two terms in a
//                stated order).  The device is held to float64 on its own fp16 operands under
//                    |z - z64| <= g'(K + 1) (sum |x w| + |b|) + K 2^-126,  g'(m) = m u' / (1 - m u'),  u' = 2^-23
//                (Higham's any-order bound with a whole ulp per addition: it covers an adder that truncates when it aligns
//                the terms of an instruction) and to its own invariance.
//   hidden act   the float kernel's fp32 sequence e = exp2(RN(-z RN32(log2 e))), d = RN(1 + e), sg = 1 / d (IEEE), then one
//                rounding to fp16.  The activation buffers are fp16.
//   output       e = exp2(RN(z RN32(log2 e))) in fp32, unstabilised; the 64-node partial sums in the layout and the order
//                (32 + 32 sequential additions, then the halves) that launch_normalize assumes; launch_normalize; fp32
//                probabilities [n][O].  A logit above 88.72 gives its entry NaN and the rest of its row 0.
//   padding      never changes a sum: the pad COLUMNS of W hold the half -0 (0x8000), the pad columns of every activation
//                buffer +0, so a pad product is the fp32 -0, and adding -0 leaves every s as it is -- a +0 product would
//                turn an s = -0 (all true products -0 or underflowed) into +0.  Pad rows of W and pad biases are +0; their
//                outputs are never stored (hidden pad activations are written +0).  Pad frames are neither read nor written.
//   subnormals   a product with a subnormal half operand counts: gfx950's fp16 MFMA does not flush its inputs (measured,
//                tests/test_gpu_half.py::test_subnormal_halves_count).
#pragma once
#include <cstring>

#include "fdnn_float.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FDNN_HALF_HD __host__ __device__ __forceinline__
#else
#define FDNN_HALF_HD inline
#endif

namespace fdnn {
namespace hf {

using fl::align_up;
using fl::chunk_range;
using fl::chunk_rows;
using fl::Counts;
using fl::counts;
using fl::DenseLayer;
using fl::kKStep;          // K_pad granularity: one LDS stage of hgemm_kernel is 32 k = two MFMAs deep
using fl::kPartialNodes;
using fl::kRowPad;         // rows_pad granularity: two node tiles
using fl::LayerDesc;       // off_w: f16 [rows_pad][K_pad] here; off_bias: f32 [rows_pad]
using fl::n_chunks;
using fl::partial_extent;
using fl::rows_extent;
using fl::Shape;

constexpr int kNodeTile = 128;   // nodes per workgroup
constexpr int kFrameTile = 256;  // frames per workgroup
constexpr uint16_t kNegZero = 0x8000;

// fp32 -> fp16 bits, round to nearest even, subnormal halves kept, NaN stays NaN (quiet), overflow -> +-inf.  ONE function for
// the loader, the debug call's rows and the device's input step: there the compiler would otherwise fuse the fp32 product
// and a conversion into v_fma_mixlo_f16, which rounds the exact product ONCE, to fp16 -- not the contract's three roundings.
FDNN_HALF_HD uint16_t half_bits(float f) {
  uint32_t x;
  __builtin_memcpy(&x, &f, 4);
  const uint16_t sign = uint16_t((x >> 16) & 0x8000u);
  x &= 0x7fffffffu;
  if (x > 0x7f800000u) return uint16_t(sign | 0x7e00u | ((x >> 13) & 0x3ffu));
  if (x >= 0x47800000u) return uint16_t(sign | 0x7c00u);  // 65536 and above (65520 .. 65536 carries into 0x7c00 below)
  if (x < 0x38800000u) {
    // below 2^-14: |f| + 0.5 rounds (to nearest even, one fp32 addition) to a multiple of ulp(0.5) = 2^-24, the step of the
    // subnormal halves; the multiple is the result's bits (0x400 = the smallest normal half included)
    float a;
    __builtin_memcpy(&a, &x, 4);
    const float t = a + 0.5f;
    uint32_t y;
    __builtin_memcpy(&y, &t, 4);
    return uint16_t(sign | (y - 0x3f000000u));
  }
  x += 0xfffu + ((x >> 13) & 1u);  // half an ulp of the half, less one when the kept bit is even
  return uint16_t(sign | ((x - 0x38000000u) >> 13));
}

// fp16 bits -> fp32, exact.
inline float half_value(uint16_t h) {
  const uint32_t sign = uint32_t(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t x;
  if (e == 0x1fu) x = sign | 0x7f800000u | (m << 13);
  else if (e != 0) x = sign | ((e + 112u) << 23) | (m << 13);
  else {
    const float v = float(m) * 5.9604644775390625e-8f;  // m 2^-24, exact
    std::memcpy(&x, &v, 4);
    x |= sign;
  }
  float f;
  std::memcpy(&f, &x, 4);
  return f;
}

// Host image of the half net: one blob, 256-byte-aligned sections.
struct HalfHostModel {
  int in_dim = 0;       // padded to x4, as the float net's
  int in_dim_file = 0;
  std::vector<LayerDesc> layers;
  uint64_t off_shift = 0, off_scale = 0;  // f32 [K_pad of layer 0], pads +0
  std::vector<uint8_t> blob;
  int out_dim() const { return layers.back().rows; }
  const uint16_t *w(int j) const { return reinterpret_cast<const uint16_t *>(blob.data() + layers[size_t(j)].off_w); }
  const float *bias(int j) const { return reinterpret_cast<const float *>(blob.data() + layers[size_t(j)].off_bias); }
};

// Packs dense fp32 layers into the blob, rounding the weights.  Returns false, naming the place in *msg, where a weight
// rounds to +-inf.
inline bool pack(const std::vector<DenseLayer> &layers, const float *shift, const float *scale, int in_dim_file, HalfHostModel *hm,
                 std::string *msg) {
  hm->in_dim = layers[0].K;
  hm->in_dim_file = in_dim_file;
  hm->layers.clear();
  size_t off = 0;
  auto place = [&](size_t bytes) {
    const size_t o = off;
    off = align_up(off + bytes, 256);
    return uint64_t(o);
  };
  for (const DenseLayer &L : layers) {
    LayerDesc d{};
    d.rows = L.rows;
    d.K = L.K;
    d.rows_pad = int32_t(align_up(size_t(L.rows), kRowPad));
    d.K_pad = int32_t(align_up(size_t(L.K), kKStep));
    d.off_w = place(sizeof(uint16_t) * size_t(d.rows_pad) * size_t(d.K_pad));
    d.off_bias = place(sizeof(float) * size_t(d.rows_pad));
    hm->layers.push_back(d);
  }
  const size_t k0 = size_t(hm->layers[0].K_pad);
  hm->off_shift = place(sizeof(float) * k0);
  hm->off_scale = place(sizeof(float) * k0);
  hm->blob.assign(off, 0);
  for (size_t j = 0; j < layers.size(); ++j) {
    const LayerDesc &d = hm->layers[j];
    uint16_t *w = reinterpret_cast<uint16_t *>(hm->blob.data() + d.off_w);
    float *b = reinterpret_cast<float *>(hm->blob.data() + d.off_bias);
    for (int r = 0; r < d.rows; ++r) {
      uint16_t *row = w + size_t(r) * size_t(d.K_pad);
      for (int k = 0; k < d.K; ++k) {
        const float v = layers[j].w[size_t(r) * size_t(d.K) + size_t(k)];
        row[k] = half_bits(v);
        if ((row[k] & 0x7fffu) == 0x7c00u) {
          *msg = "half net: the weight of layer " + std::to_string(j) + ", node " + std::to_string(r) + ", input " + std::to_string(k) + " (" +
                 std::to_string(v) + ") rounds to an infinite fp16";
          return false;
        }
      }
      for (int k = d.K; k < d.K_pad; ++k) row[k] = kNegZero;
      b[r] = layers[j].bias[r];
    }
  }
  float *sh = reinterpret_cast<float *>(hm->blob.data() + hm->off_shift);
  float *sc = reinterpret_cast<float *>(hm->blob.data() + hm->off_scale);
  for (int k = 0; k < hm->in_dim; ++k) sh[k] = shift[k], sc[k] = scale[k];
  return true;
}

inline Shape shape_of(const HalfHostModel &hm) {
  Shape s;
  s.k0_pad = hm.layers[0].K_pad;
  for (size_t j = 1; j < hm.layers.size(); ++j)
    if (hm.layers[j].K_pad > s.act_ld) s.act_ld = hm.layers[j].K_pad;
  s.out_rows = hm.layers.back().rows;
  s.out_rows_pad = hm.layers.back().rows_pad;
  return s;
}

// Grid of hgemm_kernel over m frames: (frame tiles, node tiles).  Frames past m are neither read nor written.
inline void gemm_grid(int m, int rows_pad, unsigned *gx, unsigned *gy) {
  *gx = unsigned((m + kFrameTile - 1) / kFrameTile);
  *gy = unsigned(rows_pad / kNodeTile);
}

}  // namespace hf

// Loads the half net from a .bin: the reader and the rejections of load_host_model (fdnn_model.cpp), then hf::pack.
int load_half_host_model(const std::string &path, hf::HalfHostModel *out, std::string *msg);

}  // namespace fdnn

// ---------------------------------------------------------------- launch interface of fdnn_half.hip
namespace fdnn {
namespace hf {

enum Act { kSigmoid = 0, kExp = 1 };

// act(A[n][K] . W[rows][K]^T + bias) on the fp16 MFMA.
struct GemmParams {
  const uint16_t *a;  // f16 [n][lda], columns [0, K_pad) read; pad columns +0
  const uint16_t *w;  // f16 [rows_pad][K_pad]
  const float *bias;  // [rows_pad]
  uint16_t *act;      // kSigmoid: f16 [n][ldo], columns [rows, ldo) written +0; ldo a multiple of 4
  float *e;           // kExp: [n][rows] e = exp(z)
  float *tap;         // [n][rows] z = s + bias, or null
  float *partial;     // kExp: [rows_pad / 64][partial_ld] the 64-node partial sums of e
  int n, rows, rows_pad, K_pad, lda, ldo, partial_ld;
};
void launch_hgemm(const GemmParams &p, Act act, ihipStream_t *s);
// xs[f][k] = f16((x[f][k] + shift[k]) * scale[k]) for k < dim, +0 for dim <= k < ld; lin [n][dim] receives x + shift unless null
void launch_half_input_step(const float *x, const float *shift, const float *scale, uint16_t *xs, float *lin, int n, int dim, int ld,
                            ihipStream_t *s);
// hgemm sigmoid, exp, sigmoid + tap, exp + tap, input step
constexpr int kLaunchKinds = 5;
void launch_counts(unsigned long long out[kLaunchKinds]);

// ---------------------------------------------------------------- the small-batch kernel (fdnn_half_small.hip)
// A call of 1 .. kSmallMaxFrames frames may take hsmall_kernel instead of hgemm_kernel: one workgroup per node tile and
// all the call's frames, the weights streamed through a deep LDS ring.  THE CONTRACT above holds unchanged: the same
// instruction, operand roles, k order and epilogue, so a row has the bytes hgemm_kernel gives it.
constexpr int kSmallMaxFrames = 128;
#ifndef FDNN_HSMALL_HIDDEN_TILES
#define FDNN_HSMALL_HIDDEN_TILES 1  // (a build switch for the measurement of section 33 only)
#endif
constexpr int kSmallHiddenTiles = FDNN_HSMALL_HIDDEN_TILES;  // 32-node tiles per hidden workgroup; the output form has 2: a 64-node partial
// The rule.  n is the CALL's frame count, setting the model's (0 = off): every chunk of a small call is small.
inline bool small_applies(int n, int setting) { return n >= 1 && n <= setting && setting <= kSmallMaxFrames; }
inline int small_frame_tiles(int m) { return (m + 31) / 32; }
// Workgroups of hsmall_kernel over a layer: one per node tile, whatever the frame count.
inline unsigned small_grid(int rows_pad, Act act) { return unsigned(rows_pad / (32 * (act == kExp ? 2 : kSmallHiddenTiles))); }
void launch_hsmall(const GemmParams &p, Act act, ihipStream_t *s);
// small sigmoid, exp, sigmoid + tap, exp + tap
constexpr int kSmallLaunchKinds = 4;
void small_launch_counts(unsigned long long out[kSmallLaunchKinds]);

// ---------------------------------------------------------------- the mid-batch kernel (fdnn_half_mid.hip)
// A call of up to kMidMaxFrames frames that is not small may take hmid_kernel instead of hgemm_kernel: 64 frames x 64 nodes
// per workgroup, two workgroups to a CU, the operands requested two stages ahead.  THE CONTRACT above holds unchanged: a row
// has the bytes hgemm_kernel gives it.
constexpr int kMidMaxFrames = 4096;  // the default chunk: such a call is one chunk unless the chunk was set smaller
constexpr int kMidFrameTile = 64;    // frames per workgroup
constexpr int kMidNodeTile = 64;     // nodes per workgroup: one soft-max partial
// The rule.  n is the CALL's frame count, the settings the model's (0 = off).  The small kernel keeps its own range.
inline bool mid_applies(int n, int small_setting, int mid_setting) {
  return n >= 1 && n <= mid_setting && mid_setting <= kMidMaxFrames && !small_applies(n, small_setting);
}
// Grid of hmid_kernel over m frames: (frame tiles, node tiles).  Frames past m are neither read from memory nor written.
inline void mid_grid(int m, int rows_pad, unsigned *gx, unsigned *gy) {
  *gx = unsigned((m + kMidFrameTile - 1) / kMidFrameTile);
  *gy = unsigned(rows_pad / kMidNodeTile);
}
void launch_hmid(const GemmParams &p, Act act, ihipStream_t *s);
// mid sigmoid, exp, sigmoid + tap, exp + tap
constexpr int kMidLaunchKinds = 4;
void mid_launch_counts(unsigned long long out[kMidLaunchKinds]);

// ---------------------------------------------------------------- the large-batch kernel (fdnn_half_large.hip)
// A call of large_setting frames or more that is neither small nor mid may take hlarge_kernel instead of hgemm_kernel: the
// same 256 x 128 tile and grid (gemm_grid), the operands requested 128 k ahead through a three-stage LDS ring.  THE CONTRACT
// above holds unchanged: a row has the bytes hgemm_kernel gives it.
constexpr int kLargeMaxSetting = fl::kMaxChunk;  // fdnn_half_model_set_large takes 0 (off) .. this
// The rule.  n is the CALL's frame count, the settings the model's (0 = off): small, then mid, then large, then tiled.  Every
// chunk of a large call is large, the tail included.
inline bool large_applies(int n, int small_setting, int mid_setting, int large_setting) {
  return large_setting >= 1 && n >= large_setting && !small_applies(n, small_setting) && !mid_applies(n, small_setting, mid_setting);
}
void launch_hlarge(const GemmParams &p, Act act, ihipStream_t *s);
// large sigmoid, exp, sigmoid + tap, exp + tap
constexpr int kLargeLaunchKinds = 4;
void large_launch_counts(unsigned long long out[kLargeLaunchKinds]);

}  // namespace hf
}  // namespace fdnn
