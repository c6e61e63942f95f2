// fdnn_float.hpp -- the UNQUANTIZED net (FeedForwardNetwork.calculate, FeedForwardNetwork.java:133-148, :360-414), the half
// that needs no HIP: the packed fp32 blob, the sizes and extents of a call's activation buffers as pure functions, and the
// plain host restatement of one layer's sums.  fdnn_float.hip holds the kernels, fdnn_float_api.cpp the C-ABI;
// tests/host/float_check.cpp compiles this header (and fdnn_model.cpp's loader) alone, under the sanitizers.
//
// The contract of a layer's sum, for the device and for the restatement alike:
//     s = +0;  for k = 0 .. K-1 ascending: s = fmaf(x[k], w[k], s);  z = s + bias        (a rounding of its own)
// over the TRUE K.  The fp32 MFMA (v_mfma_f32_32x32x2_f32) is bit for bit such a chain, so a row's bytes depend on nothing
// but the row: not on the batch, its position in it, the tile or the chunk.
//
// Padding never changes a sum: a pad column of W holds -0.0f and the pad columns of every activation buffer +0.0f, so a pad
// product is -0 and fmaf(+0, -0, s) = s for EVERY s -- a +0 product would turn an underflowed s = -0 into +0.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace fdnn {
namespace fl {

constexpr int kKStep = 32;         // k extent of one LDS stage of fgemm_kernel: K_pad is a multiple of it
constexpr int kNodeTile = 128;     // nodes per workgroup
constexpr int kFrameTile = 128;    // frames per workgroup
constexpr int kRowPad = 256;       // rows_pad granularity: two node tiles = one 256-node tile of the soft-max total's tree
constexpr int kPartialNodes = 64;  // nodes per partial sum of the soft-max row total
constexpr int kDefaultChunk = 4096;  // frames per internal chunk (fdnn_debug_float_set_chunk)
constexpr int kMaxChunk = 1 << 16;
constexpr int kReportRows = 32;      // rows one report thread adds before its block partial is written
constexpr int kReportCallRows = 4096;  // rows per launch group of fdnn_report_add_device (bounds the block partials)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct LayerDesc {
  uint64_t off_w;     // f32 [rows_pad][K_pad] row-major, k contiguous; pad rows +0, pad columns -0 (see above)
  uint64_t off_bias;  // f32 [rows_pad], pad +0
  int32_t rows, rows_pad, K, K_pad;
};

// Host image of the fp32 net: one blob, 256-byte-aligned sections.
struct FloatHostModel {
  int in_dim = 0;       // padded to x4 with zero weights / shift / scale (float_dnn.cc:32-33): the width of a caller's row
  int in_dim_file = 0;  // as stored in the .bin
  std::vector<LayerDesc> layers;
  uint64_t off_shift = 0, off_scale = 0;  // f32 [K_pad of layer 0], pads +0
  std::vector<uint8_t> blob;
  int out_dim() const { return layers.back().rows; }
  const float *w(int j) const { return reinterpret_cast<const float *>(blob.data() + layers[size_t(j)].off_w); }
  const float *bias(int j) const { return reinterpret_cast<const float *>(blob.data() + layers[size_t(j)].off_bias); }
  const float *shift() const { return reinterpret_cast<const float *>(blob.data() + off_shift); }
  const float *scale() const { return reinterpret_cast<const float *>(blob.data() + off_scale); }
};

// One layer of the .bin as the shared reader hands it over: w [rows][K] dense.
struct DenseLayer {
  int rows = 0, K = 0;
  const float *w = nullptr, *bias = nullptr;
};

// Packs dense layers into the blob.  shift / scale hold layers[0].K floats.
inline void pack(const std::vector<DenseLayer> &layers, const float *shift, const float *scale, int in_dim_file, FloatHostModel *fm) {
  fm->in_dim = layers[0].K;
  fm->in_dim_file = in_dim_file;
  fm->layers.clear();
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
    d.off_w = place(sizeof(float) * size_t(d.rows_pad) * size_t(d.K_pad));
    d.off_bias = place(sizeof(float) * size_t(d.rows_pad));
    fm->layers.push_back(d);
  }
  const size_t k0 = size_t(fm->layers[0].K_pad);
  fm->off_shift = place(sizeof(float) * k0);
  fm->off_scale = place(sizeof(float) * k0);
  fm->blob.assign(off, 0);
  for (size_t j = 0; j < layers.size(); ++j) {
    const LayerDesc &d = fm->layers[j];
    float *w = reinterpret_cast<float *>(fm->blob.data() + d.off_w);
    float *b = reinterpret_cast<float *>(fm->blob.data() + d.off_bias);
    for (int r = 0; r < d.rows; ++r) {
      float *row = w + size_t(r) * size_t(d.K_pad);
      for (int k = 0; k < d.K; ++k) row[k] = layers[j].w[size_t(r) * size_t(d.K) + size_t(k)];
      for (int k = d.K; k < d.K_pad; ++k) row[k] = -0.0f;
      b[r] = layers[j].bias[r];
    }
  }
  float *sh = reinterpret_cast<float *>(fm->blob.data() + fm->off_shift);
  float *sc = reinterpret_cast<float *>(fm->blob.data() + fm->off_scale);
  for (int k = 0; k < fm->in_dim; ++k) sh[k] = shift[k], sc[k] = scale[k];
}

// ---------------------------------------------------------------- a call's buffers, as functions of the shape and the chunk
inline int chunk_rows(int chunk_setting) { return chunk_setting <= 0 ? kDefaultChunk : (chunk_setting > kMaxChunk ? kMaxChunk : chunk_setting); }

struct Shape {          // what the layout depends on
  int k0_pad = 0;       // K_pad of layer 0: row length of the shifted and scaled input
  int act_ld = 0;       // row length of the hidden activations: the widest K_pad of the layers 1 ..
  int out_rows = 0;     // O
  int out_rows_pad = 0;
};
inline Shape shape_of(const FloatHostModel &fm) {
  Shape s;
  s.k0_pad = fm.layers[0].K_pad;
  for (size_t j = 1; j < fm.layers.size(); ++j)
    if (fm.layers[j].K_pad > s.act_ld) s.act_ld = fm.layers[j].K_pad;
  s.out_rows = fm.layers.back().rows;
  s.out_rows_pad = fm.layers.back().rows_pad;
  return s;
}

// Element counts of the buffers a call of n frames needs (n >= 1): every chunk has at most cap = min(n, chunk) frames.
struct Counts {
  int cap = 0;
  size_t xs = 0;       // [cap][k0_pad]
  size_t act = 0;      // each of the two: [cap][act_ld]
  size_t partial = 0;  // [out_rows_pad / 64][cap]
};
inline Counts counts(const Shape &s, int n, int chunk) {
  Counts c;
  c.cap = n < chunk ? n : chunk;
  c.xs = size_t(c.cap) * size_t(s.k0_pad);
  c.act = size_t(c.cap) * size_t(s.act_ld);
  c.partial = size_t(s.out_rows_pad / kPartialNodes) * size_t(c.cap);
  return c;
}

// Chunk i of a call: frames [first, first + rows).
inline int n_chunks(int n, int chunk) { return (n + chunk - 1) / chunk; }
inline void chunk_range(int n, int chunk, int i, int *first, int *rows) {
  *first = i * chunk;
  *rows = n - *first < chunk ? n - *first : chunk;
}

// One past the last element a launch over m frames touches in a buffer of rows `ld` apart of which it reads or writes `cols`.
inline size_t rows_extent(int m, int ld, int cols) { return m <= 0 ? 0 : size_t(m - 1) * size_t(ld) + size_t(cols); }
// ... in the partial sums [groups][ld] of which it writes frames [0, m).
inline size_t partial_extent(int m, int ld, int groups) { return m <= 0 || groups <= 0 ? 0 : size_t(groups - 1) * size_t(ld) + size_t(m); }
// Grid of fgemm_kernel over m frames: (frame tiles, node tiles).  Frames past m are neither read nor written.
inline void gemm_grid(int m, int rows_pad, unsigned *gx, unsigned *gy) {
  *gx = unsigned((m + kFrameTile - 1) / kFrameTile);
  *gy = unsigned(rows_pad / kNodeTile);
}

// ---------------------------------------------------------------- host restatement
// The input step, FeedForwardNetwork.java:121-128: x' = (x + shift) * scale, two roundings.  lin (x + shift) or act may be null.
inline void float_input_ref(const float *shift, const float *scale, int dim, const float *x, int n, float *lin, float *act) {
  for (int f = 0; f < n; ++f)
    for (int k = 0; k < dim; ++k) {
      volatile float t = x[size_t(f) * size_t(dim) + size_t(k)] + shift[k];  // (volatile: the sum exists as an fp32 before the product)
      if (lin) lin[size_t(f) * size_t(dim) + size_t(k)] = t;
      if (act) {
        volatile float p = t * scale[k];
        act[size_t(f) * size_t(dim) + size_t(k)] = p;
      }
    }
}

// One layer's sums: w [rows][ldw], in [n][ld_in], lin [n][rows].  The chain of the contract above, nothing else.
inline void float_layer_ref(const float *w, int ldw, const float *bias, int rows, int K, const float *in, int ld_in, int n, float *lin) {
  for (int f = 0; f < n; ++f) {
    const float *x = in + size_t(f) * size_t(ld_in);
    for (int r = 0; r < rows; ++r) {
      const float *wr = w + size_t(r) * size_t(ldw);
      float s = 0.0f;
      for (int k = 0; k < K; ++k) s = std::fmaf(x[k], wr[k], s);
      volatile float z = s + bias[r];
      lin[size_t(f) * size_t(rows) + size_t(r)] = z;
    }
  }
}

}  // namespace fl

// Loads the fp32 net from a .bin: the reader and the rejections of load_host_model (fdnn_model.cpp), no quantizer.
int load_float_host_model(const std::string &path, fl::FloatHostModel *out, std::string *msg);

}  // namespace fdnn

// ---------------------------------------------------------------- launch interface of fdnn_float.hip
struct ihipStream_t;  // hipStream_t is a pointer to it: this header stays free of HIP

namespace fdnn {
namespace fl {

enum Act { kSigmoid = 0, kExp = 1 };

// act(A[n][K] . W[rows][K]^T + bias) on the fp32 MFMA.
struct GemmParams {
  const float *a;     // [n][lda], columns [0, K_pad) read; pad columns +0
  const float *w;     // [rows_pad][K_pad]
  const float *bias;  // [rows_pad]
  float *out;         // kSigmoid: [n][ldo], columns [rows, ldo) written +0;  kExp: [n][rows] e = exp(z), ldo == rows
  float *tap;         // [n][rows] z = s + bias, or null
  float *partial;     // kExp: [rows_pad / 64][partial_ld] the 64-node partial sums of e; else null
  int n, rows, rows_pad, K_pad, lda, ldo, partial_ld;
};
void launch_fgemm(const GemmParams &p, Act act, ihipStream_t *s);
// xs[f][k] = (x[f][k] + shift[k]) * scale[k] for k < dim, +0 for dim <= k < ld; lin [n][dim] receives x + shift unless null
void launch_input_step(const float *x, const float *shift, const float *scale, float *xs, float *lin, int n, int dim, int ld, ihipStream_t *s);

// The report's device state: u64 cnt[3] = frames, NaN rows, rows whose top-1 agree; node_sum / node_max [O] doubles.
struct ReportParams {
  const float *ref, *q;        // [n][O]
  int n, O;
  unsigned char *row_nan;      // [n] scratch
  double *blk_sum, *blk_max;   // [ceil(n / kReportRows)][O] scratch
  unsigned long long *cnt;     // [3]
  double *node_sum, *node_max; // [O]
};
void launch_report(const ReportParams &p, ihipStream_t *s);  // n <= kReportCallRows
// fgemm sigmoid, exp, sigmoid + tap, exp + tap, input step, report rows, report nodes, report fold
constexpr int kLaunchKinds = 8;
void launch_counts(unsigned long long out[kLaunchKinds]);

}  // namespace fl
}  // namespace fdnn
