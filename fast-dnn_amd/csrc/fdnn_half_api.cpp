// fdnn_half_api.cpp -- C-ABI of the half-precision net (include/fdnn.h, last section; contract: fdnn_half.hpp): the model
// object, the chunk loop over fdnn_half.hip's launches, the host ends of the per-layer debug call, and the lazy output for
// per-segment node sets (contract: fdnn_half_set.hpp): the hidden layers as they are, then the set step on every chunk's slice.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>

#include "fdnn_half.hpp"
#include "fdnn_half_set.hpp"
#include "fdnn_internal.hpp"
#include "fdnn_stream_order.hpp"

using fdnn::DevBuf;
using fdnn::device_ok;
using fdnn::DeviceGuard;
using fdnn::fail;
namespace hf = fdnn::hf;
namespace hset = fdnn::hset;
namespace sets = fdnn::sets;

struct fdnn_half_model {
  hf::HalfHostModel hm;
  hf::Shape shape;
  int device = 0;
  int chunk = 0;  // fdnn_debug_half_set_chunk (0 = default)
  int small = 0;  // fdnn_half_model_set_small: calls of 1 .. small frames take hsmall_kernel (0 = off)
  int mid = 0;    // fdnn_half_model_set_mid: calls of up to mid frames that are not small take hmid_kernel (0 = off)
  int large = 0;  // fdnn_half_model_set_large: calls of large frames and more that are neither take hlarge_kernel (0 = off)
  std::mutex mu;
  fdnn::StreamOrder order;
  DevBuf<uint8_t> d_blob;
  DevBuf<uint16_t> d_xs, d_act[2];  // hf::counts: f16 [cap][k0_pad], [cap][act_ld]
  DevBuf<float> d_partial;
  DevBuf<float> d_x, d_out;         // the host entry points' copies: [n][in_dim], [n][O]
  DevBuf<uint16_t> d_in, d_dbg;     // fdnn_debug_half_layer: f16 [n][K_pad], [n][ldo]
  DevBuf<float> d_lin, d_prob;      // ... z [n][rows], and the last layer's rows [n][O]
  DevBuf<int32_t> d_srow;           // the set step: a chunk's ragged row pointer [cap + 1]
  DevBuf<float> d_se, d_sz;         // ... and its fallback's dense e and tap [cap][O]
  DevBuf<int32_t> d_snodes;         // the host set entries' copies: nodes,
  DevBuf<float> d_sprobs, d_sinact, d_slin;  // probs, inactive [n] and the debug call's ragged z
  const uint16_t *w(int j) const { return reinterpret_cast<const uint16_t *>(d_blob.p + hm.layers[size_t(j)].off_w); }
  const float *bias(int j) const { return reinterpret_cast<const float *>(d_blob.p + hm.layers[size_t(j)].off_bias); }
  const float *shift() const { return reinterpret_cast<const float *>(d_blob.p + hm.off_shift); }
  const float *scale() const { return reinterpret_cast<const float *>(d_blob.p + hm.off_scale); }
  int n_layers() const { return int(hm.layers.size()); }
};

namespace {

int reserve_call(fdnn_half_model *m, int n) {
  const hf::Counts c = hf::counts(m->shape, n, hf::chunk_rows(m->chunk));
  HIP_TRY(m->d_xs.reserve(c.xs));
  HIP_TRY(m->d_act[0].reserve(c.act));
  HIP_TRY(m->d_act[1].reserve(c.act));
  HIP_TRY(m->d_partial.reserve(c.partial));
  return FDNN_OK;
}

// One layer over m frames of one chunk of a call of n frames.  A hidden layer writes halves to act (rows ldo apart); the
// last one e and the partials to probs [m][rows], then the scale pass.  The one place that picks the GEMM's launcher:
// hf::small_applies, then hf::mid_applies, then hf::large_applies, on the CALL's n, so every chunk of a small call is small
// (m <= n <= kSmallMaxFrames), every chunk of a mid call is mid and every chunk of a large call is large, the tail included.
void run_layer(fdnn_half_model *hm, int j, const uint16_t *in, int lda, int m, int n, int cap, uint16_t *act, int ldo, float *probs,
               float *tap, hipStream_t s, bool normalize = true) {
  const hf::LayerDesc &d = hm->hm.layers[size_t(j)];
  const bool last = j + 1 == hm->n_layers();
  hf::GemmParams p{};
  p.a = in;
  p.w = hm->w(j);
  p.bias = hm->bias(j);
  p.act = last ? nullptr : act;
  p.e = last ? probs : nullptr;
  p.tap = tap;
  p.partial = last ? hm->d_partial.p : nullptr;
  p.n = m;
  p.rows = d.rows;
  p.rows_pad = d.rows_pad;
  p.K_pad = d.K_pad;
  p.lda = lda;
  p.ldo = last ? d.rows : ldo;
  p.partial_ld = cap;
  if (hf::small_applies(n, hm->small)) hf::launch_hsmall(p, last ? hf::kExp : hf::kSigmoid, s);
  else if (hf::mid_applies(n, hm->small, hm->mid)) hf::launch_hmid(p, last ? hf::kExp : hf::kSigmoid, s);
  else if (hf::large_applies(n, hm->small, hm->mid, hm->large)) hf::launch_hlarge(p, last ? hf::kExp : hf::kSigmoid, s);
  else hf::launch_hgemm(p, last ? hf::kExp : hf::kSigmoid, s);
  if (last && normalize) fdnn::launch_normalize(probs, probs, hm->d_partial, m, cap, d.rows, d.rows_pad / hf::kPartialNodes, s);
}

// A call with node sets: the caller's host tables over the call's rows [0, n) and its device buffers.
struct SetCall {
  sets::Tables t;
  const int32_t *d_nodes;
  float *d_probs, *d_inactive;  // the ragged blocks, one value per row
  float *d_z;                   // the ragged logits (fdnn_debug_half_set_layer), or null
};

// The output layer on the listed nodes of the chunk [first, first + m) of a call of n frames, in: the chunk's last hidden rows.
// sets::slice cuts the tables to the chunk: a segment cut by the boundary keeps its set, and its block goes on where the
// chunk before left it (src_off).  Then the list path's finish pass over the slice's row pointer, written on the device.
int set_step(fdnn_half_model *hm, const uint16_t *in, int lda, int first, int m, int n, int cap, const SetCall &sc, hipStream_t s) {
  const int last = hm->n_layers() - 1;
  const hf::LayerDesc &d = hm->hm.layers[size_t(last)];
  const std::vector<sets::Seg> segs = sets::slice(sc.t, first, first + m);
  if (segs.empty()) return FDNN_OK;  // (the tables cover [0, n): every chunk has a segment)
  long long nnz = 0;
  for (const sets::Seg &g : segs) nnz += static_cast<long long>(g.rows) * g.len;
  const std::vector<sets::Launch> launches = hset::plan(segs, fdnn::device_cus(hm->device));
  for (size_t i = 0; i < launches.size(); ++i) fdnn::launch_sets_rows(launches[i], hm->d_srow, nullptr, i + 1 == launches.size() ? m : -1, int(nnz), s);
  hset::Params p{};
  p.a = in;
  p.w = hm->w(last);
  p.bias = hm->bias(last);
  p.nodes = sc.d_nodes;
  p.probs = sc.d_probs ? sc.d_probs + segs[0].src_off : nullptr;
  p.z = sc.d_z ? sc.d_z + segs[0].src_off : nullptr;
  p.rows = d.rows;
  p.rows_pad = d.rows_pad;
  p.K_pad = d.K_pad;
  p.lda = lda;
  if (nnz > 0 && hset::applies(d.K_pad, d.rows_pad, lda, m)) {
    for (const sets::Launch &l : launches) hset::launch_score(p, l, s);
  } else if (nnz > 0) {
    // the fallback: the chunk's dense exp launch without the scale pass, then the listed entries out of it
    run_layer(hm, last, in, lda, m, n, cap, nullptr, d.rows, hm->d_se, sc.d_z ? hm->d_sz.p : nullptr, s, false);
    for (const sets::Launch &l : launches) hset::launch_gather(p, hm->d_se, sc.d_z ? hm->d_sz.p : nullptr, l, s);
  }
  fdnn::ListsParams g{};
  g.row_ptr = hm->d_srow;
  g.probs = p.probs;
  g.inactive = sc.d_inactive + first;
  g.count = m;
  g.nnz = int(nnz);
  g.rows = d.rows;
  fdnn::launch_lists_finish(g, s);
  return FDNN_OK;
}

// What the set step needs beside reserve_call's buffers (a buffer that is too small is freed and allocated anew, which waits
// for the device: earlier calls have finished).
int reserve_sets(fdnn_half_model *hm, int n, bool z) {
  const int cap = std::min(n, hf::chunk_rows(hm->chunk));
  const hf::LayerDesc &d = hm->hm.layers.back();
  HIP_TRY(hm->d_srow.reserve(size_t(cap) + 1));
  if (hset::applies(d.K_pad, d.rows_pad, d.K_pad, cap)) return FDNN_OK;
  HIP_TRY(hm->d_se.reserve(size_t(cap) * d.rows));
  if (z) HIP_TRY(hm->d_sz.reserve(size_t(cap) * d.rows));
  return FDNN_OK;
}

// The whole net on device rows d_x [n][in_dim] -> d_out [n][O], chunk by chunk -- or, with sc, the hidden layers and the set
// step in place of the last layer: such a call never launches the dense output layer (but in the set step's fallback).
int run_net(fdnn_half_model *hm, const float *d_x, int n, float *d_out, hipStream_t s, const SetCall *sc = nullptr) {
  if (int rc = reserve_call(hm, n)) return rc;
  if (sc)
    if (int rc = reserve_sets(hm, n, false)) return rc;
  const int chunk = hf::chunk_rows(hm->chunk), cap = std::min(n, chunk), L = hm->n_layers();
  const int D = hm->hm.in_dim, O = hm->hm.out_dim();
  for (int i = 0; i < hf::n_chunks(n, chunk); ++i) {
    int first, m;
    hf::chunk_range(n, chunk, i, &first, &m);
    hf::launch_half_input_step(d_x + size_t(first) * D, hm->shift(), hm->scale(), hm->d_xs, nullptr, m, D, hm->shape.k0_pad, s);
    const uint16_t *in = hm->d_xs;
    int lda = hm->shape.k0_pad;
    for (int j = 0; j < L; ++j) {
      const bool last = j + 1 == L;
      if (last && sc) {
        if (int rc = set_step(hm, in, lda, first, m, n, cap, *sc, s)) return rc;
        break;
      }
      const int ldo = last ? O : hm->hm.layers[size_t(j) + 1].K_pad;
      run_layer(hm, j, in, lda, m, n, cap, hm->d_act[j & 1].p, ldo, last ? d_out + size_t(first) * O : nullptr, nullptr, s);
      in = hm->d_act[j & 1].p;
      lda = ldo;
    }
  }
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

// fdnn_debug_half_layer and its timing twin: a hidden layer's output row length, the caller's fp32 rows [n][K] rounded to
// halves into d_in [n][K_pad] (pad columns +0, as every activation buffer has them), and the layer over them chunk by chunk.
int layer_ldo(const fdnn_half_model *hm, int j) { return int(hf::align_up(size_t(hm->hm.layers[size_t(j)].rows), hf::kKStep)); }

int layer_upload(fdnn_half_model *hm, int j, const float *in, int n, bool tap) {
  const hf::LayerDesc &d = hm->hm.layers[size_t(j)];
  const bool last = j + 1 == hm->n_layers();
  if (int rc = reserve_call(hm, n)) return rc;
  std::vector<uint16_t> padded(size_t(n) * size_t(d.K_pad), 0);
  for (int f = 0; f < n; ++f)
    for (int k = 0; k < d.K; ++k) padded[size_t(f) * d.K_pad + k] = hf::half_bits(in[size_t(f) * d.K + k]);
  HIP_TRY(hm->d_in.reserve(padded.size()));
  if (tap) HIP_TRY(hm->d_lin.reserve(size_t(n) * d.rows));
  if (last) HIP_TRY(hm->d_prob.reserve(size_t(n) * d.rows));
  else HIP_TRY(hm->d_dbg.reserve(size_t(n) * layer_ldo(hm, j)));
  HIP_TRY(hipMemcpy(hm->d_in, padded.data(), sizeof(uint16_t) * padded.size(), hipMemcpyHostToDevice));
  return FDNN_OK;
}

void layer_launch(fdnn_half_model *hm, int j, int n, bool tap) {
  const hf::LayerDesc &d = hm->hm.layers[size_t(j)];
  const bool last = j + 1 == hm->n_layers();
  const int chunk = hf::chunk_rows(hm->chunk), cap = std::min(n, chunk), ldo = layer_ldo(hm, j);
  for (int i = 0; i < hf::n_chunks(n, chunk); ++i) {
    int first, m;
    hf::chunk_range(n, chunk, i, &first, &m);
    run_layer(hm, j, hm->d_in + size_t(first) * d.K_pad, d.K_pad, m, n, cap, last ? nullptr : hm->d_dbg + size_t(first) * ldo, ldo,
              last ? hm->d_prob + size_t(first) * d.rows : nullptr, tap ? hm->d_lin + size_t(first) * d.rows : nullptr, nullptr);
  }
}

// Halves [n][ld] on the device -> the caller's fp32 [n][cols], widened on the host (exact).
int halves_to_host(const uint16_t *d_src, int n, int ld, int cols, float *dst) {
  std::vector<uint16_t> h(size_t(n) * size_t(ld));
  HIP_TRY(hipMemcpy(h.data(), d_src, sizeof(uint16_t) * h.size(), hipMemcpyDeviceToHost));  // (the null stream's work first)
  for (int f = 0; f < n; ++f)
    for (int k = 0; k < cols; ++k) dst[size_t(f) * cols + k] = hf::half_value(h[size_t(f) * ld + k]);
  return FDNN_OK;
}

// The checks every set entry shares once its tables hold: they cover [0, n) and the blocks fit an int32.
int sets_cover(const sets::Tables &t, int n) {
  if (t.n_segs == 0 ? n != 0 : (t.seg_rows[0] != 0 || t.seg_rows[t.n_segs] != n)) return fail(FDNN_E_ARG, "seg_rows must cover the rows [0, n)");
  if (sets::total(t) > INT32_MAX) return fail(FDNN_E_ARG, "the sum of rows x len over the segments must fit an int32");
  return FDNN_OK;
}

int sets_named(int bad, int output_dim, int n) {
  return fail(FDNN_E_ARG, "node sets, segment " + std::to_string(-bad - 1) + ": seg_rows must not decrease inside [0, " + std::to_string(n) +
                              "], set_ptr must begin at 0 and not decrease, a set's nodes must ascend strictly inside [0, " +
                              std::to_string(output_dim) + ")");
}

// The host forms: copies in, run_net with the sets, copies out.  The tables have been validated.
int host_sets(fdnn_half_model *hm, const float *x, int n, int dim, const sets::Tables &t, const int32_t *nodes, float *probs, float *inactive) {
  if (dim != hm->hm.in_dim)
    return fail(FDNN_E_ARG, "input vector size " + std::to_string(dim) + " must be equal with network input size " + std::to_string(hm->hm.in_dim));
  if (int rc = sets_cover(t, n)) return rc;
  if (n == 0) return FDNN_OK;
  const size_t nnz = size_t(sets::total(t)), n_nodes = size_t(t.set_ptr[t.n_segs]);
  if (!x || !inactive || (nnz > 0 && !probs)) return fail(FDNN_E_ARG, "null buffer");
  std::lock_guard<std::mutex> lk(hm->mu);
  DeviceGuard g(hm->device);
  HIP_TRY(hm->order.enter(nullptr));
  HIP_TRY(hm->d_x.reserve(size_t(n) * size_t(dim)));
  HIP_TRY(hm->d_snodes.reserve(std::max<size_t>(n_nodes, 1)));
  HIP_TRY(hm->d_sprobs.reserve(std::max<size_t>(nnz, 1)));
  HIP_TRY(hm->d_sinact.reserve(size_t(n)));
  HIP_TRY(hipMemcpyAsync(hm->d_x, x, sizeof(float) * size_t(n) * size_t(dim), hipMemcpyHostToDevice, nullptr));
  if (n_nodes) HIP_TRY(hipMemcpyAsync(hm->d_snodes, nodes, sizeof(int32_t) * n_nodes, hipMemcpyHostToDevice, nullptr));
  const SetCall sc{t, hm->d_snodes, hm->d_sprobs, hm->d_sinact, nullptr};
  if (int rc = run_net(hm, hm->d_x, n, nullptr, nullptr, &sc)) return rc;
  if (nnz) HIP_TRY(hipMemcpyAsync(probs, hm->d_sprobs, sizeof(float) * nnz, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipMemcpyAsync(inactive, hm->d_sinact, sizeof(float) * size_t(n), hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hm->order.leave(nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  return FDNN_OK;
}

}  // namespace

extern "C" {

int fdnn_half_model_load_on(const char *path, int device, fdnn_half_model **out) {
  if (!path || !out) return fail(FDNN_E_ARG, "null argument");
  *out = nullptr;
  std::unique_ptr<fdnn_half_model> hm(new fdnn_half_model());
  std::string msg;
  if (int rc = fdnn::load_half_host_model(path, &hm->hm, &msg)) return fail(rc, msg);
  if (int rc = device_ok(device)) return rc;
  hm->device = device;
  hm->shape = hf::shape_of(hm->hm);
  DeviceGuard g(device);
  if (!g.ok) return fail(FDNN_E_DEVICE, "hipSetDevice failed");
  HIP_TRY(hm->d_blob.reserve(hm->hm.blob.size()));
  HIP_TRY(hipMemcpy(hm->d_blob, hm->hm.blob.data(), hm->hm.blob.size(), hipMemcpyHostToDevice));
  *out = hm.release();
  return FDNN_OK;
}

int fdnn_half_model_load(const char *path, fdnn_half_model **out) { return fdnn_half_model_load_on(path, 0, out); }

void fdnn_half_model_free(fdnn_half_model *hm) {
  if (!hm) return;
  DeviceGuard g(hm->device);
  hipDeviceSynchronize();
  delete hm;
}

int fdnn_half_model_input_dim(const fdnn_half_model *hm) { return hm ? hm->hm.in_dim : -1; }
int fdnn_half_model_output_dim(const fdnn_half_model *hm) { return hm ? hm->hm.out_dim() : -1; }
int fdnn_half_model_layer_count(const fdnn_half_model *hm) { return hm ? hm->n_layers() : -1; }
int fdnn_half_model_layer_dim(const fdnn_half_model *hm, int index) {
  return hm && index >= 0 && index < hm->n_layers() ? hm->hm.layers[size_t(index)].rows : -1;
}
int fdnn_half_model_device(const fdnn_half_model *hm) { return hm ? hm->device : -1; }

int fdnn_debug_half_set_chunk(fdnn_half_model *hm, int rows) {
  if (!hm || rows < 0 || rows > fdnn::fl::kMaxChunk)
    return fail(FDNN_E_ARG, "chunk rows are 0 (default) .. " + std::to_string(fdnn::fl::kMaxChunk));
  std::lock_guard<std::mutex> lk(hm->mu);
  hm->chunk = rows;
  return FDNN_OK;
}

int fdnn_half_model_set_small(fdnn_half_model *hm, int max_frames) {
  if (!hm || max_frames < 0 || max_frames > hf::kSmallMaxFrames)
    return fail(FDNN_E_ARG, "small-batch frames are 0 (off) .. " + std::to_string(hf::kSmallMaxFrames));
  std::lock_guard<std::mutex> lk(hm->mu);
  hm->small = max_frames;
  return FDNN_OK;
}

int fdnn_half_model_set_mid(fdnn_half_model *hm, int max_frames) {
  if (!hm || max_frames < 0 || max_frames > hf::kMidMaxFrames)
    return fail(FDNN_E_ARG, "mid-batch frames are 0 (off) .. " + std::to_string(hf::kMidMaxFrames));
  std::lock_guard<std::mutex> lk(hm->mu);
  hm->mid = max_frames;
  return FDNN_OK;
}

int fdnn_half_model_set_large(fdnn_half_model *hm, int min_frames) {
  if (!hm || min_frames < 0 || min_frames > hf::kLargeMaxSetting)
    return fail(FDNN_E_ARG, "large-batch frames are 0 (off) .. " + std::to_string(hf::kLargeMaxSetting));
  std::lock_guard<std::mutex> lk(hm->mu);
  hm->large = min_frames;
  return FDNN_OK;
}

int fdnn_half_calculate_device(fdnn_half_model *hm, const float *d_x, int n, float *d_out, void *stream) {
  if (!hm || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!d_x || !d_out) return fail(FDNN_E_ARG, "null buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(hm->mu);
  DeviceGuard g(hm->device);
  HIP_TRY(hm->order.enter(s));
  if (int rc = run_net(hm, d_x, n, d_out, s)) return rc;
  HIP_TRY(hm->order.leave(s));
  return FDNN_OK;
}

int fdnn_half_calculate(fdnn_half_model *hm, const float *x, int n, int dim, float *out) {
  if (!hm || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (dim != hm->hm.in_dim)
    return fail(FDNN_E_ARG, "input vector size " + std::to_string(dim) + " must be equal with network input size " + std::to_string(hm->hm.in_dim));
  if (n == 0) return FDNN_OK;
  if (!x || !out) return fail(FDNN_E_ARG, "null buffer");
  std::lock_guard<std::mutex> lk(hm->mu);
  DeviceGuard g(hm->device);
  const size_t D = size_t(dim), O = size_t(hm->hm.out_dim());
  HIP_TRY(hm->order.enter(nullptr));
  HIP_TRY(hm->d_x.reserve(size_t(n) * D));
  HIP_TRY(hm->d_out.reserve(size_t(n) * O));
  HIP_TRY(hipMemcpyAsync(hm->d_x, x, sizeof(float) * size_t(n) * D, hipMemcpyHostToDevice, nullptr));
  if (int rc = run_net(hm, hm->d_x, n, hm->d_out, nullptr)) return rc;
  HIP_TRY(hipMemcpyAsync(out, hm->d_out, sizeof(float) * size_t(n) * O, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hm->order.leave(nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  return FDNN_OK;
}

int fdnn_debug_half_layer(fdnn_half_model *hm, int j, const float *in, int n, float *lin, float *act) {
  if (!hm || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const int L = hm->n_layers();
  if (j < -1 || j >= L) return fail(FDNN_E_ARG, "layer index " + std::to_string(j) + " outside -1 .. " + std::to_string(L - 1));
  if (n == 0) return FDNN_OK;
  if (!in) return fail(FDNN_E_ARG, "null buffer");
  std::lock_guard<std::mutex> lk(hm->mu);
  DeviceGuard g(hm->device);
  HIP_TRY(hm->order.enter(nullptr));
  if (j < 0) {
    const int D = hm->hm.in_dim, ld = hm->shape.k0_pad;
    HIP_TRY(hm->d_x.reserve(size_t(n) * D));
    HIP_TRY(hm->d_lin.reserve(size_t(n) * D));
    HIP_TRY(hm->d_dbg.reserve(size_t(n) * ld));
    HIP_TRY(hipMemcpyAsync(hm->d_x, in, sizeof(float) * size_t(n) * D, hipMemcpyHostToDevice, nullptr));
    hf::launch_half_input_step(hm->d_x, hm->shift(), hm->scale(), hm->d_dbg, hm->d_lin, n, D, ld, nullptr);
    HIP_TRY(hipGetLastError());
    if (lin) HIP_TRY(hipMemcpyAsync(lin, hm->d_lin, sizeof(float) * size_t(n) * D, hipMemcpyDeviceToHost, nullptr));
    if (act)
      if (int rc = halves_to_host(hm->d_dbg, n, ld, D, act)) return rc;
  } else {
    const hf::LayerDesc &d = hm->hm.layers[size_t(j)];
    if (int rc = layer_upload(hm, j, in, n, lin != nullptr)) return rc;
    layer_launch(hm, j, n, lin != nullptr);
    HIP_TRY(hipGetLastError());
    if (lin) HIP_TRY(hipMemcpyAsync(lin, hm->d_lin, sizeof(float) * size_t(n) * d.rows, hipMemcpyDeviceToHost, nullptr));
    if (act && j + 1 == L) HIP_TRY(hipMemcpyAsync(act, hm->d_prob, sizeof(float) * size_t(n) * d.rows, hipMemcpyDeviceToHost, nullptr));
    else if (act)
      if (int rc = halves_to_host(hm->d_dbg, n, layer_ldo(hm, j), d.rows, act)) return rc;
  }
  HIP_TRY(hm->order.leave(nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  return FDNN_OK;
}

int fdnn_debug_half_layer_us(fdnn_half_model *hm, int j, const float *in, int n, int reps, double *us) {
  if (!hm || !in || !us || n < 1 || reps < 1) return fail(FDNN_E_ARG, "bad argument");
  const int L = hm->n_layers();
  if (j < 0 || j >= L) return fail(FDNN_E_ARG, "layer index " + std::to_string(j) + " outside 0 .. " + std::to_string(L - 1));
  std::lock_guard<std::mutex> lk(hm->mu);
  DeviceGuard g(hm->device);
  HIP_TRY(hm->order.enter(nullptr));
  if (int rc = layer_upload(hm, j, in, n, false)) return rc;
  struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
      if (a) hipEventDestroy(a);
      if (b) hipEventDestroy(b);
    }
  } ev;
  HIP_TRY(hipEventCreate(&ev.a));
  HIP_TRY(hipEventCreate(&ev.b));
  layer_launch(hm, j, n, false);  // warm-up
  HIP_TRY(hipEventRecord(ev.a, nullptr));
  for (int r = 0; r < reps; ++r) layer_launch(hm, j, n, false);
  HIP_TRY(hipEventRecord(ev.b, nullptr));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hm->order.leave(nullptr));
  HIP_TRY(hipEventSynchronize(ev.b));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
  *us = 1000.0 * double(ms) / reps;
  return FDNN_OK;
}

int fdnn_debug_half_launches(unsigned long long *out, int cap) {
  if (!out || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  unsigned long long v[hf::kLaunchKinds];
  hf::launch_counts(v);
  for (int i = 0; i < hf::kLaunchKinds && i < cap; ++i) out[i] = v[i];
  return hf::kLaunchKinds;
}

int fdnn_debug_half_small_launches(unsigned long long *out, int cap) {
  if (!out || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  unsigned long long v[hf::kSmallLaunchKinds];
  hf::small_launch_counts(v);
  for (int i = 0; i < hf::kSmallLaunchKinds && i < cap; ++i) out[i] = v[i];
  return hf::kSmallLaunchKinds;
}

int fdnn_debug_half_mid_launches(unsigned long long *out4) {
  if (!out4) return fail(FDNN_E_ARG, "bad argument");
  hf::mid_launch_counts(out4);
  return FDNN_OK;
}

int fdnn_debug_half_large_launches(unsigned long long *out4) {
  if (!out4) return fail(FDNN_E_ARG, "bad argument");
  hf::large_launch_counts(out4);
  return FDNN_OK;
}

// ---------------------------------------------------------------- lazy output for per-segment node sets (fdnn_half_set.hip)
int fdnn_half_calculate_lazy_sets(fdnn_half_model *hm, const float *x, int n, int dim, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs,
                                  const int32_t *nodes, float *probs, float *inactive) {
  if (!hm || n < 0 || n_segs < 0) return fail(FDNN_E_ARG, "bad argument");
  if (const int bad = sets::check(seg_rows, set_ptr, nodes, n_segs, hm->hm.out_dim(), n)) return sets_named(bad, hm->hm.out_dim(), n);
  return host_sets(hm, x, n, dim, sets::Tables{seg_rows, set_ptr, n_segs}, nodes, probs, inactive);
}

int fdnn_half_calculate_lazy_set(fdnn_half_model *hm, const float *x, int n, int dim, const int32_t *nodes, int len, float *probs, float *inactive) {
  if (!hm || n < 0 || len < 0) return fail(FDNN_E_ARG, "bad argument");
  const int32_t seg_rows[2] = {0, n}, set_ptr[2] = {0, len};
  return fdnn_half_calculate_lazy_sets(hm, x, n, dim, seg_rows, set_ptr, 1, nodes, probs, inactive);
}

int fdnn_half_calculate_lazy_sets_device(fdnn_half_model *hm, const float *d_x, int n, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs,
                                         const int32_t *d_nodes, float *d_probs, float *d_inactive, void *stream) {
  if (!hm || n < 0 || n_segs < 0) return fail(FDNN_E_ARG, "bad argument");
  if (const int bad = hset::check_tables(seg_rows, set_ptr, n_segs, hm->hm.out_dim(), n)) return sets_named(bad, hm->hm.out_dim(), n);
  const sets::Tables t{seg_rows, set_ptr, n_segs};
  if (int rc = sets_cover(t, n)) return rc;
  if (n == 0) return FDNN_OK;
  if (!d_x || !d_inactive || (sets::total(t) > 0 && (!d_probs || !d_nodes))) return fail(FDNN_E_ARG, "null buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(hm->mu);
  DeviceGuard g(hm->device);
  HIP_TRY(hm->order.enter(s));
  const SetCall sc{t, d_nodes, d_probs, d_inactive, nullptr};
  if (int rc = run_net(hm, d_x, n, nullptr, s, &sc)) return rc;
  HIP_TRY(hm->order.leave(s));
  return FDNN_OK;
}

int fdnn_debug_half_set_layer(fdnn_half_model *hm, const float *in, int n, const int32_t *nodes, int len, float *z, float *probs, float *inactive) {
  if (!hm || n < 0 || len < 0) return fail(FDNN_E_ARG, "bad argument");
  const int32_t seg_rows[2] = {0, n}, set_ptr[2] = {0, len};
  if (const int bad = sets::check(seg_rows, set_ptr, nodes, 1, hm->hm.out_dim(), n)) return sets_named(bad, hm->hm.out_dim(), n);
  const sets::Tables t{seg_rows, set_ptr, 1};
  if (int rc = sets_cover(t, n)) return rc;
  if (n == 0) return FDNN_OK;
  const size_t nnz = size_t(n) * size_t(len);
  if (!in || !inactive || (nnz > 0 && !probs)) return fail(FDNN_E_ARG, "null buffer");
  std::lock_guard<std::mutex> lk(hm->mu);
  DeviceGuard g(hm->device);
  HIP_TRY(hm->order.enter(nullptr));
  const int last = hm->n_layers() - 1, K_pad = hm->hm.layers[size_t(last)].K_pad;
  if (int rc = layer_upload(hm, last, in, n, false)) return rc;
  if (int rc = reserve_sets(hm, n, z != nullptr)) return rc;
  HIP_TRY(hm->d_snodes.reserve(std::max<size_t>(size_t(len), 1)));
  HIP_TRY(hm->d_sprobs.reserve(std::max<size_t>(nnz, 1)));
  HIP_TRY(hm->d_sinact.reserve(size_t(n)));
  if (z) HIP_TRY(hm->d_slin.reserve(std::max<size_t>(nnz, 1)));
  if (len) HIP_TRY(hipMemcpyAsync(hm->d_snodes, nodes, sizeof(int32_t) * size_t(len), hipMemcpyHostToDevice, nullptr));
  const SetCall sc{t, hm->d_snodes, hm->d_sprobs, hm->d_sinact, z ? hm->d_slin.p : nullptr};
  const int chunk = hf::chunk_rows(hm->chunk), cap = std::min(n, chunk);
  for (int i = 0; i < hf::n_chunks(n, chunk); ++i) {
    int first, m;
    hf::chunk_range(n, chunk, i, &first, &m);
    if (int rc = set_step(hm, hm->d_in + size_t(first) * K_pad, K_pad, first, m, n, cap, sc, nullptr)) return rc;
  }
  HIP_TRY(hipGetLastError());
  if (nnz) HIP_TRY(hipMemcpyAsync(probs, hm->d_sprobs, sizeof(float) * nnz, hipMemcpyDeviceToHost, nullptr));
  if (nnz && z) HIP_TRY(hipMemcpyAsync(z, hm->d_slin, sizeof(float) * nnz, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipMemcpyAsync(inactive, hm->d_sinact, sizeof(float) * size_t(n), hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hm->order.leave(nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  return FDNN_OK;
}

int fdnn_debug_half_set_layer_us(fdnn_half_model *hm, const float *in, int n, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs,
                                 const int32_t *nodes, int reps, double *us) {
  if (!hm || !in || !us || n < 1 || n_segs < 1 || reps < 1) return fail(FDNN_E_ARG, "bad argument");
  if (const int bad = sets::check(seg_rows, set_ptr, nodes, n_segs, hm->hm.out_dim(), n)) return sets_named(bad, hm->hm.out_dim(), n);
  const sets::Tables t{seg_rows, set_ptr, n_segs};
  if (int rc = sets_cover(t, n)) return rc;
  const size_t nnz = size_t(sets::total(t)), n_nodes = size_t(set_ptr[n_segs]);
  std::lock_guard<std::mutex> lk(hm->mu);
  DeviceGuard g(hm->device);
  HIP_TRY(hm->order.enter(nullptr));
  const int last = hm->n_layers() - 1, K_pad = hm->hm.layers[size_t(last)].K_pad;
  if (int rc = layer_upload(hm, last, in, n, false)) return rc;
  if (int rc = reserve_sets(hm, n, false)) return rc;
  HIP_TRY(hm->d_snodes.reserve(std::max<size_t>(n_nodes, 1)));
  HIP_TRY(hm->d_sprobs.reserve(std::max<size_t>(nnz, 1)));
  HIP_TRY(hm->d_sinact.reserve(size_t(n)));
  if (n_nodes) HIP_TRY(hipMemcpy(hm->d_snodes, nodes, sizeof(int32_t) * n_nodes, hipMemcpyHostToDevice));
  const SetCall sc{t, hm->d_snodes, hm->d_sprobs, hm->d_sinact, nullptr};
  const int chunk = hf::chunk_rows(hm->chunk), cap = std::min(n, chunk);
  auto run = [&]() -> int {
    for (int i = 0; i < hf::n_chunks(n, chunk); ++i) {
      int first, m;
      hf::chunk_range(n, chunk, i, &first, &m);
      if (int rc = set_step(hm, hm->d_in + size_t(first) * K_pad, K_pad, first, m, n, cap, sc, nullptr)) return rc;
    }
    return FDNN_OK;
  };
  struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
      if (a) hipEventDestroy(a);
      if (b) hipEventDestroy(b);
    }
  } ev;
  HIP_TRY(hipEventCreate(&ev.a));
  HIP_TRY(hipEventCreate(&ev.b));
  if (int rc = run()) return rc;  // warm-up
  HIP_TRY(hipEventRecord(ev.a, nullptr));
  for (int r = 0; r < reps; ++r)
    if (int rc = run()) return rc;
  HIP_TRY(hipEventRecord(ev.b, nullptr));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hm->order.leave(nullptr));
  HIP_TRY(hipEventSynchronize(ev.b));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
  *us = 1000.0 * double(ms) / reps;
  return FDNN_OK;
}

int fdnn_debug_half_set_launches(unsigned long long *out, int cap) {
  if (!out || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  unsigned long long v[hset::kLaunchKinds];
  hset::launch_counts(v);
  for (int i = 0; i < hset::kLaunchKinds && i < cap; ++i) out[i] = v[i];
  return hset::kLaunchKinds;
}

// ---------------------------------------------------------------- no device: what the host tests read
int fdnn_debug_half_set_plan(const int32_t *seg_rows, const int32_t *set_ptr, int n_segs, int K_pad, int rows_pad, int n_cu, int *out4) {
  if (!out4 || n_segs < 0 || K_pad < 1 || rows_pad < 1) return fail(FDNN_E_ARG, "bad argument");
  const int rows = n_segs > 0 && seg_rows ? seg_rows[n_segs] : 0;
  if (const int bad = hset::check_tables(seg_rows, set_ptr, n_segs, rows_pad, rows)) return sets_named(bad, rows_pad, rows);
  const sets::Tables t{seg_rows, set_ptr, n_segs};
  const std::vector<sets::Launch> launches = hset::plan(sets::slice(t, n_segs ? seg_rows[0] : 0, rows), n_cu);
  out4[0] = hset::applies(K_pad, rows_pad, K_pad, std::max(rows, 1)) ? 1 : 0;
  out4[1] = int(launches.size());
  out4[2] = 0;
  for (const sets::Launch &l : launches) out4[2] += sets::blocks(l);
  out4[3] = launches.empty() ? 0 : launches[0].tiles_per_group;
  return FDNN_OK;
}

int fdnn_debug_half_small_plan(int n, int setting, int rows_pad, int act, int *out3) {
  if (!out3 || rows_pad < 1 || rows_pad % hf::kPartialNodes || (act != hf::kSigmoid && act != hf::kExp)) return fail(FDNN_E_ARG, "bad argument");
  const bool applies = hf::small_applies(n, setting);
  out3[0] = applies ? 1 : 0;
  out3[1] = applies ? int(hf::small_grid(rows_pad, hf::Act(act))) : 0;
  out3[2] = applies ? hf::small_frame_tiles(n) : 0;
  return FDNN_OK;
}

int fdnn_debug_half_mid_plan(int n, int small_setting, int mid_setting, int rows_pad, int act, int *out3) {
  if (!out3 || rows_pad < 1 || rows_pad % hf::kMidNodeTile || (act != hf::kSigmoid && act != hf::kExp)) return fail(FDNN_E_ARG, "bad argument");
  const bool applies = hf::mid_applies(n, small_setting, mid_setting);
  unsigned gx = 0, gy = 0;
  if (applies) hf::mid_grid(n, rows_pad, &gx, &gy);
  out3[0] = applies ? 1 : 0;
  out3[1] = int(gx);
  out3[2] = int(gy);
  return FDNN_OK;
}

int fdnn_debug_half_large_plan(int n, int small_setting, int mid_setting, int large_setting, int rows_pad, int act, int *out3) {
  if (!out3 || rows_pad < 1 || rows_pad % hf::kNodeTile || (act != hf::kSigmoid && act != hf::kExp)) return fail(FDNN_E_ARG, "bad argument");
  const bool applies = hf::large_applies(n, small_setting, mid_setting, large_setting);
  unsigned gx = 0, gy = 0;
  if (applies) hf::gemm_grid(n, rows_pad, &gx, &gy);
  out3[0] = applies ? 1 : 0;
  out3[1] = int(gx);
  out3[2] = int(gy);
  return FDNN_OK;
}

int fdnn_debug_half_pack(const char *path, void *blob, size_t cap, long long *desc, int desc_cap) {
  if (!path) return fail(FDNN_E_ARG, "null argument");
  hf::HalfHostModel hm;
  std::string msg;
  if (int rc = fdnn::load_half_host_model(path, &hm, &msg)) return fail(rc, msg);
  std::vector<long long> d;
  for (const hf::LayerDesc &l : hm.layers)
    for (long long v : {(long long)l.off_w, (long long)l.off_bias, (long long)l.rows, (long long)l.rows_pad, (long long)l.K, (long long)l.K_pad}) d.push_back(v);
  d.push_back((long long)hm.off_shift);
  d.push_back((long long)hm.off_scale);
  d.push_back((long long)hm.blob.size());
  if (blob && cap >= hm.blob.size()) std::memcpy(blob, hm.blob.data(), hm.blob.size());
  for (int i = 0; desc && i < desc_cap && i < int(d.size()); ++i) desc[i] = d[size_t(i)];
  return int(d.size());
}

int fdnn_debug_half_extents(const int *shape4, int n, int chunk_setting, long long *out7) {
  if (!shape4 || !out7 || n < 1) return fail(FDNN_E_ARG, "bad argument");
  const hf::Shape s{shape4[0], shape4[1], shape4[2], shape4[3]};
  const int chunk = hf::chunk_rows(chunk_setting);
  const hf::Counts c = hf::counts(s, n, chunk);
  long long xs = 0, act = 0, partial = 0, covered = 0, grid_ok = 1;
  for (int i = 0; i < hf::n_chunks(n, chunk); ++i) {
    int first, m;
    hf::chunk_range(n, chunk, i, &first, &m);
    if (first != covered || m < 1 || m > c.cap) grid_ok = 0;
    covered += m;
    unsigned gx, gy;
    hf::gemm_grid(m, s.out_rows_pad, &gx, &gy);
    if (size_t(gx) * hf::kFrameTile < size_t(m) || size_t(gx - 1) * hf::kFrameTile >= size_t(m) || int(gy) * hf::kNodeTile != s.out_rows_pad) grid_ok = 0;
    xs = std::max(xs, (long long)hf::rows_extent(m, s.k0_pad, s.k0_pad));
    act = std::max(act, (long long)hf::rows_extent(m, s.act_ld, s.act_ld));
    partial = std::max(partial, (long long)hf::partial_extent(m, c.cap, s.out_rows_pad / hf::kPartialNodes));
  }
  const long long v[7] = {(long long)c.xs, (long long)c.act, (long long)c.partial, xs, act, partial, covered == n ? grid_ok : 0};
  std::memcpy(out7, v, sizeof(v));
  return FDNN_OK;
}

}  // extern "C"
