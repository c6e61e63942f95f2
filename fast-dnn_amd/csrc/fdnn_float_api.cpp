// fdnn_float_api.cpp -- C-ABI of the unquantized net and of the quantization report (include/fdnn.h, last section):
// the model and report objects, the chunk loop over fdnn_float.hip's launches, the host restatements.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>

#include "fdnn_float.hpp"
#include "fdnn_internal.hpp"

using fdnn::DevBuf;
using fdnn::DeviceGuard;
using fdnn::fail;
namespace fl = fdnn::fl;

namespace {

// One set of buffers serves every call of an object: a call on another stream waits (on the device) for the one before.
struct StreamOrder {
  hipEvent_t ev = nullptr;
  hipStream_t last = nullptr;
  bool valid = false;
  ~StreamOrder() {
    if (ev) hipEventDestroy(ev);
  }
  hipError_t enter(hipStream_t s) {
    if (!ev) {
      hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
    return valid && last != s ? hipStreamWaitEvent(s, ev, 0) : hipSuccess;
  }
  hipError_t leave(hipStream_t s) {
    last = s;
    valid = true;
    return hipEventRecord(ev, s);
  }
};

int device_ok(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(FDNN_E_DEVICE, "no HIP device available: this library has no CPU path");
  if (device < 0 || device >= count) return fail(FDNN_E_ARG, "device index out of range");
  return FDNN_OK;
}

}  // namespace

struct fdnn_float_model {
  fl::FloatHostModel hm;
  fl::Shape shape;
  int device = 0;
  int chunk = 0;  // fdnn_debug_float_set_chunk (0 = default)
  std::mutex mu;
  StreamOrder order;
  DevBuf<uint8_t> d_blob;
  DevBuf<float> d_xs, d_act[2], d_partial;  // fl::counts
  DevBuf<float> d_x, d_out;                 // the host entry points' copies: [n][in_dim], [n][O]
  DevBuf<float> d_in, d_lin, d_dbg;         // fdnn_debug_float_layer: [n][K_pad], [n][rows], [n][ldo]
  const float *w(int j) const { return reinterpret_cast<const float *>(d_blob.p + hm.layers[size_t(j)].off_w); }
  const float *bias(int j) const { return reinterpret_cast<const float *>(d_blob.p + hm.layers[size_t(j)].off_bias); }
  const float *shift() const { return reinterpret_cast<const float *>(d_blob.p + hm.off_shift); }
  const float *scale() const { return reinterpret_cast<const float *>(d_blob.p + hm.off_scale); }
};

struct fdnn_report {
  int device = 0, O = 0;
  std::mutex mu;
  StreamOrder order;
  DevBuf<unsigned long long> d_cnt;           // [3]
  DevBuf<double> d_node_sum, d_node_max;      // [O]
  DevBuf<double> d_blk_sum, d_blk_max;        // [ceil(rows / kReportRows)][O], rows <= kReportCallRows
  DevBuf<unsigned char> d_row_nan;            // [rows]
  DevBuf<float> d_ref, d_q;                   // fdnn_report_add's copies
};

namespace {

int reserve_call(fdnn_float_model *fm, int n) {
  const fl::Counts c = fl::counts(fm->shape, n, fl::chunk_rows(fm->chunk));
  HIP_TRY(fm->d_xs.reserve(c.xs));
  HIP_TRY(fm->d_act[0].reserve(c.act));
  HIP_TRY(fm->d_act[1].reserve(c.act));
  HIP_TRY(fm->d_partial.reserve(c.partial));
  return FDNN_OK;
}

// One layer over m frames of one chunk.  in rows lda apart; the last layer writes e and the partials, then the scale pass.
void run_layer(fdnn_float_model *fm, int j, const float *in, int lda, int m, int cap, float *out, int ldo, float *tap, hipStream_t s) {
  const fl::LayerDesc &d = fm->hm.layers[size_t(j)];
  const bool last = j + 1 == int(fm->hm.layers.size());
  fl::GemmParams p{};
  p.a = in;
  p.w = fm->w(j);
  p.bias = fm->bias(j);
  p.out = out;
  p.tap = tap;
  p.partial = last ? fm->d_partial.p : nullptr;
  p.n = m;
  p.rows = d.rows;
  p.rows_pad = d.rows_pad;
  p.K_pad = d.K_pad;
  p.lda = lda;
  p.ldo = last ? d.rows : ldo;
  p.partial_ld = cap;
  fl::launch_fgemm(p, last ? fl::kExp : fl::kSigmoid, s);
  if (last) fdnn::launch_normalize(out, out, fm->d_partial, m, cap, d.rows, d.rows_pad / fl::kPartialNodes, s);
}

// The whole net on device rows d_x [n][in_dim] -> d_out [n][O], chunk by chunk.
int run_net(fdnn_float_model *fm, const float *d_x, int n, float *d_out, hipStream_t s) {
  if (int rc = reserve_call(fm, n)) return rc;
  const int chunk = fl::chunk_rows(fm->chunk), cap = std::min(n, chunk), L = int(fm->hm.layers.size());
  const int D = fm->hm.in_dim, O = fm->hm.out_dim();
  for (int i = 0; i < fl::n_chunks(n, chunk); ++i) {
    int first, m;
    fl::chunk_range(n, chunk, i, &first, &m);
    fl::launch_input_step(d_x + size_t(first) * D, fm->shift(), fm->scale(), fm->d_xs, nullptr, m, D, fm->shape.k0_pad, s);
    const float *in = fm->d_xs;
    int lda = fm->shape.k0_pad;
    for (int j = 0; j < L; ++j) {
      const bool last = j + 1 == L;
      float *out = last ? d_out + size_t(first) * O : fm->d_act[j & 1].p;
      const int ldo = last ? O : fm->hm.layers[size_t(j) + 1].K_pad;
      run_layer(fm, j, in, lda, m, cap, out, ldo, nullptr, s);
      in = out;
      lda = ldo;
    }
  }
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

// fdnn_debug_float_layer and its timing twin: layer j's output row length, the caller's rows [n][K] into d_in [n][K_pad]
// (pad columns +0, as every activation buffer has them), and the layer over them chunk by chunk into d_dbg (z into d_lin).
int layer_ldo(const fdnn_float_model *fm, int j) {
  const fl::LayerDesc &d = fm->hm.layers[size_t(j)];
  return j + 1 == int(fm->hm.layers.size()) ? d.rows : int(fl::align_up(size_t(d.rows), fl::kKStep));
}

int layer_upload(fdnn_float_model *fm, int j, const float *in, int n, bool tap) {
  const fl::LayerDesc &d = fm->hm.layers[size_t(j)];
  if (int rc = reserve_call(fm, n)) return rc;
  std::vector<float> padded(size_t(n) * size_t(d.K_pad), 0.0f);
  for (int f = 0; f < n; ++f) std::memcpy(&padded[size_t(f) * d.K_pad], in + size_t(f) * d.K, sizeof(float) * size_t(d.K));
  HIP_TRY(fm->d_in.reserve(padded.size()));
  if (tap) HIP_TRY(fm->d_lin.reserve(size_t(n) * d.rows));
  HIP_TRY(fm->d_dbg.reserve(size_t(n) * layer_ldo(fm, j)));
  HIP_TRY(hipMemcpy(fm->d_in, padded.data(), sizeof(float) * padded.size(), hipMemcpyHostToDevice));
  return FDNN_OK;
}

void layer_launch(fdnn_float_model *fm, int j, int n, bool tap) {
  const fl::LayerDesc &d = fm->hm.layers[size_t(j)];
  const int chunk = fl::chunk_rows(fm->chunk), cap = std::min(n, chunk), ldo = layer_ldo(fm, j);
  for (int i = 0; i < fl::n_chunks(n, chunk); ++i) {
    int first, m;
    fl::chunk_range(n, chunk, i, &first, &m);
    run_layer(fm, j, fm->d_in + size_t(first) * d.K_pad, d.K_pad, m, cap, fm->d_dbg + size_t(first) * ldo, ldo,
              tap ? fm->d_lin + size_t(first) * d.rows : nullptr, nullptr);
  }
}

}  // namespace

extern "C" {

int fdnn_float_model_load_on(const char *path, int device, fdnn_float_model **out) {
  if (!path || !out) return fail(FDNN_E_ARG, "null argument");
  *out = nullptr;
  std::unique_ptr<fdnn_float_model> fm(new fdnn_float_model());
  std::string msg;
  if (int rc = fdnn::load_float_host_model(path, &fm->hm, &msg)) return fail(rc, msg);
  if (int rc = device_ok(device)) return rc;
  fm->device = device;
  fm->shape = fl::shape_of(fm->hm);
  DeviceGuard g(device);
  if (!g.ok) return fail(FDNN_E_DEVICE, "hipSetDevice failed");
  HIP_TRY(fm->d_blob.reserve(fm->hm.blob.size()));
  HIP_TRY(hipMemcpy(fm->d_blob, fm->hm.blob.data(), fm->hm.blob.size(), hipMemcpyHostToDevice));
  *out = fm.release();
  return FDNN_OK;
}

int fdnn_float_model_load(const char *path, fdnn_float_model **out) { return fdnn_float_model_load_on(path, 0, out); }

void fdnn_float_model_free(fdnn_float_model *fm) {
  if (!fm) return;
  DeviceGuard g(fm->device);
  hipDeviceSynchronize();
  delete fm;
}

int fdnn_float_model_input_dim(const fdnn_float_model *fm) { return fm ? fm->hm.in_dim : -1; }
int fdnn_float_model_output_dim(const fdnn_float_model *fm) { return fm ? fm->hm.out_dim() : -1; }
int fdnn_float_model_layer_count(const fdnn_float_model *fm) { return fm ? int(fm->hm.layers.size()) : -1; }
int fdnn_float_model_layer_dim(const fdnn_float_model *fm, int index) {
  return fm && index >= 0 && index < int(fm->hm.layers.size()) ? fm->hm.layers[size_t(index)].rows : -1;
}
int fdnn_float_model_device(const fdnn_float_model *fm) { return fm ? fm->device : -1; }

int fdnn_debug_float_set_chunk(fdnn_float_model *fm, int rows) {
  if (!fm || rows < 0 || rows > fl::kMaxChunk) return fail(FDNN_E_ARG, "chunk rows are 0 (default) .. " + std::to_string(fl::kMaxChunk));
  std::lock_guard<std::mutex> lk(fm->mu);
  fm->chunk = rows;
  return FDNN_OK;
}

int fdnn_float_calculate_device(fdnn_float_model *fm, const float *d_x, int n, float *d_out, void *stream) {
  if (!fm || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!d_x || !d_out) return fail(FDNN_E_ARG, "null buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(fm->mu);
  DeviceGuard g(fm->device);
  HIP_TRY(fm->order.enter(s));
  if (int rc = run_net(fm, d_x, n, d_out, s)) return rc;
  HIP_TRY(fm->order.leave(s));
  return FDNN_OK;
}

int fdnn_float_calculate(fdnn_float_model *fm, const float *x, int n, int dim, float *out) {
  if (!fm || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (dim != fm->hm.in_dim)
    return fail(FDNN_E_ARG, "input vector size " + std::to_string(dim) + " must be equal with network input size " + std::to_string(fm->hm.in_dim));
  if (n == 0) return FDNN_OK;
  if (!x || !out) return fail(FDNN_E_ARG, "null buffer");
  std::lock_guard<std::mutex> lk(fm->mu);
  DeviceGuard g(fm->device);
  const size_t D = size_t(dim), O = size_t(fm->hm.out_dim());
  HIP_TRY(fm->order.enter(nullptr));
  HIP_TRY(fm->d_x.reserve(size_t(n) * D));
  HIP_TRY(fm->d_out.reserve(size_t(n) * O));
  HIP_TRY(hipMemcpyAsync(fm->d_x, x, sizeof(float) * size_t(n) * D, hipMemcpyHostToDevice, nullptr));
  if (int rc = run_net(fm, fm->d_x, n, fm->d_out, nullptr)) return rc;
  HIP_TRY(hipMemcpyAsync(out, fm->d_out, sizeof(float) * size_t(n) * O, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(fm->order.leave(nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  return FDNN_OK;
}

int fdnn_debug_float_layer(fdnn_float_model *fm, int j, const float *in, int n, float *lin, float *act) {
  if (!fm || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const int L = int(fm->hm.layers.size());
  if (j < -1 || j >= L) return fail(FDNN_E_ARG, "layer index " + std::to_string(j) + " outside -1 .. " + std::to_string(L - 1));
  if (n == 0) return FDNN_OK;
  if (!in) return fail(FDNN_E_ARG, "null buffer");
  std::lock_guard<std::mutex> lk(fm->mu);
  DeviceGuard g(fm->device);
  HIP_TRY(fm->order.enter(nullptr));
  if (j < 0) {
    const int D = fm->hm.in_dim, ld = fm->shape.k0_pad;
    HIP_TRY(fm->d_in.reserve(size_t(n) * D));
    HIP_TRY(fm->d_lin.reserve(size_t(n) * D));
    HIP_TRY(fm->d_dbg.reserve(size_t(n) * ld));
    HIP_TRY(hipMemcpyAsync(fm->d_in, in, sizeof(float) * size_t(n) * D, hipMemcpyHostToDevice, nullptr));
    fl::launch_input_step(fm->d_in, fm->shift(), fm->scale(), fm->d_dbg, fm->d_lin, n, D, ld, nullptr);
    if (lin) HIP_TRY(hipMemcpyAsync(lin, fm->d_lin, sizeof(float) * size_t(n) * D, hipMemcpyDeviceToHost, nullptr));
    if (act)
      HIP_TRY(hipMemcpy2DAsync(act, sizeof(float) * D, fm->d_dbg, sizeof(float) * ld, sizeof(float) * D, size_t(n), hipMemcpyDeviceToHost, nullptr));
  } else {
    const fl::LayerDesc &d = fm->hm.layers[size_t(j)];
    const int ldo = layer_ldo(fm, j);
    if (int rc = layer_upload(fm, j, in, n, lin != nullptr)) return rc;
    layer_launch(fm, j, n, lin != nullptr);
    if (lin) HIP_TRY(hipMemcpyAsync(lin, fm->d_lin, sizeof(float) * size_t(n) * d.rows, hipMemcpyDeviceToHost, nullptr));
    if (act)
      HIP_TRY(hipMemcpy2DAsync(act, sizeof(float) * d.rows, fm->d_dbg, sizeof(float) * ldo, sizeof(float) * d.rows, size_t(n), hipMemcpyDeviceToHost,
                               nullptr));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(fm->order.leave(nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  return FDNN_OK;
}

int fdnn_debug_float_layer_us(fdnn_float_model *fm, int j, const float *in, int n, int reps, double *us) {
  if (!fm || !in || !us || n < 1 || reps < 1) return fail(FDNN_E_ARG, "bad argument");
  const int L = int(fm->hm.layers.size());
  if (j < 0 || j >= L) return fail(FDNN_E_ARG, "layer index " + std::to_string(j) + " outside 0 .. " + std::to_string(L - 1));
  std::lock_guard<std::mutex> lk(fm->mu);
  DeviceGuard g(fm->device);
  HIP_TRY(fm->order.enter(nullptr));
  if (int rc = layer_upload(fm, j, in, n, false)) return rc;
  struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
      if (a) hipEventDestroy(a);
      if (b) hipEventDestroy(b);
    }
  } ev;
  HIP_TRY(hipEventCreate(&ev.a));
  HIP_TRY(hipEventCreate(&ev.b));
  layer_launch(fm, j, n, false);  // warm-up
  HIP_TRY(hipEventRecord(ev.a, nullptr));
  for (int r = 0; r < reps; ++r) layer_launch(fm, j, n, false);
  HIP_TRY(hipEventRecord(ev.b, nullptr));
  HIP_TRY(hipGetLastError());
  HIP_TRY(fm->order.leave(nullptr));
  HIP_TRY(hipEventSynchronize(ev.b));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
  *us = 1000.0 * double(ms) / reps;
  return FDNN_OK;
}

int fdnn_debug_float_layer_ref(const float *w, const float *bias, int rows, int K, const float *in, int n, float *lin) {
  if (!w || !bias || !in || !lin || rows < 0 || K < 0 || n < 0) return fail(FDNN_E_ARG, "bad argument");
  fl::float_layer_ref(w, K, bias, rows, K, in, K, n, lin);
  return FDNN_OK;
}

int fdnn_debug_float_input_ref(const float *shift, const float *scale, int dim, const float *x, int n, float *lin, float *act) {
  if (!shift || !scale || !x || dim < 0 || n < 0) return fail(FDNN_E_ARG, "bad argument");
  fl::float_input_ref(shift, scale, dim, x, n, lin, act);
  return FDNN_OK;
}

int fdnn_debug_float_launches(unsigned long long *out, int cap) {
  if (!out || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  unsigned long long v[fl::kLaunchKinds];
  fl::launch_counts(v);
  for (int i = 0; i < fl::kLaunchKinds && i < cap; ++i) out[i] = v[i];
  return fl::kLaunchKinds;
}

// ---------------------------------------------------------------- report
int fdnn_report_create(int device, int output_dim, fdnn_report **out) {
  if (!out) return fail(FDNN_E_ARG, "null argument");
  *out = nullptr;
  if (output_dim < 1 || output_dim > (1 << 19)) return fail(FDNN_E_ARG, "output_dim is 1 .. 524288");
  if (int rc = device_ok(device)) return rc;
  std::unique_ptr<fdnn_report> r(new fdnn_report());
  r->device = device;
  r->O = output_dim;
  DeviceGuard g(device);
  if (!g.ok) return fail(FDNN_E_DEVICE, "hipSetDevice failed");
  HIP_TRY(r->d_cnt.reserve(3));
  HIP_TRY(r->d_node_sum.reserve(size_t(output_dim)));
  HIP_TRY(r->d_node_max.reserve(size_t(output_dim)));
  HIP_TRY(r->d_cnt.fill(0));
  HIP_TRY(r->d_node_sum.fill(0));
  HIP_TRY(r->d_node_max.fill(0));
  HIP_TRY(hipStreamSynchronize(nullptr));
  *out = r.release();
  return FDNN_OK;
}

void fdnn_report_free(fdnn_report *r) {
  if (!r) return;
  DeviceGuard g(r->device);
  hipDeviceSynchronize();
  delete r;
}

int fdnn_report_reset(fdnn_report *r) {
  if (!r) return fail(FDNN_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard g(r->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(r->d_cnt.fill(0));
  HIP_TRY(r->d_node_sum.fill(0));
  HIP_TRY(r->d_node_max.fill(0));
  HIP_TRY(hipStreamSynchronize(nullptr));
  r->order.valid = false;
  return FDNN_OK;
}

static int report_enqueue(fdnn_report *r, const float *d_ref, const float *d_q, int n, hipStream_t s) {
  const int rows = std::min(n, fl::kReportCallRows), blocks = (rows + fl::kReportRows - 1) / fl::kReportRows;
  HIP_TRY(r->d_row_nan.reserve(size_t(rows)));
  HIP_TRY(r->d_blk_sum.reserve(size_t(blocks) * r->O));
  HIP_TRY(r->d_blk_max.reserve(size_t(blocks) * r->O));
  for (int first = 0; first < n; first += fl::kReportCallRows) {
    fl::ReportParams p{};
    p.ref = d_ref + size_t(first) * r->O;
    p.q = d_q + size_t(first) * r->O;
    p.n = std::min(fl::kReportCallRows, n - first);
    p.O = r->O;
    p.row_nan = r->d_row_nan;
    p.blk_sum = r->d_blk_sum;
    p.blk_max = r->d_blk_max;
    p.cnt = r->d_cnt;
    p.node_sum = r->d_node_sum;
    p.node_max = r->d_node_max;
    fl::launch_report(p, s);
  }
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

int fdnn_report_add_device(fdnn_report *r, const float *d_ref, const float *d_q, int n, void *stream) {
  if (!r || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!d_ref || !d_q) return fail(FDNN_E_ARG, "null buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard g(r->device);
  HIP_TRY(r->order.enter(s));
  if (int rc = report_enqueue(r, d_ref, d_q, n, s)) return rc;
  HIP_TRY(r->order.leave(s));
  return FDNN_OK;
}

int fdnn_report_add(fdnn_report *r, const float *ref, const float *q, int n) {
  if (!r || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!ref || !q) return fail(FDNN_E_ARG, "null buffer");
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard g(r->device);
  const size_t count = size_t(n) * size_t(r->O);
  HIP_TRY(r->order.enter(nullptr));
  HIP_TRY(r->d_ref.reserve(count));
  HIP_TRY(r->d_q.reserve(count));
  HIP_TRY(hipMemcpyAsync(r->d_ref, ref, sizeof(float) * count, hipMemcpyHostToDevice, nullptr));
  HIP_TRY(hipMemcpyAsync(r->d_q, q, sizeof(float) * count, hipMemcpyHostToDevice, nullptr));
  if (int rc = report_enqueue(r, r->d_ref, r->d_q, n, nullptr)) return rc;
  HIP_TRY(r->order.leave(nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  return FDNN_OK;
}

int fdnn_report_read(fdnn_report *r, double threshold, fdnn_accuracy *acc, double *node_sum) {
  if (!r || !acc) return fail(FDNN_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(r->mu);
  DeviceGuard g(r->device);
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long cnt[3];
  std::vector<double> sum(size_t(r->O)), mx(size_t(r->O));
  HIP_TRY(hipMemcpy(cnt, r->d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sum.data(), r->d_node_sum, sizeof(double) * sum.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(mx.data(), r->d_node_max, sizeof(double) * mx.size(), hipMemcpyDeviceToHost));
  fdnn_accuracy a{};
  a.frames = cnt[0];
  a.nan_rows = cnt[1];
  a.top1_agree = cnt[2];
  for (int i = 0; i < r->O; ++i) {  // nodes ascending: a fixed order here too
    a.sum_abs += sum[size_t(i)];
    a.max_abs = std::max(a.max_abs, mx[size_t(i)]);
    a.max_node_sum = std::max(a.max_node_sum, sum[size_t(i)]);
    if (sum[size_t(i)] > threshold) ++a.nodes_over;
  }
  *acc = a;
  if (node_sum) std::memcpy(node_sum, sum.data(), sizeof(double) * sum.size());
  return FDNN_OK;
}

}  // extern "C"
