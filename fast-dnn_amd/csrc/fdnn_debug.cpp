// fdnn_debug.cpp -- what tests, tools and measurements reach through the C-ABI (include/fdnn.h) besides scoring: the
// fdnn_debug_* switches and taps, the launch recorder's name table, per-kernel timing, the give-up / fault counters and
// the host-only model accessors (fdnn_host_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "fdnn_internal.hpp"
#include "fdnn_server_plan.hpp"

using namespace fdnn;

struct fdnn_host_model {
  fdnn::HostModel hm;
};

// ---- the launch recorder (fdnn_note.hpp)
namespace fdnn {
const LaunchNameInfo kLaunchNames[kLaunchNameCount] = {
#define FDNN_X(id, name, flags) {name, flags},
    FDNN_LAUNCH_NAMES(FDNN_X)
#undef FDNN_X
#define FDNN_G(out, shape, branch, name, abl) {name, abl},
        FDNN_GEMM_LAUNCH_NAMES(FDNN_G)
#undef FDNN_G
};
std::atomic<int> g_launch_note_on{0};
std::atomic<unsigned long long> g_launch_count[kLaunchNameCount];
int gemm_launch_name(bool output, int shape, int branch) {
  static const struct {
    int out, shape, branch, id;
  } known[] = {
#define FDNN_G(out, shape, branch, name, abl) {out, gs_##shape, gb_##branch, kLn_gemm_##out##_##shape##_##branch},
      FDNN_GEMM_LAUNCH_NAMES(FDNN_G)
#undef FDNN_G
  };
  for (const auto &k : known)
    if (k.out == (output ? 1 : 0) && k.shape == shape && k.branch == branch) return k.id;
  return kLn_unlisted;
}
}  // namespace fdnn

// ---- the scratch audit (the table is kCtxScratch, fdnn_ctx_layout.hpp)
namespace fdnn {
namespace {
std::atomic<int> g_scratch_audit_on{0};
std::atomic<unsigned long long> g_scratch_dirty[kCtxScratchCount];
std::atomic<unsigned long long> g_scratch_ctxs{0}, g_scratch_errors{0}, g_scratch_ns{0};  // (ns: what the audit itself cost, wait included)
}  // namespace

int ctx_scratch_dirty(fdnn_ctx *c, unsigned long long *out) {
  DeviceGuard g(c->m->device);
  ctx_wait_host(c);
  const bool chain_faulted = c->h_chain_fault && __atomic_load_n(c->h_chain_fault.p, __ATOMIC_RELAXED) != 0;
  // a role-split fused launch of this model left a half unwritten (fdnn_ppo.hip: the word's upper half counts them): the node
  // tiles that gave up never gathered, so the half's two counters were not rewound -- run_output zeroes the array in stream
  // order before every fused launch from then on
  const bool ppo_gave_up = c->m->h_fuse_fault && (__atomic_load_n(c->m->h_fuse_fault.p, __ATOMIC_RELAXED) >> 32) != 0;
  std::vector<uint32_t> host;
  for (int i = 0; i < kCtxScratchCount; ++i) {
    out[i] = 0;
    const ScratchBuf b = ctx_scratch_buf(c, i);
    if (!b.p || !b.words || (chain_faulted && (i == kChainCtl || i == kChainDone)) || (ppo_gave_up && i == kFuseCnt)) continue;
    host.resize(b.words);
    HIP_TRY(hipMemcpy(host.data(), b.p, sizeof(uint32_t) * b.words, hipMemcpyDeviceToHost));
    out[i] = static_cast<unsigned long long>(std::count_if(host.begin(), host.end(), [](uint32_t w) { return w != 0; }));
  }
  return FDNN_OK;
}

void scratch_audit_event(fdnn_ctx *c) {
  if (!g_scratch_audit_on.load(std::memory_order_relaxed) || !c || !c->m) return;
  unsigned long long dirty[kCtxScratchCount];
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = ctx_scratch_dirty(c, dirty);
  g_scratch_ns.fetch_add(static_cast<unsigned long long>(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count()),
                         std::memory_order_relaxed);
  if (rc != FDNN_OK) {  // (a context that cannot be read is not a clean one)
    g_scratch_errors.fetch_add(1, std::memory_order_relaxed);
    return;
  }
  for (int i = 0; i < kCtxScratchCount; ++i) g_scratch_dirty[i].fetch_add(dirty[i], std::memory_order_relaxed);
  g_scratch_ctxs.fetch_add(1, std::memory_order_relaxed);
}
}  // namespace fdnn

extern "C" {

int fdnn_debug_scratch_count(void) { return kCtxScratchCount; }

const char *fdnn_debug_scratch_name(int index) { return index >= 0 && index < kCtxScratchCount ? kCtxScratch[index].name : nullptr; }

int fdnn_debug_ctx_scratch(fdnn_ctx *c, unsigned long long *out, int n) {
  if (!c || !out || n < kCtxScratchCount) return fail(FDNN_E_ARG, "bad argument");
  return ctx_scratch_dirty(c, out);
}

int fdnn_debug_ctx_scratch_words(fdnn_ctx *c, unsigned long long *out, int n) {
  if (!c || !out || n < kCtxScratchCount) return fail(FDNN_E_ARG, "bad argument");
  for (int i = 0; i < kCtxScratchCount; ++i) out[i] = ctx_scratch_buf(c, i).words;
  return FDNN_OK;
}

int fdnn_debug_ctx_scratch_poke(fdnn_ctx *c, int which, long long index, unsigned value) {
  if (!c || which < 0 || which >= kCtxScratchCount) return fail(FDNN_E_ARG, "bad argument");
  const ScratchBuf b = ctx_scratch_buf(c, which);
  if (!b.p || index < 0 || static_cast<unsigned long long>(index) >= b.words) return fail(FDNN_E_ARG, "word index outside the buffer");
  DeviceGuard g(c->m->device);
  ctx_wait_host(c);
  const uint32_t v = value;
  HIP_TRY(hipMemcpy(b.p + index, &v, sizeof(v), hipMemcpyHostToDevice));
  return FDNN_OK;
}

int fdnn_debug_scratch_audit(int on) {
  g_scratch_audit_on.store(on ? 1 : 0, std::memory_order_relaxed);
  return FDNN_OK;
}

int fdnn_debug_scratch_dirty(unsigned long long *out, int n) {
  if (!out || n < kCtxScratchCount + 3) return fail(FDNN_E_ARG, "bad argument");
  for (int i = 0; i < kCtxScratchCount; ++i) out[i] = g_scratch_dirty[i].exchange(0, std::memory_order_relaxed);
  out[kCtxScratchCount] = g_scratch_ctxs.exchange(0, std::memory_order_relaxed);
  out[kCtxScratchCount + 1] = g_scratch_errors.exchange(0, std::memory_order_relaxed);
  out[kCtxScratchCount + 2] = g_scratch_ns.exchange(0, std::memory_order_relaxed);
  return FDNN_OK;
}

int fdnn_debug_set_l0_kernel(fdnn_model *m, int kind) {
  if (!m) return fail(FDNN_E_ARG, "null model");
  if (kind < 0 || kind > 4) return fail(FDNN_E_ARG, "layer-0 kernel kind must be 0 .. 4");
  m->l0_kernel = kind;
  return FDNN_OK;
}

int fdnn_debug_set_fuse(int mode) {
  if (mode < -1 || mode > 1) return fail(FDNN_E_ARG, "fuse mode must be -1, 0 or 1");
  fdnn::sel::tuning().fuse_mode = mode;
  return FDNN_OK;
}

int fdnn_debug_lazy_expand(float *out, const float *comp, int count, int O, int stride, const uint64_t *bits, int mode) {
  if (!out || !comp || !bits || count < 0 || O <= 0 || stride <= 0 || stride > O + 1 || mode < 0 || mode > 2) return fail(FDNN_E_ARG, "bad argument");
  lazy_expand_force_scalar(mode == 1);
  if (mode == 2) {
    if (stride > O) return fail(FDNN_E_ARG, "the in-place form needs stride <= O");
    std::memmove(out + size_t(count) * size_t(O) - size_t(count) * size_t(stride), comp, sizeof(float) * size_t(count) * size_t(stride));
    fdnn::lazy_expand_rows(out, count, size_t(O), size_t(stride), bits);
  } else {
    fdnn::lazy_expand_rows_from(out, comp, count, size_t(O), size_t(stride), bits);
  }
  lazy_expand_force_scalar(false);
  return FDNN_OK;
}

int fdnn_debug_set_l0_list_cap(fdnn_model *m, int cap) {
  if (!m || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  std::lock_guard<std::mutex> lk(m->mu);
  for (fdnn_ctx *c : m->pool) destroy_ctx(c);  // pooled contexts carry the old capacity
  m->pool.clear();
  m->l0_list_cap = cap;
  return FDNN_OK;
}

int fdnn_debug_set_pp(int mode, int min_frames) {
  if (mode < -1 || mode > 1) return fail(FDNN_E_ARG, "pp mode must be -1, 0 or 1");
  fdnn::sel::tuning().pp_mode = mode;
  fdnn::sel::tuning().pp_min = min_frames;
  return FDNN_OK;
}

int fdnn_debug_raise_fuse_fault(fdnn_model *m, int value) {
  if (!m) return fail(FDNN_E_ARG, "null model");
  if (!m->h_fuse_fault) return fail(FDNN_E_STATE, "this model has no fault word");
  __atomic_store_n(m->h_fuse_fault.p, value ? 1ull : 0ull, __ATOMIC_RELAXED);
  if (!value) m->fuse_fault_said = false;
  return FDNN_OK;
}

int fdnn_debug_set_ppo(int mode) {
  if (mode < -1 || mode > 1) return fail(FDNN_E_ARG, "ppo mode must be -1, 0 or 1");
  fdnn::sel::tuning().ppo_mode = mode;
  return FDNN_OK;
}

// ---- the launch recorder (fdnn_note.hpp)
int fdnn_debug_launch_name_count(void) { return fdnn::kLaunchNameCount; }

const char *fdnn_debug_launch_name(int index, int *flags) {
  if (index < 0 || index >= fdnn::kLaunchNameCount) return nullptr;
  if (flags) *flags = fdnn::kLaunchNames[index].flags;
  return fdnn::kLaunchNames[index].name;
}

int fdnn_debug_launch_record(int on) {
  fdnn::g_launch_note_on.store(on ? 1 : 0, std::memory_order_relaxed);
  return FDNN_OK;
}

int fdnn_debug_launch_reset(void) {
  for (auto &c : fdnn::g_launch_count) c.store(0, std::memory_order_relaxed);
  return FDNN_OK;
}

int fdnn_debug_launch_counts(unsigned long long *out, int cap) {
  if (!out || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  for (int i = 0; i < fdnn::kLaunchNameCount && i < cap; ++i) out[i] = fdnn::g_launch_count[i].load(std::memory_order_relaxed);
  return fdnn::kLaunchNameCount;
}

int fdnn_debug_set_chain(int mode, int min_frames) {
  if (mode < -1 || mode > 1) return fail(FDNN_E_ARG, "chain mode must be -1, 0 or 1");
  fdnn::sel::tuning().chain_mode = mode;
  fdnn::sel::tuning().chain_min = min_frames;
  return FDNN_OK;
}

int fdnn_debug_chain_clocks(fdnn_ctx *c, long long *out, int cap_tasks) {
  if (!c || cap_tasks <= 0) return fail(FDNN_E_ARG, "bad argument");
  DeviceGuard g(c->m->device);
  const size_t words = 8 + size_t(cap_tasks) * 10;
  if (!out) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->d_chain_clk.release();  // (a buffer of exactly this many tasks: the launch derives its task bound from the size)
    HIP_TRY(c->d_chain_clk.reserve(words));
    HIP_TRY(c->d_chain_clk.fill(0));
    HIP_TRY(hipDeviceSynchronize());
    return FDNN_OK;
  }
  if (words > c->d_chain_clk.count) return fail(FDNN_E_STATE, "no clock buffer of that size");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, c->d_chain_clk, words * sizeof(long long), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(c->d_chain_clk, 0, 8 * sizeof(long long)));
  HIP_TRY(hipDeviceSynchronize());
  return FDNN_OK;
}

// ---------------------------------------------------------------- taps
int fdnn_debug_forward_taps(fdnn_model *m, const float *x, int n, const int8_t *masks, float *l0_lin, uint8_t *u8_acts,
                            int32_t *acc_hid, int32_t *acc_out, float *logits, float *probs) {
  if (!m || !x || n <= 0) return fail(FDNN_E_ARG, "bad argument");
  DeviceGuard g(m->device);
  const BlobHeader &h = m->hm.hdr;
  const size_t H = size_t(h.hidden), O = size_t(h.out_dim), N = size_t(n);
  const int n_hidden = h.n_q;  // fp32 layer + (n_q - 1) int8 hidden layers
  fdnn_ctx *c = nullptr;
  int rc = make_ctx(m, n, &c);
  if (rc) return rc;
  fdnn::DevBuf<float> d_l0_lin, d_logits;
  fdnn::DevBuf<uint8_t> d_u8_acts;
  fdnn::DevBuf<int32_t> d_acc_hid, d_acc_out;
  hipError_t e = d_l0_lin.reserve(N * H);
  if (e == hipSuccess) e = d_u8_acts.reserve(size_t(n_hidden) * N * H);
  if (e == hipSuccess) e = d_acc_hid.reserve(size_t(std::max(n_hidden - 1, 1)) * N * H);
  if (e == hipSuccess) e = d_acc_out.reserve(N * O);
  if (e == hipSuccess) e = d_logits.reserve(N * O);
  const Taps t{d_l0_lin, d_u8_acts, d_acc_hid, d_acc_out, d_logits};
  hipStream_t s = c->stream;
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_x, x, sizeof(float) * N * h.in_dim, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && masks) e = hipMemcpyAsync(c->d_mask, masks, N * O, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    rc = run_hidden(c, c->d_x, s, &t);
    if (!rc) rc = run_output(c, {.count = n, .d_masks = masks ? c->d_mask : nullptr, .d_out = c->d_out, .taps = &t}, s);
  }
  auto fetch = [&](void *dst, const void *src, size_t bytes) {
    if (dst && e == hipSuccess && !rc) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
  };
  fetch(l0_lin, t.l0_lin, sizeof(float) * N * H);
  fetch(u8_acts, t.u8_acts, size_t(n_hidden) * N * H);
  fetch(acc_hid, t.acc_hid, sizeof(int32_t) * size_t(n_hidden - 1) * N * H);
  fetch(acc_out, t.acc_out, sizeof(int32_t) * N * O);
  fetch(logits, t.logits, sizeof(float) * N * O);
  fetch(probs, c->d_out, sizeof(float) * N * O);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  fdnn_ctx_free(c);
  if (rc) return rc;
  if (e != hipSuccess) return fail(FDNN_E_DEVICE, std::string("taps: ") + hipGetErrorString(e));
  return FDNN_OK;
}

int fdnn_debug_frame_chunks(int n, int *chunks, int cap) { return fdnn_debug_frame_chunks_for(n, 1, chunks, cap); }

int fdnn_debug_frame_chunks_for(int n, int chained, int *chunks, int cap) {
  if (n <= 0 || !chunks || cap <= 0) return -1;
  const auto v = fdnn::frame_chunks(n, nullptr, chained != 0);
  if (static_cast<int>(v.size()) > cap) return -1;
  for (size_t i = 0; i < v.size(); ++i) {
    chunks[2 * i] = v[i].first;
    chunks[2 * i + 1] = v[i].second;
  }
  return static_cast<int>(v.size());
}

int fdnn_debug_production_acc_out(fdnn_model *m, const float *x, int n, int stride, const int8_t *masks, int32_t *acc, float *probs) {
  if (!m || !x || !acc || n <= 0 || stride <= 0) return fail(FDNN_E_ARG, "bad argument");
  DeviceGuard g(m->device);
  const BlobHeader &h = m->hm.hdr;
  const size_t O = size_t(h.out_dim), N = size_t(n), NP = size_t((n + stride - 1) / stride);
  fdnn_ctx *c = nullptr;
  int rc = make_ctx(m, n, &c);
  if (rc) return rc;
  Taps t{};  // only the probe: hidden layers and output layer run their production instances
  t.probe_stride = stride;
  hipStream_t s = c->stream;
  fdnn::DevBuf<int32_t> d_probe;
  hipError_t e = d_probe.reserve(NP * O);
  t.acc_probe = d_probe;
  if (e == hipSuccess) e = hipMemsetAsync(t.acc_probe, 0xff, sizeof(int32_t) * NP * O, s);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_x, x, sizeof(float) * N * h.in_dim, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && masks) e = hipMemcpyAsync(c->d_mask, masks, N * O, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    rc = run_hidden(c, c->d_x, s, nullptr);
    if (!rc) rc = run_output(c, {.count = n, .d_masks = masks ? c->d_mask : nullptr, .d_out = c->d_out, .taps = &t}, s);
  }
  if (e == hipSuccess && !rc) e = hipMemcpyAsync(acc, t.acc_probe, sizeof(int32_t) * NP * O, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && !rc && probs) e = hipMemcpyAsync(probs, c->d_out, sizeof(float) * N * O, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  fdnn_ctx_free(c);
  if (rc) return rc;
  if (e != hipSuccess) return fail(FDNN_E_DEVICE, std::string("acc probe: ") + hipGetErrorString(e));
  return FDNN_OK;
}

int fdnn_debug_device_counters(fdnn_model *m, unsigned long long *out, int n) {  // raw device counter words (kernel clock stamps of timing builds live at [4..])
  if (!m || !out || n < 0 || n > 32) return fail(FDNN_E_ARG, "bad argument");
  if (!m->d_l0_stats) return fail(FDNN_E_STATE, "no counters");
  DeviceGuard g(m->device);
  const hipError_t e = hipMemcpy(out, m->d_l0_stats, sizeof(unsigned long long) * size_t(n), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(FDNN_E_DEVICE, std::string("device counters: ") + hipGetErrorString(e));
  return FDNN_OK;
}

// one of the model's device counters (fdnn_model::d_l0_stats); the copy synchronises with the device
static int read_counter(fdnn_model *m, int index, const char *what, unsigned long long *out) {
  if (!m || !out) return fail(FDNN_E_ARG, "null argument");
  *out = 0;
  if (!m->d_l0_stats) return FDNN_OK;
  DeviceGuard g(m->device);
  const hipError_t e = hipMemcpy(out, m->d_l0_stats + index, sizeof(*out), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(FDNN_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
  return FDNN_OK;
}

int fdnn_model_chain_faults(fdnn_model *m, unsigned long long *faults) { return read_counter(m, 3, "chain_faults", faults); }
int fdnn_model_fuse_giveups(fdnn_model *m, unsigned long long *tiles) { return read_counter(m, 2, "fuse_giveups", tiles); }

// Layer 0 alone, on a context of its own: u8_out [n][H]; with t_out / dd_out the int8 screening whatever the batch size
// and its t~ and Dd per output; *recomputed (may be null): outputs the screened path recomputed exactly.
static int debug_layer0(fdnn_model *m, const float *x, int n, uint8_t *u8_out, float *t_out, float *dd_out, unsigned long long *recomputed) {
  const bool screen = t_out != nullptr;
  DeviceGuard g(m->device);
  const BlobHeader &h = m->hm.hdr;
  fdnn_ctx *c = nullptr;
  int rc = make_ctx(m, n, &c);
  if (rc) return rc;
  const size_t outs = size_t(n) * h.hidden;
  unsigned long long before[2] = {0, 0}, after[2] = {0, 0};
  hipError_t e = hipSuccess;
  if (screen) {
    e = c->d_l0_dbg_t.reserve(outs);
    if (e == hipSuccess) e = c->d_l0_dbg_dd.reserve(outs);
    if (e == hipSuccess) e = c->d_l0_dbg_t.fill(0xff);  // NaN: an output the screening kernel did not visit
    if (e == hipSuccess) e = c->d_l0_dbg_dd.fill(0xff);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(before, m->d_l0_stats, sizeof(before), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_x, x, sizeof(float) * size_t(n) * h.in_dim, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    const int kernel_before = m->l0_kernel;
    if (screen && m->l0_kernel == 0) m->l0_kernel = 4;  // the int8 screening whatever the batch size
    run_layer0(c, c->d_x, c->stream, nullptr);  // the PRODUCTION instance (no taps): screened path for large batches
    m->l0_kernel = kernel_before;
    e = hipGetLastError();
  }
  std::vector<int8_t> tmp(size_t(n) * size_t(c->act_ld));
  if (e == hipSuccess) e = hipMemcpyAsync(tmp.data(), c->d_act[0], tmp.size(), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && screen) e = hipMemcpyAsync(t_out, c->d_l0_dbg_t, outs * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && screen) e = hipMemcpyAsync(dd_out, c->d_l0_dbg_dd, outs * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(after, m->d_l0_stats, sizeof(after), hipMemcpyDeviceToHost);
  const size_t act_ld = size_t(c->act_ld);
  fdnn_ctx_free(c);
  if (e != hipSuccess) return fail(FDNN_E_DEVICE, std::string(screen ? "layer 0 (screen debug): " : "layer 0: ") + hipGetErrorString(e));
  unpack_act_rows(tmp.data(), act_ld, n, h.hidden, u8_out);
  if (recomputed) *recomputed = after[1] - before[1];
  return FDNN_OK;
}

int fdnn_debug_layer0(fdnn_model *m, const float *x, int n, uint8_t *u8_out, unsigned long long *recomputed) {
  if (!m || !x || !u8_out || n <= 0) return fail(FDNN_E_ARG, "bad argument");
  return debug_layer0(m, x, n, u8_out, nullptr, nullptr, recomputed);
}

int fdnn_debug_layer0_screen(fdnn_model *m, const float *x, int n, uint8_t *u8_out, float *t_out, float *dd_out, unsigned long long *recomputed) {
  if (!m || !x || !u8_out || !t_out || !dd_out || n <= 0) return fail(FDNN_E_ARG, "bad argument");
  if (!m->d_w0d) return fail(FDNN_E_STATE, "this model's input layer has no int8 screening (input width outside 64..496)");
  return debug_layer0(m, x, n, u8_out, t_out, dd_out, recomputed);
}

// ---------------------------------------------------------------- the splice alone
// Host in, host out.  use_table: the raw frames and the table go up in ONE buffer laid out as a live batch of the scoring loop
// lays it out (fdnn::plan::live_table), and the table kernel runs; otherwise fdnn::splice_rows, as every other caller has it.
int fdnn_debug_splice_table(const int *offsets, int count, int raw_dim, int input_dim, const float *raw, int raw_frames, const int32_t *segs,
                            int n_segs, int rows, int use_table, float *x, int device) {
  if (!offsets || !raw || !segs || !x) return fail(FDNN_E_ARG, "null argument");
  if (count < 1 || count > fdnn::kSpliceMaxOffsets || raw_dim < 1 || input_dim < 4 || input_dim % 4 || input_dim < count * raw_dim)
    return fail(FDNN_E_ARG, "splice: 1 .. 64 offsets, an input width that is a multiple of 4 and holds count x raw_dim");
  if (raw_frames < 1 || rows < 1 || n_segs < 1 || n_segs > rows) return fail(FDNN_E_ARG, "splice: frames, rows and 1 .. rows segments");
  auto spec = std::make_shared<fdnn::SpliceSpec>();
  spec->offsets.assign(offsets, offsets + count);
  spec->raw_dim = raw_dim;
  fdnn::plan::BatchPlan b;
  b.spec = spec, b.raw = b.live = true, b.rows = rows, b.raw_frames = raw_frames;
  for (int g = 0; g < n_segs; ++g) {
    const int32_t *w = segs + 4 * size_t(g);
    // rows ascend from 0 inside [0, rows); a segment holds at least one frame of the buffer
    const bool row_ok = g ? w[0] > b.segs.back().row : w[0] == 0;
    if (!row_ok || w[0] >= rows || w[2] > w[3] || w[3] < 0 || w[2] >= raw_frames)
      return fail(FDNN_E_ARG, "splice: segment " + std::to_string(g) + " is malformed");
    b.segs.push_back(fdnn::SpliceSeg{w[0], w[1], w[2], w[3]});
  }
  DeviceGuard g(device);
  if (!g.ok) return fail(FDNN_E_DEVICE, "hipSetDevice failed");
  const fdnn::plan::LiveTable t = fdnn::plan::live_table(b);
  const size_t raw_words = size_t(raw_frames) * size_t(raw_dim), x_words = size_t(rows) * size_t(input_dim);
  std::vector<float> up(t.words, 0.0f);
  std::memcpy(up.data(), raw, sizeof(float) * raw_words);
  fdnn::plan::write_live_table(b, t, reinterpret_cast<int32_t *>(up.data()));
  fdnn::DevBuf<float> d_up, d_x;
  HIP_TRY(d_up.reserve(t.words));
  HIP_TRY(d_x.reserve(x_words));
  HIP_TRY(hipMemcpy(d_up, up.data(), sizeof(float) * t.words, hipMemcpyHostToDevice));
  const int32_t *d_table = reinterpret_cast<const int32_t *>(d_up.p);
  if (use_table)
    fdnn::splice_rows_table(*spec, input_dim, d_up, raw_frames, d_table + t.segs_at, d_table + t.row_seg_at, n_segs, rows, d_x, nullptr);
  else
    fdnn::splice_rows(*spec, input_dim, d_up, raw_frames, b.segs, 0, rows, d_x, nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(x, d_x, sizeof(float) * x_words, hipMemcpyDeviceToHost));
  return FDNN_OK;
}

int fdnn_debug_live_launches(unsigned long long *launches, unsigned long long *max_segs) {
  unsigned long long a = 0, b = 0;
  fdnn::splice_table_counts(&a, &b);
  if (launches) *launches = a;
  if (max_segs) *max_segs = b;
  return FDNN_OK;
}

// ---------------------------------------------------------------- per-kernel timing
int fdnn_profile_begin(fdnn_model *m) {
  if (!m) return fail(FDNN_E_ARG, "null model");
  std::lock_guard<std::mutex> lk(m->mu);
  for (auto &r : m->prof) {
    hipEventDestroy(r.a);
    hipEventDestroy(r.b);
  }
  m->prof.clear();
  m->profiling = true;
  return FDNN_OK;
}

int fdnn_profile_end(fdnn_model *m, double *ms, int *launches) {
  if (!m || !ms || !launches) return fail(FDNN_E_ARG, "null argument");
  DeviceGuard g(m->device);
  std::vector<fdnn_model::ProfRec> recs;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    m->profiling = false;
    recs.swap(m->prof);
  }
  for (int k = 0; k < FDNN_PROF_KINDS; ++k) {
    ms[k] = 0.0;
    launches[k] = 0;
  }
  int rc = FDNN_OK;
  for (auto &r : recs) {
    float t = 0.0f;
    hipError_t e = hipEventSynchronize(r.b);
    if (e == hipSuccess) e = hipEventElapsedTime(&t, r.a, r.b);
    if (e == hipSuccess) {
      ms[r.kind] += t;
      launches[r.kind]++;
    } else {
      rc = fail(FDNN_E_DEVICE, std::string("profile: ") + hipGetErrorString(e));
    }
    hipEventDestroy(r.a);
    hipEventDestroy(r.b);
  }
  return rc;
}

// ---------------------------------------------------------------- host-only helpers
int fdnn_host_model_load(const char *path, float cutoff, fdnn_host_model **out) {
  if (!path || !out) return fail(FDNN_E_ARG, "null argument");
  *out = nullptr;
  fdnn_host_model *hm = new fdnn_host_model();
  std::string msg;
  int rc = fdnn::load_host_model(path, cutoff, &hm->hm, &msg);
  if (rc) {
    delete hm;
    return fail(rc, msg);
  }
  *out = hm;
  return FDNN_OK;
}

void fdnn_host_model_free(fdnn_host_model *hm) { delete hm; }
int fdnn_host_model_layers(const fdnn_host_model *hm) { return hm ? hm->hm.hdr.n_affine : -1; }

int fdnn_host_model_layer_in(const fdnn_host_model *hm, int j) {
  if (!hm || j < 0 || j >= hm->hm.hdr.n_affine) return -1;
  return j == 0 ? hm->hm.hdr.in_dim : hm->hm.hdr.q[j - 1].cols;
}

int fdnn_host_model_layer_out(const fdnn_host_model *hm, int j) {
  if (!hm || j < 0 || j >= hm->hm.hdr.n_affine) return -1;
  return j == 0 ? hm->hm.hdr.hidden : hm->hm.hdr.q[j - 1].rows;
}

float fdnn_host_model_multiplier(const fdnn_host_model *hm, int j) {
  if (!hm || j < 1 || j >= hm->hm.hdr.n_affine) return 0.0f;
  return hm->hm.hdr.q[j - 1].mult;
}

int fdnn_host_model_weights_q(const fdnn_host_model *hm, int j, int8_t *out) {
  if (!hm || !out || j < 1 || j >= hm->hm.hdr.n_affine) return fail(FDNN_E_ARG, "bad layer index");
  const QLayerDesc &d = hm->hm.hdr.q[j - 1];
  const int8_t *w = hm->hm.wq(j - 1);
  for (int r = 0; r < d.rows; ++r) std::memcpy(out + size_t(r) * d.cols, w + size_t(r) * d.cols_pad, size_t(d.cols));
  return FDNN_OK;
}

int fdnn_host_model_bias(const fdnn_host_model *hm, int j, float *out) {
  if (!hm || !out || j < 0 || j >= hm->hm.hdr.n_affine) return fail(FDNN_E_ARG, "bad layer index");
  if (j == 0)
    std::memcpy(out, hm->hm.b0(), sizeof(float) * size_t(hm->hm.hdr.hidden));
  else
    std::memcpy(out, hm->hm.bias(j - 1), sizeof(float) * size_t(hm->hm.hdr.q[j - 1].rows));
  return FDNN_OK;
}

int fdnn_host_model_wsum128(const fdnn_host_model *hm, int j, int32_t *out) {
  if (!hm || !out || j < 1 || j >= hm->hm.hdr.n_affine) return fail(FDNN_E_ARG, "bad layer index");
  std::memcpy(out, hm->hm.wsum(j - 1), sizeof(int32_t) * size_t(hm->hm.hdr.q[j - 1].rows));
  return FDNN_OK;
}

long long fdnn_host_model_risky_pairs(const fdnn_host_model *hm, int j) {
  if (!hm || j < 1 || j >= hm->hm.hdr.n_affine) return -1;
  return hm->hm.hdr.q[j - 1].n_fix;
}

size_t fdnn_host_model_blob_size(const fdnn_host_model *hm) { return hm ? hm->hm.blob.size() : 0; }

int fdnn_host_model_blob(const fdnn_host_model *hm, void *out, size_t capacity) {
  if (!hm || !out) return fail(FDNN_E_ARG, "null argument");
  if (capacity < hm->hm.blob.size()) return fail(FDNN_E_ARG, "destination smaller than the blob");
  std::memcpy(out, hm->hm.blob.data(), hm->hm.blob.size());
  return FDNN_OK;
}

int fdnn_host_blob_check(const void *bytes, size_t size, int *input_dim, int *hidden_dim, int *output_dim,
                         int *n_affine) {
  if (!bytes) return fail(FDNN_E_ARG, "null argument");
  std::vector<uint8_t> copy(static_cast<const uint8_t *>(bytes), static_cast<const uint8_t *>(bytes) + size);
  fdnn::HostModel hm;
  std::string msg;
  int rc = fdnn::adopt_blob(std::move(copy), &hm, &msg);
  if (rc) return fail(rc, msg);
  if (input_dim) *input_dim = hm.hdr.in_dim;
  if (hidden_dim) *hidden_dim = hm.hdr.hidden;
  if (output_dim) *output_dim = hm.hdr.out_dim;
  if (n_affine) *n_affine = hm.hdr.n_affine;
  return FDNN_OK;
}

int fdnn_host_sigmoid_lut(uint8_t *out) {
  if (!out) return fail(FDNN_E_ARG, "null argument");
  fdnn::build_sigmoid_lut(out);
  return FDNN_OK;
}

int fdnn_host_quantize(const float *w, int rows, int cols, float cutoff, int8_t *out, float *multiplier) {
  if (!w || !out || !multiplier || rows <= 0 || cols <= 0) return fail(FDNN_E_ARG, "bad argument");
  fdnn::quantize_layer(w, rows, cols, cutoff, out, multiplier);
  return FDNN_OK;
}

}  // extern "C"
