// fdnn_runtime.cpp -- device model, calculation contexts and the passes over them; the C-ABI that drives them
// (include/fdnn.h) is fdnn_api.cpp, the debug / profiling / host-model calls fdnn_debug.cpp.
//
// Host-side counterpart of the reference's QuantizedDnn (dnn.h:106-142) and
// CalculationContext (dnn.h:144-208, dnn.cc:194-215, :402-454), re-designed for
// one MI355X: the model is one immutable packed blob in HBM; a context is a set
// of persistent device scratch buffers sized for n frames plus its own stream;
// fdnn_calculate draws contexts from a per-model pool so that concurrent callers
// (MultiThreadedStressTest.java:48-69) never share scratch.
#include <hip/hip_runtime.h>
#include <immintrin.h>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fdnn_internal.hpp"
#include "fdnn_lists.hpp"

namespace {
thread_local std::string g_err;
}  // namespace

namespace fdnn {
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
}  // namespace fdnn

namespace fdnn {

int upload_model(fdnn_model *m) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(FDNN_E_DEVICE, "no HIP device available: this library has no CPU path");
  if (m->device < 0 || m->device >= count) return fail(FDNN_E_ARG, "device index out of range");
  DeviceGuard g(m->device);
  if (!g.ok) return fail(FDNN_E_DEVICE, "hipSetDevice failed");
  HIP_TRY(m->d_blob.reserve(m->hm.blob.size()));
  // exhaustive validation of the 3-op division per layer (see dequant() in fdnn_kernels.hip)
  DevBuf<unsigned long long> d_bad;
  HIP_TRY(d_bad.reserve(fdnn::kMaxQLayers));
  HIP_TRY(d_bad.fill(0));
  BlobHeader &h = m->hm.hdr;
  for (int qi = 0; qi < h.n_q; ++qi) {
    // same coefficient as an earlier layer -> same verdict, skip the sweep (every int8 layer has the hidden width for K:
    // one cols_pad, one range)
    int same = -1;
    for (int pj = 0; pj < qi; ++pj)
      if (h.q[pj].coef == h.q[qi].coef) same = pj;
    if (same >= 0) continue;
    // the layer's own accumulator range: cols_pad / 2 pairs, each saturated to int16 (2^26 at K = 4096, 2^29 at 32 768)
    const long long acc_bound = static_cast<long long>(h.q[qi].cols_pad / 2) * 32768;
    fdnn::launch_fastdiv_check(h.q[qi].coef, h.q[qi].rcp_coef, acc_bound, d_bad + qi, nullptr);
  }
  unsigned long long bad[fdnn::kMaxQLayers];
  HIP_TRY(hipMemcpy(bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
  for (int qi = 0; qi < h.n_q; ++qi) {
    int src = qi;
    for (int pj = 0; pj < qi; ++pj)
      if (h.q[pj].coef == h.q[qi].coef) {
        src = pj;
        break;
      }
    // the fast epilogue = validated 3-op division + half-step table (needs bounded |lin|)
    h.q[qi].fastdiv_ok = (bad[src] == 0 && h.q[qi].lin_bounded) ? 1 : 0;
  }
  std::memcpy(m->hm.blob.data(), &h, sizeof(h));
  HIP_TRY(hipMemcpy(m->d_blob, m->hm.blob.data(), m->hm.blob.size(), hipMemcpyHostToDevice));
  return build_l0_image(m);
}

// Layer-0 weight image for the chain-pass kernel, built on the device from the blob's [H][D] rows.
int build_l0_image(fdnn_model *m) {
  const BlobHeader &h = m->hm.hdr;
  m->l0_jc = fdnn::l0_chunk_rows(h.in_dim);
  m->l0_j_pad = round_up(h.in_dim / 4, m->l0_jc);
  m->l0_h_ld = round_up(h.hidden, 128);
  HIP_TRY(m->d_w0t.reserve(4 * size_t(m->l0_j_pad) * m->l0_h_ld));
  fdnn::launch_l0_weight_image(reinterpret_cast<const float *>(m->d_blob + h.off_w0), m->d_w0t, h.hidden, h.in_dim, m->l0_j_pad,
                               m->l0_h_ld, nullptr);
  HIP_TRY(hipGetLastError());
  // ||w_n||_2 per layer-0 node, in double, rounded up to float: with the frame norms it bounds sum_k |x_k w_k| of every
  // output (Cauchy-Schwarz) for the screened path (fdnn_l0.hip)
  {
    const float *w0 = m->hm.w0();
    std::vector<float> wn(size_t(h.hidden));
    for (int i = 0; i < h.hidden; ++i) {
      double acc = 0.0;
      for (int k = 0; k < h.in_dim; ++k) acc += double(w0[size_t(i) * h.in_dim + k]) * double(w0[size_t(i) * h.in_dim + k]);
      const double up = std::sqrt(acc) * (1.0 + 1e-6);
      float f = float(up);
      if (double(f) < up) f = std::nextafter(f, std::numeric_limits<float>::infinity());
      wn[size_t(i)] = f;  // inf / NaN weights stay inf / NaN: every output of that node is then recomputed exactly
    }
    HIP_TRY(m->d_w0norm.reserve(wn.size()));
    HIP_TRY(hipMemcpy(m->d_w0norm, wn.data(), sizeof(float) * wn.size(), hipMemcpyHostToDevice));
    if (sel::l0_split_ok(h.in_dim, h.hidden)) {  // the node half of the int8 screening (fdnn_l0s.hip): digit planes + constants
      std::vector<int8_t> planes;
      std::vector<float> stat;
      std::vector<uint32_t> pairs;
      fdnn::l0_split_build_weights(w0, wn.data(), m->hm.blob.data() + h.off_lut2, h.hidden, h.in_dim, m->l0_h_ld, &planes, &stat, &pairs);
      HIP_TRY(m->d_lutpair.reserve(pairs.size()));
      HIP_TRY(hipMemcpy(m->d_lutpair, pairs.data(), sizeof(uint32_t) * pairs.size(), hipMemcpyHostToDevice));
      HIP_TRY(m->d_w0d.reserve(planes.size()));
      HIP_TRY(hipMemcpy(m->d_w0d, planes.data(), planes.size(), hipMemcpyHostToDevice));
      HIP_TRY(m->d_w0stat.reserve(stat.size()));
      HIP_TRY(hipMemcpy(m->d_w0stat, stat.data(), sizeof(float) * stat.size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(m->d_l0_stats.reserve(32));
    HIP_TRY(m->d_l0_stats.fill(0));
    if (m->h_fuse_fault.reserve(1) != hipSuccess) (void)hipGetLastError();  // refused: stays null, the model goes on without
    if (m->h_fuse_fault) *m->h_fuse_fault.p = 0;
  }
  if (int rc = build_lists_index(m)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return FDNN_OK;
}

// The output layer's saturating pairs per node, for the list kernels (fdnn_lists.hip): a side buffer of the model, from
// the blob's group-ordered entries.  The blob, its version and its bytes stay as they are.
int build_lists_index(fdnn_model *m) {
  const BlobHeader &h = m->hm.hdr;
  const QLayerDesc &d = h.q[h.n_q - 1];
  if (d.n_fix <= 0) return FDNN_OK;
  std::vector<int32_t> off;
  std::vector<uint32_t> pairs;
  lists::build_node_fix_index(reinterpret_cast<const FixEntry *>(m->hm.blob.data() + d.off_fix_ent),
                              reinterpret_cast<const int32_t *>(m->hm.blob.data() + d.off_fix_grp), d.rows, d.rows_pad, &off, &pairs);
  HIP_TRY(m->d_lfix_off.reserve(off.size()));
  HIP_TRY(m->d_lfix_pairs.reserve(std::max<size_t>(pairs.size(), 1)));
  HIP_TRY(hipMemcpy(m->d_lfix_off, off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice));
  if (!pairs.empty()) HIP_TRY(hipMemcpy(m->d_lfix_pairs, pairs.data(), sizeof(uint32_t) * pairs.size(), hipMemcpyHostToDevice));
  return FDNN_OK;
}

void destroy_ctx(fdnn_ctx *c) {
  if (!c) return;
  DeviceGuard g(c->m->device);  // (for the buffers' destructors too)
  if (c->stream) {
    fuse_chain_retire_stream(c->m->device, c->stream);
    hipStreamSynchronize(c->stream);
  }
  scratch_audit_event(c);  // (fdnn_debug_scratch_audit: nothing unless switched on)
  if (c->done) hipEventDestroy(c->done);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

int make_ctx(fdnn_model *m, int n, fdnn_ctx **out, bool lean) {
  DeviceGuard g(m->device);
  if (!g.ok) return fail(FDNN_E_DEVICE, "hipSetDevice failed");
  const BlobHeader &h = m->hm.hdr;
  int max_rows_pad = 0;
  for (int qi = 0; qi < h.n_q; ++qi) max_rows_pad = std::max(max_rows_pad, h.q[qi].rows_pad);
  const CtxLayout l = ctx_layout({h.in_dim, h.hidden, h.out_dim, max_rows_pad, m->l0_j_pad, m->l0_h_ld, m->d_w0d != nullptr,
                                  sel::tuning().l0_chain_tn, m->l0_list_cap, lean, n});
  fdnn_ctx *c = new fdnn_ctx();
  c->m = m;
  c->n = n;
  c->cap = l.cap;
  c->act_ld = l.act_ld;
  c->xt_ld = l.xt_ld;
  hipError_t e = hipSuccess;
  // one allocation per buffer, in this order; an empty one still gets 16 bytes
  auto alloc = [&](auto &buf, size_t count) {
    if (e == hipSuccess) e = buf.reserve(count ? count : 16 / sizeof(*buf.p));
  };
  auto zero = [&](auto &buf, size_t count) {  // (a counter array the kernels keep zero; nothing for an empty one)
    if (e == hipSuccess) e = hipMemset(buf, 0, sizeof(*buf.p) * count);
  };
  if (!lean) alloc(c->d_x, l.x);
  alloc(c->d_xt, l.xt);
  alloc(c->d_scr_count, l.scr_count);
  alloc(c->d_scr_list, l.scr_list);
  zero(c->d_scr_count, l.scr_count);
  if (m->d_w0d) {
    alloc(c->d_xd, l.xd);
    alloc(c->d_xstat, l.xstat);
    alloc(c->d_glist, size_t(l.glist_cap));
    alloc(c->d_glist_count, l.glist_count);
    zero(c->d_glist, size_t(l.glist_cap));
    zero(c->d_glist_count, l.glist_count);
  }
  if (l.l0park) alloc(c->d_l0park, l.l0park);
  alloc(c->d_act[0], l.act);
  alloc(c->d_act[1], l.act);
  if (!lean) alloc(c->d_out, l.out);
  alloc(c->d_partial, l.partial);
  if (!lean) alloc(c->d_mask, l.mask);
  alloc(c->d_mask_bits, l.mask_bits);
  alloc(c->d_fuse_s, l.fuse_s);
  alloc(c->d_fuse_cnt, l.fuse_cnt);
  alloc(c->d_fuse_flag, l.fuse_flag);
  zero(c->d_fuse_cnt, l.fuse_cnt);
  zero(c->d_fuse_flag, l.fuse_flag);
  alloc(c->d_chain_ctl, l.chain_ctl);
  alloc(c->d_chain_done, l.chain_done);
  zero(c->d_chain_ctl, l.chain_ctl);
  zero(c->d_chain_done, l.chain_done);
  if (e == hipSuccess && c->h_chain_fault.reserve(1) == hipSuccess) *c->h_chain_fault.p = 0;  // (refused: stays null, nobody listens)
  if (e == hipSuccess && !lean) e = c->h_mask_pin.reserve(l.mask_pin);
  if (e == hipSuccess && !lean) e = c->h_out_pin.reserve(l.out_pin);
  // The hipMemsets above are ordered on the NULL stream and return before they have run; the context's kernels go to
  // non-blocking streams, which do not wait for it.  Without this wait a new context's first kernels could start first and
  // have their counters (flagged-output list, fused soft-max arrivals) zeroed under them: a partly walked list -- a few
  // layer-0 bytes left at their screened value -- or a frame tile waiting for arrivals that were wiped.  Seen as one failure
  // in ten of the many-streams test (contexts are created while other callers' kernels run), never in a single-stream run.
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done, hipEventDisableTiming | hipEventDisableSystemFence);  // (orders streams of one device only: no system-scope flush per record)
  if (e != hipSuccess) {
    std::string msg = std::string("context allocation for ") + std::to_string(n) + " frames: " + hipGetErrorString(e);
    destroy_ctx(c);
    return fail(e == hipErrorOutOfMemory ? FDNN_E_NOMEM : FDNN_E_DEVICE, msg);
  }
  *out = c;
  return FDNN_OK;
}

// Row `row` of the self-rewinding scratch table (kCtxScratch, fdnn_ctx_layout.hpp) in this context: the buffer make_ctx
// allocated and zeroed for it, all of its words -- not only those some launch reaches.
ScratchBuf ctx_scratch_buf(fdnn_ctx *c, int row) {
  switch (row) {
    case kScrCount: return {c->d_scr_count.p, c->d_scr_count.count};
    case kFuseCnt: return {c->d_fuse_cnt.p, c->d_fuse_cnt.count};
    case kFuseFlag: return {c->d_fuse_flag.p, c->d_fuse_flag.count};
    case kChainCtl: return {c->d_chain_ctl.p, c->d_chain_ctl.count};
    case kChainDone: return {c->d_chain_done.p, c->d_chain_done.count};
    default: return {nullptr, 0};
  }
}

// one device-side u8 snapshot of the s8 activation buffer (taps only)
int snapshot_acts(const fdnn_ctx *c, int buf, uint8_t *d_dst, hipStream_t s) {
  const BlobHeader &h = c->m->hm.hdr;
  // compact [n_pad][act_ld] -> [n][H] while flipping bit 7
  if (c->act_ld == h.hidden) {
    fdnn::launch_xor80(c->d_act[buf], d_dst, size_t(c->n) * h.hidden, s);
  } else {
    for (int f = 0; f < c->n; ++f)
      fdnn::launch_xor80(c->d_act[buf] + size_t(f) * c->act_ld, d_dst + size_t(f) * h.hidden, size_t(h.hidden), s);
  }
  return FDNN_OK;
}

// CUs of a device, asked once per device (256 where the runtime cannot say): the rules and the persistent kernels' grids
// take it for the model's device
int device_cus(int device) {
  static std::atomic<int> cus[64];
  int n_cu = cus[device & 63].load(std::memory_order_relaxed);
  if (n_cu == 0) {
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu <= 0) n_cu = 256;
    cus[device & 63].store(n_cu, std::memory_order_relaxed);
  }
  return n_cu;
}

sel::LayerShape layer_shape(const QLayerDesc &d, bool output) {
  return {d.rows, d.rows_pad, d.cols_pad - fdnn::kRowSkew, d.fastdiv_ok != 0, d.n_fix > 0, output};
}

// GEMM descriptor of one int8 layer over `n` frames starting at activation row
// `act`, with the tiles of the choice made for this call (sel::choose_layer).
fdnn::QGemmParams prepare_qlayer(fdnn_ctx *c, const QLayerDesc &d, const int8_t *act, int n, const sel::LayerChoice &ch) {
  fdnn_model *m = c->m;
  const BlobHeader &h = m->hm.hdr;
  const uint8_t *B = m->d_blob;
  fdnn::QGemmParams g{};
  g.small = ch.form == sel::Form::small ? 1 : 0;
  g.frame_tile = ch.frame_tile;
  g.node_tile = ch.node_tile;
  g.debug = sel::tuning().gemm_debug;
  g.n = n;
  g.n_pad = ch.n_pad;
  if (d.n_fix > 0) {
    g.fix_grp = reinterpret_cast<const int32_t *>(B + d.off_fix_grp);
    g.fix_ent = B + d.off_fix_ent;
  }
  g.w = reinterpret_cast<const int8_t *>(B + d.off_w);
  g.a = act;
  g.bias = reinterpret_cast<const float *>(B + d.off_bias);
  g.wsum = reinterpret_cast<const int32_t *>(B + d.off_wsum);
  g.lut = B + h.off_lut;
  g.lut2 = B + h.off_lut2;
  g.rows = d.rows;
  g.rows_pad = d.rows_pad;
  g.K = d.cols_pad - fdnn::kRowSkew;
  g.ldw = d.cols_pad;
  g.lda = c->act_ld;
  g.coef = d.coef;
  g.rcp_coef = d.rcp_coef;
  g.fastdiv = d.fastdiv_ok;
  return g;
}

// Layer 0 of the context's n frames into d_act[0] (shift/scale, fp32 affine, bias, table).
void run_layer0(fdnn_ctx *c, const float *d_x, hipStream_t s, const Taps *taps) {
  fdnn_model *m = c->m;
  const BlobHeader &h = m->hm.hdr;
  const uint8_t *B = m->d_blob;
  fdnn::L0Params l0{};
  l0.x = d_x;
  l0.shift = reinterpret_cast<const float *>(B + h.off_shift);
  l0.scale = reinterpret_cast<const float *>(B + h.off_scale);
  l0.w = reinterpret_cast<const float *>(B + h.off_w0);
  l0.bias = reinterpret_cast<const float *>(B + h.off_b0);
  l0.lut = B + h.off_lut;
  l0.act_out = c->d_act[0];
  l0.act_ld = c->act_ld;
  l0.tap_lin = taps ? taps->l0_lin : nullptr;
  l0.n = c->n;
  l0.n_rows = c->n;
  l0.D = h.in_dim;
  l0.H = h.hidden;
  l0.fma = m->l0_fma;
  l0.kernel = m->l0_kernel;
  l0.xt = c->d_xt;
  l0.wt = m->d_w0t;
  l0.park = c->d_l0park;
  l0.wnorm = m->d_w0norm;
  l0.scr_count = c->d_scr_count;
  l0.scr_list = c->d_scr_list;
  l0.scr_stats = m->d_l0_stats;
  l0.xd = c->d_xd;
  l0.xstat = c->d_xstat;
  l0.wd = m->d_w0d;
  l0.wstat = m->d_w0stat;
  l0.luthalf = m->d_lutpair;
  l0.glist = c->d_glist;
  l0.glist_count = c->d_glist_count;
  l0.glist_cap = int(c->d_glist.count);
  l0.dbg_t = c->d_l0_dbg_t;
  l0.dbg_dd = c->d_l0_dbg_dd;
  l0.j_pad = m->l0_j_pad;
  l0.jc = m->l0_jc;
  l0.n_ld = c->xt_ld;
  l0.h_ld = m->l0_h_ld;
  const sel::L0Call call{l0.D, l0.H, l0.h_ld, l0.n, l0.n_rows, l0.fma != 0, l0.kernel, l0.tap_lin != nullptr, l0.xt && l0.wt, l0.wnorm && l0.scr_count && l0.scr_list,
                               l0.xd && l0.xstat && l0.wd && l0.wstat && l0.luthalf && l0.glist && l0.glist_count && l0.scr_count && l0.scr_list};
  {
    ProfScope ps(m, s, FDNN_PROF_L0);
    fdnn::launch_l0(l0, sel::choose_l0(call, sel::tuning()), s);
  }
}

// CalculateUntilLastHiddenLayer (dnn.cc:402-424): layer 0, then every int8
// hidden layer, layer-major over the whole frame batch.
int run_hidden(fdnn_ctx *c, const float *d_x, hipStream_t s, const Taps *taps) {
  fdnn_model *m = c->m;
  const BlobHeader &h = m->hm.hdr;
  run_layer0(c, d_x, s, taps);
  int cur = 0;
  if (taps && taps->u8_acts) snapshot_acts(c, cur, taps->u8_acts, s);
  // Large batches, no taps: the int8 hidden layers as ONE persistent launch (fdnn_chain.hip) -- tasks (layer, frame tile,
  // node tile) drawn from per-XCD queues, each waiting only for its own frame tile's node tiles of the layer before.
  const int n_hid = h.n_q - 1;
  // (advisor, round 5) a chained launch of this context ran into its wait bound: its counters are dirty and its results
  // were wrong.  Re-zero the counters in stream order and never chain on this context again; the host-synchronising dense
  // call re-runs its pass (calculate_on_one_device), the others observe fdnn_model_chain_faults.
  if (c->h_chain_fault && __atomic_load_n(c->h_chain_fault.p, __ATOMIC_RELAXED) != 0 && !c->chain_broken) {
    c->chain_broken = true;
    (void)hipMemsetAsync(c->d_chain_ctl, 0, sizeof(uint32_t) * c->d_chain_ctl.count, s);
    (void)hipMemsetAsync(c->d_chain_done, 0, sizeof(uint32_t) * c->d_chain_done.count, s);
  }
  const sel::Tuning &tune = sel::tuning();
  const int n_cu = device_cus(m->device);
  const sel::HiddenPlan plan = sel::plan_hidden(n_hid, [&](int i) { return layer_shape(h.q[i], false); }, c->n,
                                                            !taps && c->d_chain_ctl != nullptr && !c->chain_broken, tune, {n_cu});
  if (plan.chain) {
    const uint8_t *B = m->d_blob;
    for (int q0 = 0; q0 < n_hid; q0 += fdnn::kMaxChainLayers) {
      const int nl = sel::chain_segment(n_hid, q0);
      fdnn::QChainParams g{};
      for (int i = 0; i < nl; ++i) {
        const QLayerDesc &d = h.q[q0 + i];
        fdnn::QChainLayer &L = g.layer[i];
        L.w = reinterpret_cast<const int8_t *>(B + d.off_w);
        L.bias = reinterpret_cast<const float *>(B + d.off_bias);
        L.wsum = reinterpret_cast<const int32_t *>(B + d.off_wsum);
        L.fix_grp = d.n_fix > 0 ? reinterpret_cast<const int32_t *>(B + d.off_fix_grp) : nullptr;
        L.fix_ent = d.n_fix > 0 ? B + d.off_fix_ent : nullptr;
        L.coef = d.coef;
        L.rcp_coef = d.rcp_coef;
      }
      g.n_layers = nl;
      g.act[0] = c->d_act[cur];
      g.act[1] = c->d_act[cur ^ 1];
      g.lut2 = B + h.off_lut2;
      g.rows = h.q[0].rows;
      g.rows_pad = h.q[0].rows_pad;
      g.K = h.q[0].cols_pad - fdnn::kRowSkew;
      g.ldw = h.q[0].cols_pad;
      g.lda = c->act_ld;
      g.n = c->n;
      g.frame_tile = plan.frame_tile;
      g.n_pad = plan.n_pad;
      g.ctl = c->d_chain_ctl;
      g.done = c->d_chain_done;
      g.faults = m->d_l0_stats ? m->d_l0_stats + 3 : nullptr;
      g.fault_flag = c->h_chain_fault.dev;
      g.clk = c->d_chain_clk;
      g.clk_cap = c->d_chain_clk ? int((c->d_chain_clk.count - 8) / 10) : 0;  // [8 + tasks * 10] words
      {
        ProfScope ps(m, s, FDNN_PROF_HIDDEN);
        fdnn::launch_qchain(g, n_cu, s);
      }
      cur ^= nl & 1;
    }
    c->last = cur;
    HIP_TRY(hipGetLastError());
    return FDNN_OK;
  }
  for (int qi = 0; qi < h.n_q - 1; ++qi) {
    sel::LayerCall call{c->n, qi};
    call.tap_acc = taps && taps->acc_hid;
    const sel::LayerChoice ch = sel::choose_layer(layer_shape(h.q[qi], false), call, tune);
    fdnn::QGemmParams g = prepare_qlayer(c, h.q[qi], c->d_act[cur], c->n, ch);
    g.act_out = c->d_act[cur ^ 1];
    g.act_ld = c->act_ld;
    g.tap_acc = call.tap_acc ? taps->acc_hid + size_t(qi) * c->n * h.hidden : nullptr;
    {
      ProfScope ps(m, s, FDNN_PROF_HIDDEN);
      if (ch.form == sel::Form::pp) fdnn::launch_qpp_hidden(g, n_cu, s);
      else if (ch.form == sel::Form::small) fdnn::launch_qgemm_small_hidden(g, ch.small_ntm, s);
      else fdnn::launch_qgemm_hidden(g, ch.shape, s);
    }
    cur ^= 1;
    if (taps && taps->u8_acts) snapshot_acts(c, cur, taps->u8_acts + size_t(qi + 1) * c->n * h.hidden, s);
  }
  c->last = cur;
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

// CalculateOutput (dnn.cc:428-454) / LazyOutputActivations (dnn.cc:355-392)
// over frames [first, first+count) of the context's last hidden activations.
// Rows [first+count, first+n_pad) are read by the GEMM as padding frames; the
// activation buffers carry one tile of slack rows for that.
// Two PROCESSES on one GPU.  Inside a process the fused soft-max launches of a device are chained (FuseChain below); two
// processes cannot be, and their fused kernels' workgroups can hold each other's CUs while every one of them sits out its
// bounded wait (correct results, ~100 x the latency).  So the first process to load a model on a device takes an advisory
// lock on /dev/shm/fdnn-gpu-<pci bus id> and keeps it for its lifetime; a process that finds the lock taken runs the
// UNFUSED output path (output kernel + scale pass: nothing in it waits for another workgroup) and says so once on stderr.
// The chained hidden-layer kernel needs no such care: its tasks only ever wait for tasks drawn earlier (fdnn_chain.hip).
// FDNN_FUSE_NORM=0 / 1 in the environment forces the unfused / fused path regardless.  Two containers that share a GPU but
// not /dev/shm cannot see each other: set FDNN_FUSE_NORM=0 there.
int device_marker_state(int device) {  // 1 = this process owns the device's marker (or cannot tell), 0 = another process does
  static std::mutex mu;
  static int state[64];
  static bool known[64];
  std::lock_guard<std::mutex> lk(mu);
  const int d = device & 63;
  if (known[d]) return state[d];
  known[d] = true;
  state[d] = 1;
  char bus[64] = "";
  if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess || !bus[0]) std::snprintf(bus, sizeof(bus), "dev%d", device);
  for (char *q = bus; *q; ++q)
    if (*q == ':' || *q == '/') *q = '-';
  // The marker is ADVISORY (advisor, round 5): a world-writable lock file in a sticky directory.  Never follow a planted
  // symlink (O_NOFOLLOW), only touch the mode of a regular file this user owns, and do not wander to another directory when
  // /dev/shm is unusable -- two processes looking in different places would both believe they are alone: "cannot tell" is
  // treated as SHARED (the unfused soft-max: correct, a little slower) and said once.
  const std::string path = std::string("/dev/shm/fdnn-gpu-") + bus;
  const int fd = open(path.c_str(), O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0666);
  if (fd < 0) {
    state[d] = 0;
    std::fprintf(stderr, "fast-dnn: cannot open the device marker %s (%s): assuming GPU %s is shared -- unfused soft-max (FDNN_FUSE_NORM=1 overrides)\n",
                 path.c_str(), std::strerror(errno), bus);
    return state[d];
  }
  struct stat st {};
  if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_uid == geteuid()) fchmod(fd, 0666);
  if (flock(fd, LOCK_EX | LOCK_NB) == 0) return state[d];  // (kept open: the lock lives as long as this process)
  close(fd);
  state[d] = 0;
  std::fprintf(stderr, "fast-dnn: another process is scoring on GPU %s: this one runs the unfused soft-max (fdnn_device_shared)\n", bus);
  return state[d];
}
// The model's own evidence (see fdnn_model::h_fuse_fault): once a fused launch of this model has given up, it does not fuse again.
static bool model_may_fuse(fdnn_model *m) {
  if (!m->h_fuse_fault || __atomic_load_n(m->h_fuse_fault.p, __ATOMIC_RELAXED) == 0) return true;
  if (!m->fuse_fault_said) {
    m->fuse_fault_said = true;
    std::fprintf(stderr,
                 "fast-dnn: a fused soft-max launch on GPU %d sat out its bounded wait (another process scoring on this GPU that the device marker "
                 "did not show?): this model runs the unfused soft-max from here on (fdnn_model_fuse_giveups counts; FDNN_FUSE_NORM=1 overrides)\n",
                 m->device);
  }
  return sel::tuning().fuse_norm == 1 || sel::tuning().fuse_mode == 1;
}

static bool process_may_fuse(int device) {
  const int o = sel::tuning().fuse_mode;  // fdnn_debug_set_fuse: -1 = by environment / device marker, 0 = never, 1 = always
  if (o >= 0) return o == 1;
  const int forced = sel::tuning().fuse_norm;
  if (forced >= 0) return forced == 1;
  return device_marker_state(device) == 1;
}

// One chain of fused soft-max launches per device (see run_output).
struct FuseChain {
  std::mutex mu;
  hipEvent_t ev = nullptr;  // recorded after the device's latest fused output launch -- at once on a caller's stream;
  bool recorded = false;    // on a durable stream (stream_is_durable) only when a launch on ANOTHER stream needs it:
  bool pending = false;     // `pending` = the latest launch went to last_stream and `ev` does not cover it yet
  hipStream_t last_stream = nullptr;
};
static FuseChain &fuse_chain(int device) {
  static FuseChain chains[64];
  return chains[device & 63];
}
// REQUIREMENT (advisor, round 4): whoever owns a stream that stream_is_durable() answers true for -- a context's own stream,
// a scoring loop's -- must call this before destroying it (destroy_ctx and fdnn_server_free do): the chain keeps the raw
// handle of the stream its last launch went to and records its event there later.  A caller-created stream is never
// remembered (its record is made at once).
void fuse_chain_retire_stream(int device, hipStream_t s) {
  FuseChain &fc = fuse_chain(device);
  std::lock_guard<std::mutex> lk(fc.mu);
  if (fc.pending && fc.last_stream == s && fc.ev) {
    fc.recorded = hipEventRecord(fc.ev, s) == hipSuccess;
    fc.pending = false;
  }
}

// The output layer's choice for `count` frames of this context: what run_output launches.
static sel::LayerChoice choose_output(fdnn_ctx *c, int count, bool byte_mask, bool bit_mask, const Taps *taps, bool ctx_may_fuse) {
  fdnn_model *m = c->m;
  sel::LayerCall call{count};
  call.tap_acc = taps && taps->acc_out;
  call.tap_logit = taps && taps->logits;
  call.acc_probe = taps && taps->acc_probe;
  call.byte_mask = byte_mask;
  call.bit_mask = bit_mask;
  call.may_fuse = ctx_may_fuse && process_may_fuse(m->device) && model_may_fuse(m);
  return sel::choose_layer(layer_shape(m->hm.hdr.q[m->hm.hdr.n_q - 1], true), call, sel::tuning());
}

int run_output(fdnn_ctx *c, const OutputCall &oc, hipStream_t s) {
  const int first = oc.first, count = oc.count;
  const int8_t *d_masks = oc.d_masks;
  const uint64_t *d_bits = oc.d_bits;
  float *const d_out = oc.d_out, *const d_final = oc.d_final;
  const Taps *const taps = oc.taps;
  fdnn_model *m = c->m;
  const BlobHeader &h = m->hm.hdr;
  const QLayerDesc &d = h.q[h.n_q - 1];
  if (c->last < 0) return fail(FDNN_E_STATE, "output requested before the hidden layers were computed");
  if (first < 0 || count < 0 || first + count > c->n) return fail(FDNN_E_ARG, "frame range outside the context");
  if (count == 0) return FDNN_OK;
  // (One frame and decoder-sized blocks take the small-batch GEMM kernels as well: a row-by-row kernel that skips the
  // masked-out nodes as the reference does, dnn.cc:361-365, was measured against them -- DESIGN.md section 6 -- and lost
  // at every block size from 40 % active nodes up: the call is two launches of latency either way.)
  const sel::LayerChoice ch = choose_output(c, count, d_masks != nullptr, d_bits != nullptr, taps, !c->no_fuse);
  fdnn::QGemmParams g = prepare_qlayer(c, d, c->d_act[c->last] + size_t(first) * c->act_ld, count, ch);
  g.out = d_out;
  g.partial = c->d_partial;
  g.partial_ld = ch.partial_ld;
  if (d_bits && !d_masks) {  // bit-mask entry points
    if (!ch.mask_bits) {  // (the small-batch and the tap instances read bytes)
      if (!c->d_mask) return fail(FDNN_E_STATE, "this context has no byte-mask scratch for a small bit-mask batch");
      ProfScope ps(m, s, FDNN_PROF_OUTPUT);
      fdnn::launch_mask_unpack(d_bits, c->d_mask, count, d.rows, s);
      d_masks = c->d_mask;
      d_bits = nullptr;
    } else {
      d_masks = reinterpret_cast<const int8_t *>(d_bits);  // (non-null = the masked instances; they read mask_bits only)
    }
  }
  g.mask = d_masks;
  if (d_bits) {
    g.mask_bits = d_bits;
    g.mask_wpr = (d.rows + 63) / 64;
  } else if (d_masks && ch.mask_bits) {
    // large-batch production instances: the mask travels as bits (one pass over the caller's bytes at HBM speed)
    ProfScope ps(m, s, FDNN_PROF_OUTPUT);
    fdnn::launch_mask_pack(d_masks, c->d_mask_bits, count, d.rows, s);
    g.mask_bits = c->d_mask_bits;
    g.mask_wpr = (d.rows + 63) / 64;
    c->mask_bits_packed = true;  // (fdnn_ctx_lazy_output_batch needs the same bits for its compacted return: not twice)
  }
  g.tap_acc = taps ? taps->acc_out : nullptr;
  g.tap_logit = taps ? taps->logits : nullptr;
  g.acc_probe = taps ? taps->acc_probe : nullptr;
  g.probe_stride = taps ? std::max(1, taps->probe_stride) : 1;
  const bool fused = ch.fused, ppo = ch.form == sel::Form::ppo;
  if (fused && m->h_fuse_fault && __atomic_load_n(m->h_fuse_fault.p, __ATOMIC_RELAXED) != 0) {
    // (fusing although a launch of this model gave up before -- FDNN_FUSE_NORM=1 / fdnn_debug_set_fuse(1): a workgroup that
    // gave up may have left its exchange counters half counted; they are zeroed in stream order before every such launch)
    HIP_TRY(hipMemsetAsync(c->d_fuse_cnt, 0, sizeof(uint32_t) * c->d_fuse_cnt.count, s));
    HIP_TRY(hipMemsetAsync(c->d_fuse_flag, 0, sizeof(uint32_t) * c->d_fuse_flag.count, s));
  }
  if (fused) {
    g.final = d_final ? d_final : d_out;
    g.fuse_s = c->d_fuse_s;
    g.fuse_cnt = c->d_fuse_cnt;
    g.fuse_flag = c->d_fuse_flag;
    g.fuse_giveups = m->d_l0_stats ? m->d_l0_stats + 2 : nullptr;
    g.fuse_fault = m->h_fuse_fault.dev;
    g.fuse_stagger = sel::tuning().fuse_stagger;
  }
  {
    ProfScope ps(m, s, FDNN_PROF_OUTPUT);
    if (fused) {
      // The fused kernel's workgroups wait for their frame tile's other node tiles, which is safe while ONE such kernel is
      // being dispatched (in block order: the oldest unfinished frame tile always has all its workgroups resident) and a
      // latency cliff when several are -- nine partially dispatched frame tiles fill the 256 CUs and every one of them sits
      // in its bounded wait.  So the fused launches of a DEVICE form one chain, whatever stream, context, model or entry
      // point they come from: each waits for the previous one's event and records its own.  Other kernels overlap them
      // freely (they wait for nothing).  Two PROCESSES on one GPU cannot be chained: FDNN_FUSE_NORM=0.
      FuseChain &fc = fuse_chain(m->device);
      std::lock_guard<std::mutex> lk(fc.mu);
      if (!fc.ev) HIP_TRY(hipEventCreateWithFlags(&fc.ev, hipEventDisableTiming | hipEventDisableSystemFence));
      static const bool eager = FDNN_TUNE_ENV("FDNN_EAGER_EVENTS") != nullptr;
      if (fc.last_stream != s || !(fc.pending || fc.recorded)) {  // (same stream as the previous fused launch: in order already)
        if (fc.pending) {  // the deferred record: the tail of the previous launch's stream is behind that launch
          fc.pending = false;
          fc.recorded = false;
          HIP_TRY(hipEventRecord(fc.ev, fc.last_stream));
          fc.recorded = true;
        }
        if (fc.recorded) HIP_TRY(hipStreamWaitEvent(s, fc.ev, 0));
      }
      if (ppo) fdnn::launch_qppo_output(g, device_cus(m->device), s);
      else fdnn::launch_qgemm_output(g, ch.shape, s);
      fc.last_stream = s;
      if (stream_is_durable(c, s) && !eager) {
        fc.pending = true;
      } else {
        fc.pending = false;
        fc.recorded = false;
        HIP_TRY(hipEventRecord(fc.ev, s));
        fc.recorded = true;
      }
    } else if (g.small) {
      fdnn::launch_qgemm_small_output(g, s);
    } else {
      fdnn::launch_qgemm_output(g, ch.shape, s);
    }
  }
  if (!fused) {
    ProfScope ps(m, s, FDNN_PROF_NORMALIZE);
    fdnn::launch_normalize(d_out, d_final ? d_final : d_out, c->d_partial, count, g.partial_ld, d.rows, d.rows_pad / fdnn::kPartialNodes, s);
  }
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

// Device -> pageable host memory for large results (the 8000-float rows of a whole batch:
// 320 MB for 10 000 frames).  hipMemcpy into resident pageable memory runs at ~45 GB/s, but a
// result array that was just allocated (numpy's np.empty; a JVM float[] is already zeroed) is
// not resident: the copy then takes every first-touch page fault on one thread, 31 of the
// call's 34 ms.  So the destination is faulted in first, by a few host threads, one byte per
// page (it is about to be overwritten anyway) -- while the GPU is still computing, the
// kernels are already enqueued -- and the copy itself stays the runtime's.
// Measured, 10 000 frames: fresh array 33 -> 24.5 ms, resident array 7.1 ms either way.  (A
// hand-made pipeline over pinned bounce buffers with parallel host memcpy: 7.9 / 23.5 ms.)
// Synchronises the stream.
int copy_out(void *dst, const void *d_src, size_t bytes, hipStream_t s) {
  static const bool plain = FDNN_TUNE_ENV("FDNN_PLAIN_COPY_OUT") != nullptr;
  if (bytes >= (size_t(64) << 20) && !plain) {
    const unsigned hw = std::thread::hardware_concurrency();
    const int T = static_cast<int>(std::min<unsigned>(16, std::max<unsigned>(1, hw / 2)));
    const size_t page = 4096;
    const uintptr_t lo = (reinterpret_cast<uintptr_t>(dst) + page - 1) & ~(page - 1);
    const uintptr_t hi = (reinterpret_cast<uintptr_t>(dst) + bytes) & ~(page - 1);
    if (hi > lo) {
      const size_t pages = (hi - lo) / page;
      std::vector<std::thread> pool;
      for (int t = 0; t < T; ++t)
        pool.emplace_back([=] {
          const size_t b = pages * size_t(t) / size_t(T), e = pages * size_t(t + 1) / size_t(T);
          if (e == b) return;
          volatile char *q = reinterpret_cast<volatile char *>(lo);
          for (size_t i = b; i < e; ++i) q[i * page] = 0;  // (MADV_POPULATE_WRITE and MADV_HUGEPAGE were both slower)
        });
      for (auto &th : pool) th.join();
    }
  }
  HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FDNN_OK;
}

// pool: idle contexts with capacity >= n.  The hand-over event orders a reuse
// on another stream behind the previous user's kernels.
static int acquire_ctx(fdnn_model *m, int n, fdnn_ctx **out) {
  fdnn_ctx *c = nullptr;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    int best = -1;
    for (size_t i = 0; i < m->pool.size(); ++i)
      if (m->pool[i]->cap >= n && (best < 0 || m->pool[i]->cap < m->pool[size_t(best)]->cap)) best = int(i);
    if (best >= 0) {
      c = m->pool[size_t(best)];
      m->pool.erase(m->pool.begin() + best);
    }
  }
  if (!c) {
    int rc = make_ctx(m, n, &c);
    if (rc) return rc;
    c->pooled = true;
  }
  c->n = n;
  c->last = -1;
  *out = c;
  return FDNN_OK;
}

// Would run_hidden chain the int8 hidden layers of an n-frame batch of this model?  (The context-independent part of its
// decision: taps and a context whose chain faulted are the caller's business.)
bool hidden_layers_chain(const fdnn_model *m, int n) {
  const BlobHeader &h = m->hm.hdr;
  return sel::plan_hidden(h.n_q - 1, [&](int i) { return layer_shape(h.q[i], false); }, n, true, sel::tuning(), {device_cus(m->device)}).chain;
}

pass::Chunks frame_chunks(int n, const fdnn_model *m, bool assume_chained) {
  static const int kChunk = pass::chunk_size(sel::tuning().chunk_set, sel::tuning().chunk_frames);  // FDNN_CHUNK_FRAMES: measurement switch
  return pass::frame_chunks(n, kChunk, [&](int cnt) { return m ? hidden_layers_chain(m, cnt) : assume_chained; });
}

// A context's scratch is touched from two kinds of streams: the caller's (the *_device entry
// points) and the context's own (the host-pointer entry points; created non-blocking, so not even
// the NULL stream orders it).  Every entry point therefore starts by making its stream wait for
// the context's last enqueued work and ends by recording it: calculateUntilOutputDevice(stream)
// followed by calculateForOutputNodes() or hiddenActivations() reads finished activations
// without the caller synchronising anything.  On one stream both calls are no-ops for the device.
bool stream_is_durable(const fdnn_ctx *c, hipStream_t s) {
  return s == nullptr || s == c->stream || s == c->durable[0] || s == c->durable[1];
}
hipError_t ctx_enter(fdnn_ctx *c, hipStream_t s) {
  if (c->done_stream == s && (c->done_valid || c->done_pending)) return hipSuccess;  // same stream: already in order
  if (c->done_pending) {  // the deferred record: the tail of done_stream covers everything the context enqueued there
    c->done_pending = false;
    const hipError_t e = hipEventRecord(c->done, c->done_stream);
    c->done_valid = e == hipSuccess;
    if (e != hipSuccess) return e;
  }
  return hipStreamWaitEvent(s, c->done, 0);
}
void ctx_leave(fdnn_ctx *c, hipStream_t s) {
  static const bool eager = FDNN_TUNE_ENV("FDNN_EAGER_EVENTS") != nullptr;  // (measurements: every record made at once, as before round 4)
  c->done_stream = s;
  if (stream_is_durable(c, s) && !eager) {
    c->done_pending = true;
    c->done_valid = false;
    return;
  }
  c->done_pending = false;
  c->done_valid = hipEventRecord(c->done, s) == hipSuccess;
}
void ctx_wait_host(fdnn_ctx *c) {
  if (c->done_pending)
    hipStreamSynchronize(c->done_stream);
  else if (c->done_valid)
    hipEventSynchronize(c->done);
}

void release_ctx(fdnn_ctx *c) {
  fdnn_model *m = c->m;
  scratch_audit_event(c);  // (before another caller can draw it from the pool; nothing unless switched on)
  fdnn_ctx *victim = nullptr;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    m->pool.push_back(c);
    if (m->pool.size() > 8) {  // keep a handful of the largest contexts
      auto it = std::min_element(m->pool.begin(), m->pool.end(),
                                 [](const fdnn_ctx *a, const fdnn_ctx *b) { return a->cap < b->cap; });
      victim = *it;
      m->pool.erase(it);
    }
  }
  if (victim) {
    ctx_wait_host(victim);
    destroy_ctx(victim);
  }
}

// What leaves the device after a dense pass, synchronising s: the whole rows, or the selection of them (fdnn_topk.hip)
// into the context's own pair buffer -- [n][k] nodes, then [n][k] values -- and its two halves to the caller's arrays, or
// their class sums (fdnn_pool.hip) into the context's own [n][C] buffer and from there to the caller's in one transfer.
static int dense_leave(fdnn_ctx *c, const DenseTo &to, hipStream_t s) {
  const size_t n = size_t(c->n), O = size_t(c->m->hm.hdr.out_dim);
  if (to.pool) {
    const size_t nc = n * size_t(to.pool->n_classes);
    HIP_TRY(c->d_pool.reserve(nc));
    fdnn::launch_pool(c->d_out, c->n, int(O), to.pool->d_class_ptr(), to.pool->d_member(), to.pool->n_classes, c->d_pool, s);
    HIP_TRY(hipMemcpyAsync(to.pooled, c->d_pool, sizeof(float) * nc, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FDNN_OK;
  }
  if (to.loglik) {  // the rows as decoder scores (fdnn_loglik.hip) into the context's own [n][O] buffer, then one transfer
    const size_t bytes = n * O * fdnn::loglik::elem_bytes(to.loglik->type);
    HIP_TRY(c->d_loglik.reserve((bytes + 3) / 4));
    fdnn::launch_loglik_rows(c->d_out, c->n, int(O), to.loglik->d_log_prior, to.loglik->floor, to.loglik->type, c->d_loglik.p, s);
    HIP_TRY(hipMemcpyAsync(to.scores, c->d_loglik.p, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FDNN_OK;
  }
  if (to.k == 0) return copy_out(to.out, c->d_out, sizeof(float) * n * O, s);
  const size_t nk = n * size_t(to.k);
  HIP_TRY(c->d_topk.reserve(2 * nk));
  fdnn::launch_topk(c->d_out, c->n, int(O), to.k, c->d_topk, reinterpret_cast<float *>(c->d_topk.p + nk), s);
  HIP_TRY(hipMemcpyAsync(to.nodes, c->d_topk, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(to.probs, c->d_topk.p + nk, sizeof(float) * nk, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FDNN_OK;
}

// The dense pass over the context's frames (c->n of them) to a host caller, synchronising s: the hidden layers over c->d_x
// (hidden = false: they have run, the context holds their activations), the output layer, then what leaves the device.
int dense_pass(fdnn_ctx *c, const DenseTo &to, hipStream_t s, bool hidden) {
  fdnn_model *m = c->m;
  const unsigned long long unwritten_before = m->h_fuse_fault ? __atomic_load_n(m->h_fuse_fault.p, __ATOMIC_RELAXED) >> 32 : 0ull;
  const auto pass = [&](bool with_hidden) {
    int rc = with_hidden ? run_hidden(c, c->d_x, s, nullptr) : FDNN_OK;
    if (!rc) rc = run_output(c, {.count = c->n, .d_out = c->d_out}, s);
    if (!rc) rc = dense_leave(c, to, s);
    if (rc) hipStreamSynchronize(s);
    return rc;
  };
  int rc = pass(hidden);
  // dense_leave has synchronised: did a fused soft-max workgroup of THIS pass sit out its bounded wait?  fdnn_gemm.hip's
  // tiles finish such a frame tile after the fact, fdnn_ppo.hip's leave the half's rows unwritten (and say so through the
  // same word): the output layer runs again -- unfused now, model_may_fuse has seen the word -- over the activations that
  // are still in the context, before anything of it is handed out.  (The word's upper half counts such halves.  Callers of
  // the *_device entry points observe fdnn_model_fuse_giveups after their own synchronisation: INTEGRATION.md.)
  if (!rc && m->h_fuse_fault && (__atomic_load_n(m->h_fuse_fault.p, __ATOMIC_RELAXED) >> 32) != unwritten_before) {
    const bool saved = c->no_fuse;
    c->no_fuse = true;  // (whatever FDNN_FUSE_NORM says)
    rc = pass(false);
    c->no_fuse = saved;
  }
  // dense_leave has synchronised: did this pass's chained launch run into its wait bound?  Then what it computed on may not have
  // been written -- run the pass again, layer by layer (run_hidden sees the flag, re-zeroes the counters, stops chaining)
  if (!rc && hidden && c->h_chain_fault && __atomic_load_n(c->h_chain_fault.p, __ATOMIC_RELAXED) != 0 && !c->chain_broken) rc = pass(true);
  return rc;
}

int dense_pass_to_host(fdnn_ctx *c, float *out, hipStream_t s) { return dense_pass(c, {.out = out}, s, true); }

// ---------------------------------------------------------------- raw feature frames
int splice_check(const SpliceRef &spec, int raw_dim) {
  if (!spec) return fail(FDNN_E_STATE, "no splice spec set (fdnn_model_set_splice)");
  if (raw_dim >= 0 && raw_dim != spec->raw_dim)
    return fail(FDNN_E_ARG, "raw frame width " + std::to_string(raw_dim) + " is not the splice spec's " + std::to_string(spec->raw_dim));
  return FDNN_OK;
}

int ctx_raw_reserve(fdnn_ctx *c, size_t frames, int raw_dim) {
  const fdnn_model *m = c->m;
  if (!c->d_x) HIP_TRY(c->d_x.reserve(size_t(c->cap) * m->hm.hdr.in_dim));
  const size_t D = size_t(raw_dim);  // (a pooled context's last raw call may have had another width)
  // (a buffer that is too small is freed first: the context's earlier work is ordered before, callers hold it)
  if (c->d_raw.count < frames * D) HIP_TRY(c->d_raw.reserve(std::max(frames, size_t(c->cap)) * D));
  return FDNN_OK;
}

void splice_rows(const SpliceSpec &spec, int input_dim, const float *raw, int raw_frames, const std::vector<SpliceSeg> &segs,
                 int row0, int rows, float *d_x, hipStream_t s) {
  fdnn::SpliceArgs a{};
  a.count = int(spec.offsets.size());
  a.raw_dim = spec.raw_dim;
  a.input_dim = input_dim;
  std::copy(spec.offsets.begin(), spec.offsets.end(), a.offsets);
  // the segment holding row0, then launch by launch up to kSpliceMaxSegs segments each
  size_t g = size_t(std::upper_bound(segs.begin(), segs.end(), row0, [](int r, const SpliceSeg &sg) { return r < sg.row; }) - segs.begin());
  g = g ? g - 1 : 0;
  const int end = row0 + rows;
  int r = row0;
  while (r < end && g < segs.size()) {
    a.n_segs = 0;
    for (size_t k = g; k < segs.size() && a.n_segs < fdnn::kSpliceMaxSegs && (k == g || segs[k].row < end); ++k) {
      a.seg_row[a.n_segs] = segs[k].row;
      a.seg_center[a.n_segs] = segs[k].center;
      a.seg_lo[a.n_segs] = segs[k].lo;
      a.seg_hi[a.n_segs] = segs[k].hi;
      ++a.n_segs;
    }
    const size_t next = g + size_t(a.n_segs);
    const int stop = next < segs.size() ? std::min(end, segs[next].row) : end;
    fdnn::launch_splice(raw, raw_frames, d_x + size_t(r - row0) * a.input_dim, r, stop - r, a, s);
    r = stop;
    g = next;
  }
}

void splice_rows_table(const SpliceSpec &spec, int input_dim, const float *raw, int raw_frames, const int32_t *d_segs,
                       const int32_t *d_row_seg, int n_segs, int rows, float *d_x, hipStream_t s) {
  fdnn::SpliceOffsets a{};
  a.count = int(spec.offsets.size());
  a.raw_dim = spec.raw_dim;
  a.input_dim = input_dim;
  std::copy(spec.offsets.begin(), spec.offsets.end(), a.offsets);
  fdnn::launch_splice_table(raw, raw_frames, d_x, rows, d_segs, d_row_seg, n_segs, a, s);
}

// Lazy results to a host caller.  Every inactive node of a row reads the same 1 / total (dnn.cc:366-369, :389), so what
// crosses PCIe is the active nodes' probabilities and that one value per frame (lazy_compact_kernel); the rows are
// rebuilt on the host inside the caller's array: the compacted block lands in its tail, and the rows are expanded front to
// back (row f's place never reaches the compacted rows of later frames; its own is copied aside first).  d_bits: the
// masks of the `count` frames on the device; bits: the same on the host.  With mostly active masks (> 3/4) the plain copy
// is used.  Synchronises the stream.
int lazy_copy_out(fdnn_ctx *c, int count, const uint64_t *d_bits, const uint64_t *bits, float *out, hipStream_t s) {
  const size_t O = size_t(c->m->hm.hdr.out_dim), wpr = (O + 63) / 64;
  static const bool no_compact = FDNN_TUNE_ENV("FDNN_LAZY_NO_COMPACT") != nullptr;
  size_t most = 0;
  const uint64_t tail_mask = (O & 63) ? ((uint64_t(1) << (O & 63)) - 1) : ~uint64_t(0);
  for (int f = 0; f < count; ++f) {
    size_t k = 0;
    const uint64_t *row = bits + size_t(f) * wpr;
    for (size_t w = 0; w + 1 < wpr; ++w) k += size_t(__builtin_popcountll(row[w]));
    k += size_t(__builtin_popcountll(row[wpr - 1] & tail_mask));
    most = std::max(most, k);
  }
  const size_t stride = most + 1;
  if (no_compact || stride * 4 > O * 3) return copy_out(out, c->d_out, sizeof(float) * size_t(count) * O, s);
  HIP_TRY(c->d_comp.reserve(size_t(count) * stride));
  fdnn::launch_lazy_compact(c->d_out, d_bits, c->d_comp, count, int(O), int(stride), s);
  float *land = out + size_t(count) * O - size_t(count) * stride;
  HIP_TRY(hipMemcpyAsync(land, c->d_comp, sizeof(float) * size_t(count) * stride, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  fdnn::lazy_expand_rows(out, count, O, stride, bits);
  return FDNN_OK;
}

// ---------------------------------------------------------------- the scoring pass of every pooled entry point
int check_input_width(const fdnn_model *m, int dim) {
  if (dim == m->hm.hdr.in_dim) return FDNN_OK;
  return fail(FDNN_E_ARG, "input vector size " + std::to_string(dim) + " must be equal with network input size " + std::to_string(m->hm.hdr.in_dim));
}

int check_pool(const fdnn_model *m, const fdnn_pool *pool) {
  if (!pool) return fail(FDNN_E_ARG, "null pool");
  if (m->group) return fail(FDNN_E_ARG, "pool calls do not run on a model that leads a device group");
  if (pool->width != m->hm.hdr.out_dim)
    return fail(FDNN_E_ARG, "pool width " + std::to_string(pool->width) + " is not the network's output size " + std::to_string(m->hm.hdr.out_dim));
  if (pool->device != m->device) return fail(FDNN_E_ARG, "the pool was created on another device than the model's");
  return FDNN_OK;
}

int check_loglik(const fdnn_model *m, const fdnn_loglik *ll) {
  if (!ll) return fail(FDNN_E_ARG, "null score handle");
  if (m->group) return fail(FDNN_E_ARG, "loglik calls do not run on a model that leads a device group");
  if (ll->width != m->hm.hdr.out_dim)
    return fail(FDNN_E_ARG, "score handle width " + std::to_string(ll->width) + " is not the network's output size " + std::to_string(m->hm.hdr.out_dim));
  if (ll->device != m->device) return fail(FDNN_E_ARG, "the score handle was created on another device than the model's");
  return FDNN_OK;
}

int check_frames_aligned(const float *d_x) {
  if ((reinterpret_cast<uintptr_t>(d_x) & 15) == 0) return FDNN_OK;
  return fail(FDNN_E_ARG, "device frames must start on a 16-byte boundary (include/fdnn.h, Device buffers)");
}

// What each sink does with a chunk whose rows are in place (d_x: on the device, the caller's or the context's frame buffer).
static int to_device_rows(fdnn_ctx *c, const float *d_x, int cnt, const int8_t *d_masks, const uint64_t *d_bits, float *d_out, hipStream_t s) {
  int rc = run_hidden(c, d_x, s, nullptr);
  if (!rc) rc = run_output(c, {.count = cnt, .d_masks = d_masks, .d_bits = d_bits, .d_out = d_out}, s);
  return rc;
}
static int to_host_behind_bits(fdnn_ctx *c, const pass::ChunkView &v, hipStream_t s) {
  int rc = to_device_rows(c, c->d_x, v.cnt, nullptr, c->d_mask_bits, c->d_out, s);
  if (!rc) rc = lazy_copy_out(c, v.cnt, c->d_mask_bits, v.bits, v.rows, s);
  if (rc) hipStreamSynchronize(s);
  return rc;
}
// device top-k: the rows stay in the context, the selection goes to the caller's buffers
static int to_device_topk(fdnn_ctx *c, const float *d_x, const pass::ChunkView &v, int k, hipStream_t s) {
  int rc = to_device_rows(c, d_x, v.cnt, nullptr, nullptr, c->d_out, s);
  if (!rc) fdnn::launch_topk(c->d_out, v.cnt, c->m->hm.hdr.out_dim, k, v.topk_nodes, v.topk_probs, s);
  return rc;
}
// device pool: the rows stay in the context, their class sums go to the caller's buffer
static int to_device_pool(fdnn_ctx *c, const float *d_x, const pass::ChunkView &v, const fdnn_pool *pool, hipStream_t s) {
  int rc = to_device_rows(c, d_x, v.cnt, nullptr, nullptr, c->d_out, s);
  if (!rc) fdnn::launch_pool(c->d_out, v.cnt, c->m->hm.hdr.out_dim, pool->d_class_ptr(), pool->d_member(), pool->n_classes, v.pooled, s);
  return rc;
}
// device loglik: the rows stay in the context, their scores go to the caller's buffer
static int to_device_loglik(fdnn_ctx *c, const float *d_x, const pass::ChunkView &v, const fdnn_loglik *ll, hipStream_t s) {
  int rc = to_device_rows(c, d_x, v.cnt, nullptr, nullptr, c->d_out, s);
  if (!rc) fdnn::launch_loglik_rows(c->d_out, v.cnt, c->m->hm.hdr.out_dim, ll->d_log_prior, ll->floor, ll->type, v.scores, s);
  return rc;
}
// the chunk's entries through the host form, which synchronises (a sets chunk without a segment scores nothing)
static int to_host_entries(fdnn_ctx *c, const pass::Sink &to, const pass::ChunkView &v, hipStream_t s) {
  int rc = run_hidden(c, c->d_x, s, nullptr);
  HostEntries he;
  he.count = v.cnt, he.nodes = v.nodes, he.n_nodes = v.n_nodes, he.probs = v.probs, he.inactive = v.inactive;
  if (to.kind == pass::Sink::host_lists) he.row_ptr = v.row_ptr.data();
  else if (to.kind == pass::Sink::host_set) he.len = to.len;
  else he.segs = &v.segs;
  if (!rc && (to.kind != pass::Sink::host_sets || !v.segs.empty())) rc = entries_to_host(c, he, s);
  if (rc) hipStreamSynchronize(s);
  return rc;
}
static int to_device_sets(fdnn_ctx *c, const float *d_x, const pass::ChunkView &v, hipStream_t s) {
  int rc = run_hidden(c, d_x, s, nullptr);
  SetsCall sc;
  sc.segs = &v.segs, sc.d_nodes = v.nodes, sc.d_probs = v.probs, sc.d_inactive = v.inactive;
  if (!rc) rc = run_sets(c, sc, s);
  return rc;
}

// align: the chunk's slice of the sets into the context's align buffers (align_stage has put the nodes there); the blocks of
// a call's slices follow each other in d_al_probs as they do in a host caller's probs
static int to_align_sets(fdnn_ctx *c, const pass::ChunkView &v, hipStream_t s) {
  int rc = run_hidden(c, c->d_x, s, nullptr);
  SetsCall sc;
  sc.segs = &v.segs, sc.d_nodes = c->d_al_int, sc.d_inactive = c->d_al_inact;
  sc.d_probs = c->d_al_probs.p + (v.segs.empty() ? 0 : size_t(v.segs[0].src_off));
  if (!rc && !v.segs.empty()) rc = run_sets(c, sc, s);
  if (rc) hipStreamSynchronize(s);
  return rc;
}

int run_chunks(fdnn_ctx *c, hipStream_t s, const pass::Chunks &chunks, const pass::Pass &p) {
  using pass::Rows;
  using pass::Sink;
  const BlobHeader &h = c->m->hm.hdr;
  const pass::Dims dims{size_t(h.in_dim), size_t(h.out_dim), (size_t(h.out_dim) + 63) / 64};
  const pass::Raw &raw = p.rows.raw;
  for (const auto &ch : chunks) {  // frames are independent: a chunk is a batch of its own
    const pass::ChunkView v = pass::chunk_view(p, dims, ch.first, ch.second);
    c->n = v.cnt;
    hipError_t e = hipSuccess;
    if (raw.spec) splice_rows(*raw.spec, h.in_dim, p.rows.kind == Rows::raw_host ? c->d_raw.p : raw.frames, raw.n_frames, *raw.segs, v.splice_row, v.cnt, c->d_x, s);
    if (p.rows.kind == Rows::host) e = hipMemcpyAsync(c->d_x, v.x, sizeof(float) * size_t(v.cnt) * dims.D, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && p.mask.kind == pass::Mask::host_bits)
      e = hipMemcpyAsync(c->d_mask_bits, v.bits, sizeof(uint64_t) * size_t(v.cnt) * dims.wpr, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail(FDNN_E_DEVICE, std::string(p.who) + ": " + hipGetErrorString(e));
    const float *d_x = p.rows.kind == Rows::device ? v.x : c->d_x.p;
    int rc = FDNN_OK;
    switch (p.sink.kind) {
      case Sink::device_rows: rc = to_device_rows(c, d_x, v.cnt, v.bytes, v.bits, v.rows, s); break;
      case Sink::host_dense: rc = dense_pass_to_host(c, v.rows, s); break;
      case Sink::host_behind_bits: rc = to_host_behind_bits(c, v, s); break;
      case Sink::host_topk: rc = dense_pass(c, {.k = p.sink.k, .nodes = v.topk_nodes, .probs = v.topk_probs}, s, true); break;  // n x k x 8 bytes cross PCIe
      case Sink::device_topk: rc = to_device_topk(c, d_x, v, p.sink.k, s); break;
      case Sink::host_lists:
      case Sink::host_set:
      case Sink::host_sets: rc = to_host_entries(c, p.sink, v, s); break;
      case Sink::device_sets: rc = to_device_sets(c, d_x, v, s); break;
      case Sink::host_pool: rc = dense_pass(c, {.pool = p.sink.pool, .pooled = v.pooled}, s, true); break;  // n x C x 4 bytes cross PCIe
      case Sink::device_pool: rc = to_device_pool(c, d_x, v, p.sink.pool, s); break;
      case Sink::host_loglik: rc = dense_pass(c, {.loglik = p.sink.loglik, .scores = v.scores}, s, true); break;  // n x O x 4 or 2 bytes cross PCIe
      case Sink::device_loglik: rc = to_device_loglik(c, d_x, v, p.sink.loglik, s); break;
      case Sink::align_sets: rc = to_align_sets(c, v, s); break;
    }
    if (rc) return rc;
  }
  return FDNN_OK;
}

int score_chunks(fdnn_model *m, const pass::Chunks &chunks, const pass::Pass &p, hipStream_t callers, const CtxStep &before, const CtxStep &after) {
  DeviceGuard g(m->device);
  int cap = 0;  // the scratch only has to hold the largest chunk
  for (const auto &ch : chunks) cap = std::max(cap, ch.second);
  fdnn_ctx *c = nullptr;
  int rc = acquire_ctx(m, cap, &c);
  if (rc) return rc;
  hipStream_t s = pass::on_callers_stream(p.sink.kind) ? callers : c->stream;
  CtxUse use;  // (also on the error paths: the context goes back to the pool)
  hipError_t e = use.enter(c, s);
  const pass::Raw &raw = p.rows.raw;
  if (e == hipSuccess && p.rows.kind == pass::Rows::raw_host) {  // host raw frames travel once; every chunk splices its rows from them
    rc = ctx_raw_reserve(c, size_t(raw.n_frames), raw.spec->raw_dim);
    if (rc) return rc;
    e = hipMemcpyAsync(c->d_raw, raw.frames, sizeof(float) * size_t(raw.n_frames) * size_t(raw.spec->raw_dim), hipMemcpyHostToDevice, s);
  }
  if (e != hipSuccess) return fail(FDNN_E_DEVICE, std::string(p.who) + ": " + hipGetErrorString(e));
  if (before)
    if ((rc = before(c, s))) return rc;
  rc = run_chunks(c, s, chunks, p);
  if (!rc && after) rc = after(c, s);
  return rc;
}

// ---------------------------------------------------------------- forced alignment (fdnn_align.hip)
int align_prepare(AlignJob *j, int output_dim, int ctx_rows) {
  align::Why why;
  const int bad = align::check(j->seg_rows, j->state_ptr, j->states, j->self_lp, j->next_lp, j->n_segs, output_dim, ctx_rows, true, &why);
  if (bad) return fail(FDNN_E_ARG, "align, segment " + std::to_string(-bad - 1) + ": " + align::why_text(why));
  const int n = j->n_segs;
  j->sets = align::build_sets(j->state_ptr, j->states, n);
  j->seg_T.resize(size_t(n)), j->row_ld.resize(size_t(n)), j->row_off.resize(size_t(n));
  j->nnz = 0;
  for (int s = 0; s < n; ++s) {
    j->seg_T[size_t(s)] = j->seg_rows[s + 1] - j->seg_rows[s];
    j->row_ld[size_t(s)] = j->sets.set_ptr[size_t(s) + 1] - j->sets.set_ptr[size_t(s)];
    j->row_off[size_t(s)] = j->nnz;
    j->nnz += static_cast<long long>(j->seg_T[size_t(s)]) * j->row_ld[size_t(s)];
    if (j->nnz > INT32_MAX) return fail(FDNN_E_ARG, "align, segment " + std::to_string(s) + ": the sum of rows x distinct nodes over the segments must fit an int32");
  }
  j->rows = n ? j->seg_rows[n] - j->seg_rows[0] : 0;
  j->plan = align::plan(j->seg_T.data(), j->row_off.data(), j->row_ld.data(), j->state_ptr, n, align_kernel_mode());
  if (j->plan.scratch_words * 4 > align::kMaxScratchBytes)
    return fail(FDNN_E_ARG, "align: the back-pointer words of the call (" + std::to_string(j->plan.scratch_words * 4) + " bytes) are above " + std::to_string(align::kMaxScratchBytes));
  return FDNN_OK;
}

int align_stage(fdnn_ctx *c, const AlignJob &j, hipStream_t s) {
  const size_t n_nodes = j.sets.nodes.size(), n_states = j.sets.col.size();
  HIP_TRY(c->d_al_int.reserve(n_nodes + 2 * n_states));
  HIP_TRY(c->d_al_lp.reserve(2 * n_states));
  HIP_TRY(c->d_al_probs.reserve(std::max<size_t>(size_t(j.nnz), 1)));
  HIP_TRY(c->d_al_inact.reserve(std::max<size_t>(size_t(j.rows), 1)));
  HIP_TRY(c->d_al_bp.reserve(std::max<size_t>(size_t(j.plan.scratch_words), 2)));
  HIP_TRY(c->d_al_res.reserve(size_t(j.rows) + size_t(j.n_segs)));
  HIP_TRY(hipMemcpyAsync(c->d_al_int, j.sets.nodes.data(), sizeof(int32_t) * n_nodes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_al_int.p + n_nodes, j.sets.col.data(), sizeof(int32_t) * n_states, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_al_int.p + n_nodes + n_states, j.states, sizeof(int32_t) * n_states, hipMemcpyHostToDevice, s));
  if (j.self_lp) HIP_TRY(hipMemcpyAsync(c->d_al_lp, j.self_lp, sizeof(float) * n_states, hipMemcpyHostToDevice, s));
  if (j.next_lp) HIP_TRY(hipMemcpyAsync(c->d_al_lp.p + n_states, j.next_lp, sizeof(float) * n_states, hipMemcpyHostToDevice, s));
  return FDNN_OK;
}

int align_finish(fdnn_ctx *c, const AlignJob &j, int32_t *path, float *total, bool host, hipStream_t s) {
  const size_t n_nodes = j.sets.nodes.size(), n_states = j.sets.col.size(), rows = size_t(j.rows), n = size_t(j.n_segs);
  AlignArgs a;
  a.d_rows = c->d_al_probs, a.d_col = c->d_al_int.p + n_nodes, a.d_state_node = c->d_al_int.p + n_nodes + n_states;
  a.d_log_prior = j.ll->d_log_prior, a.width = j.ll->width, a.floor = j.ll->floor, a.type = j.ll->type;
  a.d_self_lp = j.self_lp ? c->d_al_lp.p : nullptr, a.d_next_lp = j.next_lp ? c->d_al_lp.p + n_states : nullptr;
  a.d_scratch = c->d_al_bp, a.d_path = c->d_al_res, a.d_total = reinterpret_cast<float *>(c->d_al_res.p + rows);
  launch_align(j.plan, a, s);
  HIP_TRY(hipGetLastError());
  if (!host) {
    HIP_TRY(hipMemcpyAsync(path, c->d_al_res, sizeof(int32_t) * rows, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(total, c->d_al_res.p + rows, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    return FDNN_OK;
  }
  std::vector<int32_t> land(rows + n);  // one transfer: 4 bytes a frame and 4 a segment
  HIP_TRY(hipMemcpyAsync(land.data(), c->d_al_res, sizeof(int32_t) * (rows + n), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::memcpy(path, land.data(), sizeof(int32_t) * rows);
  std::memcpy(total, land.data() + rows, sizeof(float) * n);
  return FDNN_OK;
}

// ---------------------------------------------------------------- alignment graphs (fdnn_align_graph.hip)
int align_graph_prepare(AlignGraphJob *j, int output_dim, int ctx_rows) {
  align_graph::Why why;
  const int bad = align_graph::check(j->t, output_dim, ctx_rows, &why);
  if (bad) return fail(FDNN_E_ARG, "align graph, segment " + std::to_string(-bad - 1) + ": " + align_graph::why_text(why));
  const int n = j->t.n_segs;
  j->sets = align::build_sets(j->t.state_ptr, j->t.states, n);
  j->seg_T.resize(size_t(n)), j->row_ld.resize(size_t(n)), j->row_off.resize(size_t(n));
  j->nnz = 0;
  for (int s = 0; s < n; ++s) {
    j->seg_T[size_t(s)] = j->t.seg_rows[s + 1] - j->t.seg_rows[s];
    j->row_ld[size_t(s)] = j->sets.set_ptr[size_t(s) + 1] - j->sets.set_ptr[size_t(s)];
    j->row_off[size_t(s)] = j->nnz;
    j->nnz += static_cast<long long>(j->seg_T[size_t(s)]) * j->row_ld[size_t(s)];
    if (j->nnz > INT32_MAX)
      return fail(FDNN_E_ARG, "align graph, segment " + std::to_string(s) + ": the sum of rows x distinct nodes over the segments must fit an int32");
  }
  j->rows = n ? j->t.seg_rows[n] - j->t.seg_rows[0] : 0;
  j->plan = align_graph::plan(j->seg_T.data(), j->row_off.data(), j->row_ld.data(), j->t.state_ptr, j->t.arc_ptr, n, align_graph_kernel_mode());
  if (j->plan.scratch_words * 4 > align_graph::kMaxScratchBytes)
    return fail(FDNN_E_ARG, "align graph: the back-pointers of the call (" + std::to_string(j->plan.scratch_words * 4) + " bytes) are above " +
                                std::to_string(align_graph::kMaxScratchBytes));
  return FDNN_OK;
}

int align_graph_stage(fdnn_ctx *c, const AlignGraphJob &j, hipStream_t s) {
  const size_t n_nodes = j.sets.nodes.size(), n_states = j.sets.col.size(), n_arcs = size_t(j.t.arc_ptr[n_states]);
  HIP_TRY(c->d_al_int.reserve(n_nodes + 2 * n_states));
  HIP_TRY(c->d_ag_int.reserve(n_states + 1 + std::max<size_t>(n_arcs, 1)));
  HIP_TRY(c->d_ag_lp.reserve(std::max<size_t>(n_arcs, 1) + 2 * n_states));
  HIP_TRY(c->d_al_probs.reserve(std::max<size_t>(size_t(j.nnz), 1)));
  HIP_TRY(c->d_al_inact.reserve(std::max<size_t>(size_t(j.rows), 1)));
  HIP_TRY(c->d_al_bp.reserve(std::max<size_t>(size_t(j.plan.scratch_words), 2)));
  HIP_TRY(c->d_al_res.reserve(size_t(j.rows) + size_t(j.t.n_segs)));
  HIP_TRY(hipMemcpyAsync(c->d_al_int, j.sets.nodes.data(), sizeof(int32_t) * n_nodes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_al_int.p + n_nodes, j.sets.col.data(), sizeof(int32_t) * n_states, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_al_int.p + n_nodes + n_states, j.t.states, sizeof(int32_t) * n_states, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_ag_int, j.t.arc_ptr, sizeof(int32_t) * (n_states + 1), hipMemcpyHostToDevice, s));
  if (n_arcs) {
    HIP_TRY(hipMemcpyAsync(c->d_ag_int.p + n_states + 1, j.t.arc_src, sizeof(int32_t) * n_arcs, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_ag_lp, j.t.arc_lp, sizeof(float) * n_arcs, hipMemcpyHostToDevice, s));
  }
  float *tail = c->d_ag_lp.p + std::max<size_t>(n_arcs, 1);
  if (j.t.start_lp) HIP_TRY(hipMemcpyAsync(tail, j.t.start_lp, sizeof(float) * n_states, hipMemcpyHostToDevice, s));
  if (j.t.final_lp) HIP_TRY(hipMemcpyAsync(tail + n_states, j.t.final_lp, sizeof(float) * n_states, hipMemcpyHostToDevice, s));
  return FDNN_OK;
}

int align_graph_finish(fdnn_ctx *c, const AlignGraphJob &j, int32_t *path, float *total, bool host, hipStream_t s) {
  const size_t n_nodes = j.sets.nodes.size(), n_states = j.sets.col.size(), rows = size_t(j.rows), n = size_t(j.t.n_segs);
  const size_t n_arcs = size_t(j.t.arc_ptr[n_states]);
  float *tail = c->d_ag_lp.p + std::max<size_t>(n_arcs, 1);
  AlignGraphArgs a;
  a.d_rows = c->d_al_probs, a.d_col = c->d_al_int.p + n_nodes, a.d_state_node = c->d_al_int.p + n_nodes + n_states;
  a.d_log_prior = j.ll->d_log_prior, a.width = j.ll->width, a.floor = j.ll->floor, a.type = j.ll->type;
  a.d_arc_ptr = c->d_ag_int, a.d_arc_src = c->d_ag_int.p + n_states + 1, a.d_arc_lp = c->d_ag_lp;
  a.d_start_lp = j.t.start_lp ? tail : nullptr, a.d_final_lp = j.t.final_lp ? tail + n_states : nullptr;
  a.d_scratch = c->d_al_bp, a.d_path = c->d_al_res, a.d_total = reinterpret_cast<float *>(c->d_al_res.p + rows);
  launch_align_graph(j.plan, a, s);
  HIP_TRY(hipGetLastError());
  if (!host) {
    HIP_TRY(hipMemcpyAsync(path, c->d_al_res, sizeof(int32_t) * rows, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(total, c->d_al_res.p + rows, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    return FDNN_OK;
  }
  std::vector<int32_t> land(rows + n);  // one transfer: 4 bytes a frame and 4 a segment
  HIP_TRY(hipMemcpyAsync(land.data(), c->d_al_res, sizeof(int32_t) * (rows + n), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::memcpy(path, land.data(), sizeof(int32_t) * rows);
  std::memcpy(total, land.data() + rows, sizeof(float) * n);
  return FDNN_OK;
}

// ---------------------------------------------------------------- alignment graphs, summed (fdnn_fb.hip)
int fb_prepare(FbJob *j, int output_dim, int ctx_rows) {
  align_graph::Why why;
  const int bad = align_graph::check(j->t, output_dim, ctx_rows, &why);
  if (bad) return fail(FDNN_E_ARG, "forward-backward, segment " + std::to_string(-bad - 1) + ": " + align_graph::why_text(why));
  const int n = j->t.n_segs;
  j->sets = align::build_sets(j->t.state_ptr, j->t.states, n);
  j->seg_T.resize(size_t(n)), j->row_ld.resize(size_t(n)), j->row_off.resize(size_t(n));
  j->nnz = 0;
  for (int s = 0; s < n; ++s) {
    j->seg_T[size_t(s)] = j->t.seg_rows[s + 1] - j->t.seg_rows[s];
    j->row_ld[size_t(s)] = j->sets.set_ptr[size_t(s) + 1] - j->sets.set_ptr[size_t(s)];
    j->row_off[size_t(s)] = j->nnz;
    j->nnz += static_cast<long long>(j->seg_T[size_t(s)]) * j->row_ld[size_t(s)];
    if (j->nnz > INT32_MAX)
      return fail(FDNN_E_ARG, "forward-backward, segment " + std::to_string(s) + ": the sum of rows x distinct nodes over the segments must fit an int32");
  }
  j->rows = n ? j->t.seg_rows[n] - j->t.seg_rows[0] : 0;
  if (j->want_gamma && n) {
    const size_t n_states = size_t(j->t.state_ptr[n]), n_arcs = size_t(j->t.arc_ptr[n_states]);
    j->t_ptr.assign(n_states + 1, 0), j->t_src.assign(n_arcs, 0), j->t_lp.assign(n_arcs, 0.0f);
    if (fb::transpose(j->t.state_ptr, n, j->t.arc_ptr, j->t.arc_src, j->t.arc_lp, j->t_ptr.data(), j->t_src.data(), j->t_lp.data()))
      return fail(FDNN_E_ARG, "forward-backward: malformed arc tables");  // (the validator has passed: not reached)
  }
  j->plan = fb::plan(j->seg_T.data(), j->row_off.data(), j->row_ld.data(), j->t.state_ptr, j->t.arc_ptr, n, j->want_gamma, fb_kernel_mode());
  if (j->plan.scratch_words * 4 > fb::kMaxScratchBytes)
    return fail(FDNN_E_ARG, "forward-backward: the lattice of the call (" + std::to_string(j->plan.scratch_words * 4) + " bytes) is above " +
                                std::to_string(fb::kMaxScratchBytes));
  return FDNN_OK;
}

int fb_stage(fdnn_ctx *c, const FbJob &j, hipStream_t s) {
  const size_t n_nodes = j.sets.nodes.size(), n_states = j.sets.col.size(), n_arcs = size_t(j.t.arc_ptr[n_states]), n = size_t(j.t.n_segs);
  const size_t arcs1 = std::max<size_t>(n_arcs, 1);
  HIP_TRY(c->d_al_int.reserve(n_nodes + 2 * n_states));
  HIP_TRY(c->d_ag_int.reserve(n_states + 1 + arcs1));
  HIP_TRY(c->d_ag_lp.reserve(arcs1 + 2 * n_states));
  HIP_TRY(c->d_al_probs.reserve(std::max<size_t>(size_t(j.nnz), 1)));
  HIP_TRY(c->d_al_inact.reserve(std::max<size_t>(size_t(j.rows), 1)));
  HIP_TRY(c->d_al_bp.reserve(std::max<size_t>(size_t(j.plan.scratch_words), 2)));
  HIP_TRY(c->d_fb_res.reserve(n + (j.want_gamma ? size_t(j.plan.gamma_words) : 0)));
  HIP_TRY(hipMemcpyAsync(c->d_al_int, j.sets.nodes.data(), sizeof(int32_t) * n_nodes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_al_int.p + n_nodes, j.sets.col.data(), sizeof(int32_t) * n_states, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_al_int.p + n_nodes + n_states, j.t.states, sizeof(int32_t) * n_states, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_ag_int, j.t.arc_ptr, sizeof(int32_t) * (n_states + 1), hipMemcpyHostToDevice, s));
  if (n_arcs) {
    HIP_TRY(hipMemcpyAsync(c->d_ag_int.p + n_states + 1, j.t.arc_src, sizeof(int32_t) * n_arcs, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_ag_lp, j.t.arc_lp, sizeof(float) * n_arcs, hipMemcpyHostToDevice, s));
  }
  float *tail = c->d_ag_lp.p + arcs1;
  if (j.t.start_lp) HIP_TRY(hipMemcpyAsync(tail, j.t.start_lp, sizeof(float) * n_states, hipMemcpyHostToDevice, s));
  if (j.t.final_lp) HIP_TRY(hipMemcpyAsync(tail + n_states, j.t.final_lp, sizeof(float) * n_states, hipMemcpyHostToDevice, s));
  if (j.want_gamma) {
    HIP_TRY(c->d_fb_int.reserve(n_states + 1 + arcs1));
    HIP_TRY(c->d_fb_lp.reserve(arcs1));
    HIP_TRY(hipMemcpyAsync(c->d_fb_int, j.t_ptr.data(), sizeof(int32_t) * (n_states + 1), hipMemcpyHostToDevice, s));
    if (n_arcs) {
      HIP_TRY(hipMemcpyAsync(c->d_fb_int.p + n_states + 1, j.t_src.data(), sizeof(int32_t) * n_arcs, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(c->d_fb_lp, j.t_lp.data(), sizeof(float) * n_arcs, hipMemcpyHostToDevice, s));
    }
  }
  return FDNN_OK;
}

int fb_finish(fdnn_ctx *c, const FbJob &j, float *total, float *gamma, bool host, hipStream_t s) {
  const size_t n_nodes = j.sets.nodes.size(), n_states = j.sets.col.size(), n = size_t(j.t.n_segs);
  const size_t n_arcs = size_t(j.t.arc_ptr[n_states]), words = j.want_gamma ? size_t(j.plan.gamma_words) : 0;
  float *tail = c->d_ag_lp.p + std::max<size_t>(n_arcs, 1);
  FbArgs a;
  a.d_rows = c->d_al_probs, a.d_col = c->d_al_int.p + n_nodes, a.d_state_node = c->d_al_int.p + n_nodes + n_states;
  a.d_log_prior = j.ll->d_log_prior, a.width = j.ll->width, a.floor = j.ll->floor, a.type = j.ll->type;
  a.d_arc_ptr = c->d_ag_int, a.d_arc_src = c->d_ag_int.p + n_states + 1, a.d_arc_lp = c->d_ag_lp;
  a.d_start_lp = j.t.start_lp ? tail : nullptr, a.d_final_lp = j.t.final_lp ? tail + n_states : nullptr;
  if (j.want_gamma) {
    a.d_t_ptr = c->d_fb_int, a.d_t_src = c->d_fb_int.p + n_states + 1, a.d_t_lp = c->d_fb_lp;
    a.d_scratch = reinterpret_cast<float *>(c->d_al_bp.p), a.d_gamma = c->d_fb_res.p + n;
  }
  a.d_total = c->d_fb_res;
  launch_fb(j.plan, a, s);
  HIP_TRY(hipGetLastError());
  if (!host) {
    HIP_TRY(hipMemcpyAsync(total, c->d_fb_res, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    if (words) HIP_TRY(hipMemcpyAsync(gamma, c->d_fb_res.p + n, sizeof(float) * words, hipMemcpyDeviceToDevice, s));
    return FDNN_OK;
  }
  // one transfer of the totals (4 bytes a segment) and one of gamma where asked, straight into the caller's arrays
  HIP_TRY(hipMemcpyAsync(total, c->d_fb_res, sizeof(float) * n, hipMemcpyDeviceToHost, s));
  if (words) HIP_TRY(hipMemcpyAsync(gamma, c->d_fb_res.p + n, sizeof(float) * words, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FDNN_OK;
}

// The host half of a compacted lazy return (lazy_compact_kernel): a compacted row is the row's inactive value followed by
// its active nodes' probabilities in node order; expanding it = every node reads the next active value or the inactive one.
// With AVX-512 that is one expanding load per 16 nodes (the mask's 16 bits select which lanes take the next values from
// memory); checked at run time, scalar otherwise (whole words of inactive / active nodes as runs).  100 frames x 8000 nodes
// at 40 %: 0.55 ms scalar bit by bit (round 5's first form), ~0.05 ms with the expanding loads -- this runs on the caller's
// thread for every utterance, next to a 1.3 MB transfer.
static void expand_row_scalar(float *row, const float *vals, const uint64_t *brow, size_t O) {
  const size_t wpr = (O + 63) / 64;
  const uint64_t tail_mask = (O & 63) ? ((uint64_t(1) << (O & 63)) - 1) : ~uint64_t(0);
  const float inact = vals[0];
  const float *src = vals + 1;
  for (size_t w = 0; w < wpr; ++w) {
    const size_t width = std::min<size_t>(64, O - 64 * w);
    uint64_t word = brow[w];
    if (w + 1 == wpr) word &= tail_mask;
    float *dst = row + 64 * w;
    if (word == 0) {
      std::fill(dst, dst + width, inact);
    } else if (width == 64 && word == ~uint64_t(0)) {
      std::memcpy(dst, src, 64 * sizeof(float));
      src += 64;
    } else {
      for (size_t b = 0; b < width; ++b) dst[b] = ((word >> b) & 1u) ? *src++ : inact;
    }
  }
}

__attribute__((target("avx512f,popcnt"))) static void expand_row_avx512(float *row, const float *vals, const uint64_t *brow, size_t O) {
  const __m512 inact = _mm512_set1_ps(vals[0]);
  const float *src = vals + 1;
  const size_t full = O / 64;
  for (size_t w = 0; w < full; ++w) {
    const uint64_t word = brow[w];
    float *dst = row + 64 * w;
    for (int q = 0; q < 4; ++q) {
      const __mmask16 mk = static_cast<__mmask16>(word >> (16 * q));
      _mm512_storeu_ps(dst + 16 * q, _mm512_mask_expandloadu_ps(inact, mk, src));
      src += __builtin_popcount(static_cast<unsigned>(mk));
    }
  }
  if (O & 63) {  // the last, partial word
    const uint64_t word = brow[full] & ((uint64_t(1) << (O & 63)) - 1);
    float *dst = row + 64 * full;
    for (size_t b = 0; b < (O & 63); ++b) dst[b] = ((word >> b) & 1u) ? *src++ : vals[0];
  }
}

static std::atomic<bool> g_expand_scalar{false};  // fdnn_debug_lazy_expand, mode 1
void lazy_expand_force_scalar(bool on) { g_expand_scalar.store(on, std::memory_order_relaxed); }
static void expand_row(float *row, const float *vals, const uint64_t *brow, size_t O) {
  static const bool wide = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("popcnt");
  if (wide && !g_expand_scalar.load(std::memory_order_relaxed))
    expand_row_avx512(row, vals, brow, O);
  else
    expand_row_scalar(row, vals, brow, O);
}

// `count` compacted rows of `stride` floats sit in the TAIL of the caller's [count][O] block and are expanded front to back
// (row f's place never reaches the compacted rows of later frames; its own is copied aside first).  bits: the rows' masks.
void lazy_expand_rows(float *out, int count, size_t O, size_t stride, const uint64_t *bits) {
  const size_t wpr = (O + 63) / 64;
  const float *land = out + size_t(count) * O - size_t(count) * stride;
  std::vector<float> mine(stride);
  for (int f = 0; f < count; ++f) {
    std::memcpy(mine.data(), land + size_t(f) * stride, sizeof(float) * stride);
    expand_row(out + size_t(f) * O, mine.data(), bits + size_t(f) * wpr, O);
  }
}

// The same from a separate buffer of compacted rows (the scoring loop's pinned landing area).
void lazy_expand_rows_from(float *out, const float *comp, int count, size_t O, size_t stride, const uint64_t *bits) {
  const size_t wpr = (O + 63) / 64;
  for (int f = 0; f < count; ++f) expand_row(out + size_t(f) * O, comp + size_t(f) * stride, bits + size_t(f) * wpr, O);
}

}  // namespace fdnn

extern "C" const char *fdnn_last_error(void) { return g_err.c_str(); }
