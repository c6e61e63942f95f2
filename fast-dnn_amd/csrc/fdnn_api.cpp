// fdnn_api.cpp -- the scoring C-ABI (include/fdnn.h): model load / free / queries, calculation contexts, the one-call
// entry points (dense, lazy, raw frames) and streams of raw frames.  Argument checks and the choice of a chunk list; the
// passes themselves are fdnn_runtime.cpp's.
#include <hip/hip_runtime.h>
#include <emmintrin.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "fdnn_internal.hpp"
#include "fdnn_lists.hpp"
#include "fdnn_stream_plan.hpp"

using namespace fdnn;
using fdnn::pass::Pass;

namespace fdnn {

int calculate_on_one_device(fdnn_model *m, const float *x, int n, int dim, int batch_hint, float *out) {
  (void)batch_hint;
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;  // QuantizedDnn.java:154-156
  if (!x || !out) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  if (m->batcher) {  // coalesced with the other callers' utterances (fdnn_server.cpp)
    uint64_t ticket = 0;
    return batcher_wait(m->batcher, fdnn_server_submit(m->batcher, x, n, nullptr, out, &ticket), &ticket);
  }
  return score_chunks(m, {{0, n}}, Pass::host_dense("fdnn_calculate", x, out));
}

int calculate_raw_rows(fdnn_model *m, const SpliceRef &spec, const float *raw, int n, int a, int b, float *out) {
  if (b <= a) return FDNN_OK;
  if (m->batcher) {  // coalesced with the other callers' raw utterances (fdnn_server.cpp), each with its own edges
    uint64_t ticket = 0;
    return batcher_wait(m->batcher, server_submit_raw_rows(m->batcher, spec, raw, n, a, b, nullptr, out, &ticket), &ticket);
  }
  int fa, fb;  // the raw frames those rows reference travel once
  splice_halo(*spec, n, a, b, &fa, &fb);
  const std::vector<SpliceSeg> segs{SpliceSeg{a, a - fa, -fa, n - 1 - fa}};
  return score_chunks(m, frame_chunks(b - a, m), Pass::raw_dense("fdnn_calculate_raw", {spec.get(), &segs, raw + size_t(fa) * size_t(spec->raw_dim), fb - fa, a}, out));
}

}  // namespace fdnn

extern "C" {

const char *fdnn_version(void) { return "fast-dnn_amd 0.1 (gfx950)"; }

int fdnn_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

int fdnn_model_load_on(const char *path, float cutoff, int device, fdnn_model **out) {
  if (!path || !out) return fail(FDNN_E_ARG, "null argument");
  *out = nullptr;
  std::unique_ptr<fdnn_model> own(new fdnn_model());  // (a load that fails half way: what it allocated goes with the model)
  fdnn_model *m = own.get();
  std::string msg;
  int rc = fdnn::load_host_model(path, cutoff, &m->hm, &msg);
  if (rc) return fail(rc, msg);
  m->device = device;
  rc = upload_model(m);
  if (rc) return rc;
  (void)fdnn_device_shared(device);  // take (or find taken) the device's process marker now, not at the first large call
  if (const char *env = std::getenv("FDNN_BATCHER")) {  // max_frames[:depth[:linger_us]]
    int mf = 0, depth = 2, linger = 0;
    if (std::sscanf(env, "%d:%d:%d", &mf, &depth, &linger) >= 1 && mf > 0) {
      rc = fdnn_model_enable_batcher(m, mf, depth, linger);
      if (rc) {
        fdnn_model_free(own.release());
        return rc;
      }
    }
  }
  *out = own.release();
  return FDNN_OK;
}

int fdnn_model_load(const char *path, float cutoff, fdnn_model **out) {
  // FDNN_DEVICES="0,1,2,3" or "all": one replica per listed device, weights distributed at load,
  // fdnn_calculate on the returned handle shards its frames over them (fdnn_group.cpp) -- how the
  // unmodified Java class reaches every GPU of the node.
  if (const char *env = std::getenv("FDNN_DEVICES")) {
    std::vector<int> devs;
    if (std::strcmp(env, "all") == 0) {
      for (int d = 0; d < fdnn_device_count(); ++d) devs.push_back(d);
    } else {
      for (const char *q = env; *q;) {
        char *end = nullptr;
        const long v = std::strtol(q, &end, 10);
        if (end == q) break;
        devs.push_back(int(v));
        q = (*end == ',') ? end + 1 : end;
      }
    }
    if (devs.size() > 1) {
      if (!out) return fail(FDNN_E_ARG, "null argument");
      fdnn_group *g = nullptr;
      int rc = fdnn_group_load(path, cutoff, devs.data(), int(devs.size()), &g);
      if (rc) return rc;
      fdnn_group_attach(g);
      *out = fdnn_group_model(g, 0);
      return FDNN_OK;
    }
    if (devs.size() == 1) return fdnn_model_load_on(path, cutoff, devs[0], out);
  }
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  return fdnn_model_load_on(path, cutoff, dev, out);
}

int fdnn_model_enable_batcher(fdnn_model *m, int max_frames, int depth, int linger_us) {
  if (!m) return fail(FDNN_E_ARG, "null model");
  if (m->batcher) return fail(FDNN_E_STATE, "the model already has a batcher");
  fdnn_server *srv = nullptr;
  int rc = fdnn_server_create(m, max_frames, depth, &srv);
  if (!rc) rc = fdnn_server_set_linger_us(srv, linger_us);
  if (rc) {
    fdnn_server_free(srv);
    return rc;
  }
  m->batcher = srv;
  return FDNN_OK;
}

void fdnn_model_free(fdnn_model *m) {
  if (!m) return;
  if (m->group) {  // the leader of an attached group: the group owns every replica, this one included
    fdnn_group_free(m->group);
    return;
  }
  if (m->batcher) fdnn_server_free(m->batcher);
  m->batcher = nullptr;
  for (fdnn_ctx *c : m->pool) destroy_ctx(c);
  m->pool.clear();
  DeviceGuard g(m->device);
  delete m;
}

int fdnn_model_input_dim(const fdnn_model *m) { return m ? m->hm.hdr.in_dim : -1; }
int fdnn_model_output_dim(const fdnn_model *m) { return m ? m->hm.hdr.out_dim : -1; }
int fdnn_model_hidden_dim(const fdnn_model *m) { return m ? m->hm.hdr.hidden : -1; }
int fdnn_model_layer_count(const fdnn_model *m) { return m ? m->hm.hdr.n_q + 1 : -1; }  // jni_dnn.cc:155
int fdnn_model_device(const fdnn_model *m) { return m ? m->device : -1; }

int fdnn_model_layer_dim(const fdnn_model *m, int index) {
  if (!m) return -1;
  const BlobHeader &h = m->hm.hdr;
  if (index < 0) return -1;
  if (index == 0) return h.hidden;           // input_layer()->node_count(), jni_dnn.cc:144-146
  if (index >= h.n_q) return -1;             // layers()[index] must exist (see fdnn.h)
  return h.q[index].rows;                    // layers()[index]->node_count(), jni_dnn.cc:147
}

int fdnn_model_set_l0_fma(fdnn_model *m, int on) {
  if (!m) return fail(FDNN_E_ARG, "null model");
  m->l0_fma = on ? 1 : 0;
  return FDNN_OK;
}

int fdnn_model_set_lists_union(fdnn_model *m, int group_tiles) {
  if (!m) return fail(FDNN_E_ARG, "null model");
  const int g = lunion::group_tiles_of(group_tiles);
  if (g < 0) return fail(FDNN_E_ARG, "group_tiles is 0 (off), 1 .. " + std::to_string(lunion::kMaxGroupTiles) + ", or -1 (the default group)");
  m->lists_union = g;
  return FDNN_OK;
}

int fdnn_device_shared(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return fail(FDNN_E_ARG, "no such device");
  return device_marker_state(device) == 1 ? 0 : 1;
}

// ---------------------------------------------------------------- contexts
int fdnn_ctx_create(fdnn_model *m, int n, int batch_hint, fdnn_ctx **out) {
  (void)batch_hint;  // frame blocking is a CPU cache device; results never depend on it
  if (!m || !out) return fail(FDNN_E_ARG, "null argument");
  if (n < 0) return fail(FDNN_E_ARG, "negative frame count");
  return make_ctx(m, n, out);
}

void fdnn_ctx_free(fdnn_ctx *c) {
  if (!c) return;
  destroy_ctx(c);
}

int fdnn_ctx_frame_count(const fdnn_ctx *c) { return c ? c->n : -1; }
int fdnn_ctx_output_dim(const fdnn_ctx *c) { return c ? c->m->hm.hdr.out_dim : -1; }

int fdnn_ctx_forward_hidden_device(fdnn_ctx *c, const float *d_x, void *stream) {
  if (!c || (!d_x && c->n)) return fail(FDNN_E_ARG, "null argument");
  if (c->n == 0) {
    c->last = 0;
    return FDNN_OK;
  }
  if (int rc = check_frames_aligned(d_x)) return rc;
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  return run_hidden(c, d_x, s, nullptr);
}

int fdnn_ctx_forward_hidden(fdnn_ctx *c, const float *x) {
  if (!c || (!x && c->n)) return fail(FDNN_E_ARG, "null argument");
  if (c->n == 0) {
    c->last = 0;
    return FDNN_OK;
  }
  DeviceGuard g(c->m->device);
  const BlobHeader &h = c->m->hm.hdr;
  CtxUse use;
  HIP_TRY(use.enter(c, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_x, x, sizeof(float) * size_t(c->n) * h.in_dim, hipMemcpyHostToDevice, c->stream));
  int rc = run_hidden(c, c->d_x, c->stream, nullptr);
  use.leave();
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return FDNN_OK;
}

int fdnn_ctx_lazy_output_batch_device(fdnn_ctx *c, int first, int count, const int8_t *d_masks, float *d_out,
                                      void *stream) {
  if (!c || !d_out) return fail(FDNN_E_ARG, "null argument");
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  return run_output(c, {.first = first, .count = count, .d_masks = d_masks, .d_out = d_out}, s);
}

// masks [count][O] bytes (non-zero = active, dnn.cc:361) -> bits [count][ceil(O / 64)], 16 bytes per step
static void pack_mask_rows(const int8_t *masks, int count, size_t O, uint64_t *bits) {
  const size_t wpr = (O + 63) / 64;
  const __m128i zero = _mm_setzero_si128();
  for (int f = 0; f < count; ++f) {
    const int8_t *mrow = masks + size_t(f) * O;
    uint64_t *brow = bits + size_t(f) * wpr;
    size_t k = 0;
    for (size_t w = 0; w < wpr; ++w) {
      uint64_t word = 0;
      for (int q = 0; q < 4 && k + 16 <= O; ++q, k += 16) {
        const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i *>(mrow + k));
        word |= uint64_t(uint32_t(~_mm_movemask_epi8(_mm_cmpeq_epi8(v, zero))) & 0xffffu) << (16 * q);
      }
      const size_t base = 64 * w;
      for (; k < O && k < base + 64; ++k) word |= uint64_t(mrow[k] != 0) << (k - base);
      brow[w] = word;
    }
  }
}

int fdnn_ctx_lazy_output_batch(fdnn_ctx *c, int first, int count, const int8_t *masks, float *out) {
  if (!c || !out || !masks) return fail(FDNN_E_ARG, "null argument");
  if (c->last < 0) return fail(FDNN_E_STATE, "calculateLazy before calculateUntilOutput");
  if (first < 0 || count < 0 || first + count > c->n) return fail(FDNN_E_ARG, "frame index outside the context");
  if (count == 0) return FDNN_OK;
  DeviceGuard g(c->m->device);
  const BlobHeader &h = c->m->hm.hdr;
  const size_t O = size_t(h.out_dim);
  CtxUse use;
  HIP_TRY(use.enter(c, c->stream));
  if (count <= kPinFrames) {  // the per-frame protocol: no copy commands (see fdnn_ctx)
    std::memcpy(c->h_mask_pin, masks, size_t(count) * O);
    // (blocks of 1..8 frames go through the small GEMM kernel's 32-frame tile, which reads the mask bytes straight from the
    // host-mapped staging; nets the small kernel cannot take -- K > 2048, no validated fast division -- fall to the large
    // tiles behind a mask_pack pass over the same staging)
    const int rc = run_output(c, {.first = first, .count = count, .d_masks = c->h_mask_pin.dev, .d_out = c->d_out, .d_final = c->h_out_pin.dev}, c->stream);
    use.leave();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(out, c->h_out_pin, sizeof(float) * size_t(count) * O);
    return FDNN_OK;
  }
  HIP_TRY(hipMemcpyAsync(c->d_mask, masks, size_t(count) * O, hipMemcpyHostToDevice, c->stream));
  c->mask_bits_packed = false;
  int rc = run_output(c, {.first = first, .count = count, .d_masks = c->d_mask, .d_out = c->d_out}, c->stream);
  if (!rc) {
    // the same masks as bits, for the compacted return (lazy_copy_out): on the host while the GPU computes, on the device
    // by the pack kernel (a large batch's output kernel has run it already)
    const size_t wpr = (O + 63) / 64;
    std::vector<uint64_t> hb(size_t(count) * wpr, 0);
    pack_mask_rows(masks, count, O, hb.data());
    if (!c->mask_bits_packed) fdnn::launch_mask_pack(c->d_mask, c->d_mask_bits, count, int(O), c->stream);  // (a large batch's output kernel has)
    rc = lazy_copy_out(c, count, c->d_mask_bits, hb.data(), out, c->stream);
  }
  return rc;
}

int fdnn_ctx_lazy_output_batch_bits_device(fdnn_ctx *c, int first, int count, const uint64_t *d_bits, float *d_out, void *stream) {
  if (!c || !d_out || !d_bits) return fail(FDNN_E_ARG, "null argument");
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  return run_output(c, {.first = first, .count = count, .d_bits = d_bits, .d_out = d_out}, s);
}

int fdnn_ctx_lazy_output_batch_bits(fdnn_ctx *c, int first, int count, const uint64_t *bits, float *out) {
  if (!c || !out || !bits) return fail(FDNN_E_ARG, "null argument");
  if (c->last < 0) return fail(FDNN_E_STATE, "calculateLazy before calculateUntilOutput");
  if (first < 0 || count < 0 || first + count > c->n) return fail(FDNN_E_ARG, "frame index outside the context");
  if (count == 0) return FDNN_OK;
  DeviceGuard g(c->m->device);
  const BlobHeader &h = c->m->hm.hdr;
  const size_t O = size_t(h.out_dim), wpr = (O + 63) / 64;
  CtxUse use;
  HIP_TRY(use.enter(c, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_mask_bits, bits, sizeof(uint64_t) * size_t(count) * wpr, hipMemcpyHostToDevice, c->stream));
  int rc = run_output(c, {.first = first, .count = count, .d_bits = c->d_mask_bits, .d_out = c->d_out}, c->stream);
  if (!rc) rc = lazy_copy_out(c, count, c->d_mask_bits, bits, out, c->stream);
  return rc;
}

// ---------------------------------------------------------------- lazy output by active-node lists (fdnn_lists.hip)
// FDNN_E_ARG naming the first row whose list is not a mask in list form (fdnn_lists.hpp: check)
static int lists_validate(const int32_t *row_ptr, const int32_t *nodes, int count, int output_dim) {
  const int bad = lists::check(row_ptr, nodes, count, output_dim);
  if (!bad) return FDNN_OK;
  return fail(FDNN_E_ARG, "active list of row " + std::to_string(-bad - 1) + ": row_ptr must start at 0 and never decrease, a row's nodes must ascend strictly inside [0, " +
                              std::to_string(output_dim) + ")");
}

// The common front of the host forms of a lazy-entries call (lists, set, sets): the texts their callers see, whatever
// run_lists / run_set / run_sets say of the same conditions to the device forms and the scoring loop.
static int ctx_entries_front(const fdnn_ctx *c, bool args_given, int first, int count) {
  if (!c || !args_given) return fail(FDNN_E_ARG, "null argument");
  if (c->last < 0) return fail(FDNN_E_STATE, "calculateLazy before calculateUntilOutput");
  if (first < 0 || count < 0 || first + count > c->n) return fail(FDNN_E_ARG, "frame index outside the context");
  return FDNN_OK;
}

// Their common end: the result-buffer rule (the parity forms bring acc alone), then the host form on the context's stream.
static int ctx_entries_to_host(fdnn_ctx *c, long long nnz, const HostEntries &h) {
  if ((!h.acc && !h.inactive) || (nnz > 0 && !h.acc && !h.probs)) return fail(FDNN_E_ARG, "null result buffer");
  DeviceGuard g(c->m->device);
  CtxUse use;
  HIP_TRY(use.enter(c, c->stream));
  return entries_to_host(c, h, c->stream);
}

static int ctx_lists_host(fdnn_ctx *c, int first, int count, const int32_t *row_ptr, const int32_t *nodes, float *probs, float *inactive,
                          int32_t *acc) {
  if (int rc = ctx_entries_front(c, row_ptr != nullptr, first, count)) return rc;
  if (count == 0) return FDNN_OK;
  if (int rc = lists_validate(row_ptr, nodes, count, c->m->hm.hdr.out_dim)) return rc;
  return ctx_entries_to_host(c, row_ptr[count], {.first = first, .count = count, .row_ptr = row_ptr, .nodes = nodes, .n_nodes = row_ptr[count],
                                                 .probs = probs, .inactive = inactive, .acc = acc});
}

int fdnn_ctx_lazy_output_lists(fdnn_ctx *c, int first, int count, const int32_t *row_ptr, const int32_t *nodes, float *probs,
                               float *inactive) {
  return ctx_lists_host(c, first, count, row_ptr, nodes, probs, inactive, nullptr);
}

int fdnn_debug_ctx_lists_acc(fdnn_ctx *c, int first, int count, const int32_t *row_ptr, const int32_t *nodes, int32_t *acc) {
  if (!acc) return fail(FDNN_E_ARG, "null argument");
  return ctx_lists_host(c, first, count, row_ptr, nodes, nullptr, nullptr, acc);
}

int fdnn_ctx_lazy_output_lists_device(fdnn_ctx *c, int first, int count, const int32_t *d_row_ptr, const int32_t *d_nodes, int nnz,
                                      float *d_probs, float *d_inactive, void *stream) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  return run_lists(c, {first, count, d_row_ptr, d_nodes, nnz, d_probs, d_inactive, nullptr}, s);
}

int fdnn_debug_lists_check(const int32_t *row_ptr, const int32_t *nodes, int count, int output_dim) {
  if (!row_ptr || count < 0) return fail(FDNN_E_ARG, "bad argument");
  return lists::check(row_ptr, nodes, count, output_dim);
}

// The first `cap` of a launcher's n (<= 4) counts (fdnn_launch.hpp: LaunchCounts) into out; returns n
static int counts_out(unsigned long long *out, int cap, int n, void (*reader)(unsigned long long *)) {
  if (!out || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  unsigned long long v[4];
  reader(v);
  for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
  return n;
}

int fdnn_debug_lists_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 3, fdnn::lists_launch_counts); }

int fdnn_debug_lists_union_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 4, fdnn::lists_union_launch_counts); }

// The union-build kernel alone on validated host lists: words it does not write come back as -1.
int fdnn_debug_ctx_lists_union(fdnn_ctx *c, int first, int count, const int32_t *row_ptr, const int32_t *nodes, int group_tiles, int32_t *u_len,
                               int32_t *u_nodes, int32_t *pos) {
  if (!c || !row_ptr || !u_len) return fail(FDNN_E_ARG, "null argument");
  if (group_tiles < 1 || group_tiles > lunion::kMaxGroupTiles) return fail(FDNN_E_ARG, "group_tiles is 1 .. " + std::to_string(lunion::kMaxGroupTiles));
  if (first < 0 || count < 0 || first + count > c->n) return fail(FDNN_E_ARG, "frame index outside the context");
  if (count == 0) return FDNN_OK;
  const int O = c->m->hm.hdr.out_dim;
  if (int rc = lists_validate(row_ptr, nodes, count, O)) return rc;
  if (O > lunion::kMaxNodes) return fail(FDNN_E_ARG, "the union bitset holds " + std::to_string(lunion::kMaxNodes) + " nodes");
  const size_t nnz = size_t(row_ptr[count]);
  if (nnz > 0 && (!u_nodes || !pos)) return fail(FDNN_E_ARG, "null result buffer");
  const lunion::Layout l = lunion::layout(static_cast<long long>(nnz), count, group_tiles);
  if (nnz == 0) {
    std::fill(u_len, u_len + l.n_groups, 0);
    return FDNN_OK;
  }
  DeviceGuard g(c->m->device);
  hipStream_t s = c->stream;
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  HIP_TRY(c->d_lrow.reserve(size_t(count) + 1));
  HIP_TRY(c->d_lnodes.reserve(nnz));
  HIP_TRY(c->d_lprobs.reserve(nnz));
  HIP_TRY(c->d_union.reserve(l.words));
  int32_t *const b = c->d_union.p;
  HIP_TRY(hipMemcpyAsync(c->d_lrow, row_ptr, sizeof(int32_t) * (size_t(count) + 1), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->d_lnodes, nodes, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(b, 0xff, sizeof(int32_t) * l.words, s));
  const UnionParams u = union_params(l, b, {0, count, c->d_lrow, c->d_lnodes, int(nnz), c->d_lprobs}, O, group_tiles);
  HIP_TRY(launch_lists_union_build(u, l.n_groups, s));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(u_len, b + l.u_len, sizeof(int32_t) * size_t(l.n_groups), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(u_nodes, b + l.u_nodes, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(pos, b + l.pos, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FDNN_OK;
}

// The same in plain C++ (fdnn_lists_union.hpp: union_ref), no device; the lists are validated, nnz is row_ptr[count].
int fdnn_debug_lists_union_ref(const int32_t *row_ptr, const int32_t *nodes, int count, int output_dim, int group_tiles, int32_t *u_len,
                               int32_t *u_nodes, int32_t *pos) {
  if (!row_ptr || !u_len || count < 0 || output_dim < 1) return fail(FDNN_E_ARG, "bad argument");
  if (group_tiles < 1 || group_tiles > lunion::kMaxGroupTiles) return fail(FDNN_E_ARG, "group_tiles is 1 .. " + std::to_string(lunion::kMaxGroupTiles));
  if (count == 0) return FDNN_OK;
  if (int rc = lists_validate(row_ptr, nodes, count, output_dim)) return rc;
  const int nnz = row_ptr[count];
  if (nnz > 0 && (!u_nodes || !pos)) return fail(FDNN_E_ARG, "null result buffer");
  std::fill(u_nodes, u_nodes + nnz, -1);
  std::fill(pos, pos + nnz, -1);
  lunion::union_ref(row_ptr, nodes, count, nnz, output_dim, group_tiles, u_len, u_nodes, pos);
  return FDNN_OK;
}

// One-call form: hidden layers + lists on a pooled context, a large n chunk by chunk with its slice of the lists rebased.
int fdnn_calculate_lazy_lists(fdnn_model *m, const float *x, int n, int dim, const int32_t *row_ptr, const int32_t *nodes, float *probs,
                              float *inactive) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!x || !row_ptr || !inactive) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  if (int rc = lists_validate(row_ptr, nodes, n, m->hm.hdr.out_dim)) return rc;
  if (row_ptr[n] > 0 && !probs) return fail(FDNN_E_ARG, "null buffer");
  return score_chunks(m, frame_chunks(n, m), Pass::host_lists("fdnn_calculate_lazy_lists", x, row_ptr, nodes, probs, inactive));
}

// ---------------------------------------------------------------- lazy output for a shared node set (fdnn_set.hip)
// The set is the one-row list {0, len} (fdnn_lists.hpp: check)
static int set_validate(const int32_t *nodes, int len, int output_dim) {
  if (len < 0) return fail(FDNN_E_ARG, "negative set length");
  const int32_t row_ptr[2] = {0, len};
  if (!lists::check(row_ptr, nodes, 1, output_dim)) return FDNN_OK;
  return fail(FDNN_E_ARG, "node set: the nodes must ascend strictly inside [0, " + std::to_string(output_dim) + ")");
}

static int ctx_set_host(fdnn_ctx *c, int first, int count, const int32_t *nodes, int len, float *probs, float *inactive, int32_t *acc) {
  if (int rc = ctx_entries_front(c, true, first, count)) return rc;
  if (int rc = set_validate(nodes, len, c->m->hm.hdr.out_dim)) return rc;
  if (static_cast<long long>(count) * len > INT32_MAX) return fail(FDNN_E_ARG, "count x len must fit an int32");
  if (count == 0) return FDNN_OK;
  return ctx_entries_to_host(c, len, {.first = first, .count = count, .len = len, .nodes = nodes, .n_nodes = len, .probs = probs,
                                      .inactive = inactive, .acc = acc});
}

int fdnn_ctx_lazy_output_set(fdnn_ctx *c, int first, int count, const int32_t *nodes, int len, float *probs, float *inactive) {
  return ctx_set_host(c, first, count, nodes, len, probs, inactive, nullptr);
}

int fdnn_debug_ctx_set_acc(fdnn_ctx *c, int first, int count, const int32_t *nodes, int len, int32_t *acc) {
  if (!acc) return fail(FDNN_E_ARG, "null argument");
  return ctx_set_host(c, first, count, nodes, len, nullptr, nullptr, acc);
}

int fdnn_ctx_lazy_output_set_device(fdnn_ctx *c, int first, int count, const int32_t *d_nodes, int len, float *d_probs, float *d_inactive,
                                    void *stream) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  return run_set(c, {first, count, d_nodes, len, d_probs, d_inactive, nullptr}, s);
}

int fdnn_debug_set_check(const int32_t *nodes, int len, int output_dim) {
  if (len < 0 || (len > 0 && !nodes)) return fail(FDNN_E_ARG, "bad argument");
  const int32_t row_ptr[2] = {0, len};
  return lists::check(row_ptr, nodes, 1, output_dim);
}

int fdnn_debug_set_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 3, fdnn::set_launch_counts); }

int fdnn_debug_set_kernel(int mode) {
  if (mode < 0 || mode > 2) return fail(FDNN_E_ARG, "mode is 0 (the default rule), 1 (the MFMA kernel) or 2 (the list kernels)");
  fdnn::set_kernel_mode(mode);
  return FDNN_OK;
}

// One-call form: hidden layers + the set on a pooled context, a large n chunk by chunk, every chunk with the same set.
int fdnn_calculate_lazy_set(fdnn_model *m, const float *x, int n, int dim, const int32_t *nodes, int len, float *probs, float *inactive) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = set_validate(nodes, len, m->hm.hdr.out_dim)) return rc;
  if (static_cast<long long>(n) * len > INT32_MAX) return fail(FDNN_E_ARG, "count x len must fit an int32");
  if (n == 0) return FDNN_OK;
  if (!x || !inactive || (len > 0 && !probs)) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::host_set("fdnn_calculate_lazy_set", x, nodes, len, probs, inactive));
}

// ---------------------------------------------------------------- lazy output for per-segment node sets (fdnn_sets.hip)
// FDNN_E_ARG names the first malformed segment (fdnn_sets.hpp: check)
static int sets_validate(const int32_t *seg_rows, const int32_t *set_ptr, const int32_t *nodes, int n_segs, int output_dim, int ctx_rows) {
  if (n_segs < 0) return fail(FDNN_E_ARG, "negative segment count");
  const int bad = sets::check(seg_rows, set_ptr, nodes, n_segs, output_dim, ctx_rows);
  if (!bad) return FDNN_OK;
  return fail(FDNN_E_ARG, "node sets, segment " + std::to_string(-bad - 1) + ": seg_rows must not decrease inside [0, " + std::to_string(ctx_rows) +
                              "], set_ptr must begin at 0 and not decrease, a set's nodes must ascend strictly inside [0, " +
                              std::to_string(output_dim) + ")");
}

static int ctx_sets_host(fdnn_ctx *c, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs, const int32_t *nodes, float *probs,
                         float *inactive, int32_t *acc) {
  if (int rc = ctx_entries_front(c, true, 0, 0)) return rc;  // (the row range is the tables': sets_validate)
  if (int rc = sets_validate(seg_rows, set_ptr, nodes, n_segs, c->m->hm.hdr.out_dim, c->n)) return rc;
  if (n_segs == 0) return FDNN_OK;
  const sets::Tables t{seg_rows, set_ptr, n_segs};
  const long long nnz = sets::total(t);
  if (nnz > INT32_MAX) return fail(FDNN_E_ARG, "the sum of rows x len over the segments must fit an int32");
  const int count = seg_rows[n_segs] - seg_rows[0];
  if (count == 0) return FDNN_OK;
  const std::vector<sets::Seg> segs = sets::slice(t, seg_rows[0], seg_rows[n_segs]);
  return ctx_entries_to_host(c, nnz, {.first = seg_rows[0], .count = count, .segs = &segs, .nodes = nodes, .n_nodes = set_ptr[n_segs],
                                      .probs = probs, .inactive = inactive, .acc = acc});
}

int fdnn_ctx_lazy_output_sets(fdnn_ctx *c, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs, const int32_t *nodes, float *probs,
                              float *inactive) {
  return ctx_sets_host(c, seg_rows, set_ptr, n_segs, nodes, probs, inactive, nullptr);
}

int fdnn_debug_ctx_sets_acc(fdnn_ctx *c, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs, const int32_t *nodes, int32_t *acc) {
  if (!acc) return fail(FDNN_E_ARG, "null argument");
  return ctx_sets_host(c, seg_rows, set_ptr, n_segs, nodes, nullptr, nullptr, acc);
}

// The tables are host memory and are checked (the plan is made from them); the nodes are on the device and are not.
int fdnn_ctx_lazy_output_sets_device(fdnn_ctx *c, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs, const int32_t *d_nodes,
                                     float *d_probs, float *d_inactive, void *stream) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  if (int rc = lazy_state(c)) return rc;
  if (n_segs < 0) return fail(FDNN_E_ARG, "negative segment count");
  if (n_segs == 0) return FDNN_OK;
  if (!seg_rows || !set_ptr || seg_rows[0] < 0 || set_ptr[0] != 0) return fail(FDNN_E_ARG, "node sets, segment 0: malformed tables");
  for (int s = 0; s < n_segs; ++s)
    if (seg_rows[s + 1] < seg_rows[s] || seg_rows[s + 1] > c->n || set_ptr[s + 1] < set_ptr[s] || set_ptr[s + 1] - set_ptr[s] > c->m->hm.hdr.out_dim)
      return fail(FDNN_E_ARG, "node sets, segment " + std::to_string(s) + ": malformed tables");
  const sets::Tables t{seg_rows, set_ptr, n_segs};
  if (sets::total(t) > INT32_MAX) return fail(FDNN_E_ARG, "the sum of rows x len over the segments must fit an int32");
  const std::vector<sets::Seg> segs = sets::slice(t, seg_rows[0], seg_rows[n_segs]);
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  SetsCall sc;
  sc.first = seg_rows[0], sc.segs = &segs, sc.d_nodes = d_nodes, sc.d_probs = d_probs, sc.d_inactive = d_inactive;
  return run_sets(c, sc, s);
}

int fdnn_debug_sets_check(const int32_t *seg_rows, const int32_t *set_ptr, const int32_t *nodes, int n_segs, int output_dim, int ctx_rows) {
  if (n_segs < 0) return fail(FDNN_E_ARG, "bad argument");
  return sets::check(seg_rows, set_ptr, nodes, n_segs, output_dim, ctx_rows);
}

int fdnn_debug_sets_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 3, fdnn::sets_launch_counts); }

// One-call form: hidden layers + the sets on a pooled context, a large n chunk by chunk, every chunk with its slice of the
// segments (a segment cut in two keeps its set).
int fdnn_calculate_lazy_sets(fdnn_model *m, const float *x, int n, int dim, const int32_t *seg_rows, const int32_t *set_ptr, int n_segs,
                             const int32_t *nodes, float *probs, float *inactive) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = sets_validate(seg_rows, set_ptr, nodes, n_segs, m->hm.hdr.out_dim, n)) return rc;
  if (n_segs == 0 ? n != 0 : (seg_rows[0] != 0 || seg_rows[n_segs] != n)) return fail(FDNN_E_ARG, "seg_rows must cover the rows [0, n)");
  if (n == 0) return FDNN_OK;
  const sets::Tables t{seg_rows, set_ptr, n_segs};
  const long long nnz = sets::total(t);
  if (nnz > INT32_MAX) return fail(FDNN_E_ARG, "the sum of rows x len over the segments must fit an int32");
  if (!x || !inactive || (nnz > 0 && !probs)) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::host_sets("fdnn_calculate_lazy_sets", x, t, nodes, probs, inactive));
}

int fdnn_ctx_lazy_output(fdnn_ctx *c, int frame, const int8_t *mask, float *out) {
  return fdnn_ctx_lazy_output_batch(c, frame, 1, mask, out);
}

int fdnn_ctx_output_device(fdnn_ctx *c, float *d_out, void *stream) {
  if (!c || !d_out) return fail(FDNN_E_ARG, "null argument");
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  return run_output(c, {.count = c->n, .d_out = d_out}, s);
}

int fdnn_ctx_output(fdnn_ctx *c, float *out) {
  if (!c || !out) return fail(FDNN_E_ARG, "null argument");
  if (c->n == 0) return FDNN_OK;
  DeviceGuard g(c->m->device);
  CtxUse use;
  HIP_TRY(use.enter(c, c->stream));
  int rc = run_output(c, {.count = c->n, .d_out = c->d_out}, c->stream);
  use.leave();
  if (rc) return rc;
  return copy_out(out, c->d_out, sizeof(float) * size_t(c->n) * c->m->hm.hdr.out_dim, c->stream);
}

// ---------------------------------------------------------------- dense output with a top-k return (fdnn_topk.hip)
static int topk_k_check(int width, int k) {
  if (fdnn::topk::args_ok(width, k)) return FDNN_OK;
  return fail(FDNN_E_ARG, "k is 1 .. min(row width, " + std::to_string(fdnn::topk::kTopkMaxK) + ")");
}

int fdnn_topk_rows_device(const float *d_rows, int n, int width, int k, int32_t *d_nodes, float *d_vals, void *stream) {
  if (n < 0 || width < 1) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = topk_k_check(width, k)) return rc;
  if (n == 0) return FDNN_OK;
  if (!d_rows || !d_nodes || !d_vals) return fail(FDNN_E_ARG, "null buffer");
  fdnn::launch_topk(d_rows, n, width, k, d_nodes, d_vals, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

int fdnn_ctx_output_topk_device(fdnn_ctx *c, int k, int32_t *d_nodes, float *d_probs, void *stream) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  if (int rc = lazy_state(c)) return rc;
  if (int rc = topk_k_check(c->m->hm.hdr.out_dim, k)) return rc;
  if (c->n == 0) return FDNN_OK;
  if (!d_nodes || !d_probs) return fail(FDNN_E_ARG, "null buffer");
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  if (!c->d_out) HIP_TRY(c->d_out.reserve(size_t(c->cap) * size_t(c->m->hm.hdr.out_dim)));  // (a lean context)
  if (int rc = run_output(c, {.count = c->n, .d_out = c->d_out}, s)) return rc;
  fdnn::launch_topk(c->d_out, c->n, c->m->hm.hdr.out_dim, k, d_nodes, d_probs, s);
  return FDNN_OK;
}

int fdnn_ctx_output_topk(fdnn_ctx *c, int k, int32_t *nodes, float *probs) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  if (int rc = lazy_state(c)) return rc;
  if (int rc = topk_k_check(c->m->hm.hdr.out_dim, k)) return rc;
  if (c->n == 0) return FDNN_OK;
  if (!nodes || !probs) return fail(FDNN_E_ARG, "null buffer");
  DeviceGuard g(c->m->device);
  CtxUse use;
  HIP_TRY(use.enter(c, c->stream));
  if (!c->d_out) HIP_TRY(c->d_out.reserve(size_t(c->cap) * size_t(c->m->hm.hdr.out_dim)));  // (a lean context)
  return dense_pass(c, {.k = k, .nodes = nodes, .probs = probs}, c->stream, /*hidden=*/false);
}

int fdnn_calculate_topk(fdnn_model *m, const float *x, int n, int dim, int k, int32_t *nodes, float *probs) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = topk_k_check(m->hm.hdr.out_dim, k)) return rc;
  if (n == 0) return FDNN_OK;
  if (!x || !nodes || !probs) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::host_topk("fdnn_calculate_topk", x, k, nodes, probs));
}

int fdnn_calculate_topk_raw(fdnn_model *m, const float *raw, int n, int raw_dim, int k, int32_t *nodes, float *probs) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  if (int rc = fdnn::splice_check(spec, raw_dim)) return rc;
  if (int rc = topk_k_check(m->hm.hdr.out_dim, k)) return rc;
  if (n == 0) return FDNN_OK;
  if (!raw || !nodes || !probs) return fail(FDNN_E_ARG, "null buffer");
  const std::vector<SpliceSeg> segs{SpliceSeg{0, 0, 0, n - 1}};  // (the whole utterance's raw frames travel once, as fdnn_calculate_raw's)
  return score_chunks(m, frame_chunks(n, m), Pass::raw_topk("fdnn_calculate_topk_raw", {spec.get(), &segs, raw, n}, k, nodes, probs));
}

int fdnn_calculate_topk_device(fdnn_model *m, const float *d_x, int n, int k, int32_t *d_nodes, float *d_probs, void *stream) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = topk_k_check(m->hm.hdr.out_dim, k)) return rc;
  if (n == 0) return FDNN_OK;
  if (!d_x || !d_nodes || !d_probs) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_frames_aligned(d_x)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::device_topk("fdnn_calculate_topk_device", d_x, k, d_nodes, d_probs), static_cast<hipStream_t>(stream));
}

int fdnn_debug_topk_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 2, fdnn::topk_launch_counts); }

int fdnn_debug_set_topk_kernel(int mode) {
  if (mode < 0 || mode > 2) return fail(FDNN_E_ARG, "mode is 0 (the plan's rule), 1 (resident where the width allows) or 2 (streaming)");
  fdnn::topk_kernel_mode(mode);
  return FDNN_OK;
}

// The selection in plain C++ (fdnn_topk.hpp: ref), no device
int fdnn_debug_topk_ref(const float *rows, int n, int width, int k, int32_t *nodes, float *vals) {
  if (n < 0 || width < 1) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = topk_k_check(width, k)) return rc;
  if (n == 0) return FDNN_OK;
  if (!rows || !nodes || !vals) return fail(FDNN_E_ARG, "null buffer");
  fdnn::topk::ref(reinterpret_cast<const uint32_t *>(rows), n, width, k, nodes, reinterpret_cast<uint32_t *>(vals));
  return FDNN_OK;
}

int fdnn_debug_topk_limits(int *max_k, int *resident_width) {
  if (max_k) *max_k = fdnn::topk::kTopkMaxK;
  if (resident_width) *resident_width = fdnn::topk::kTopkResidentWidth;
  return FDNN_OK;
}

// ---------------------------------------------------------------- dense output pooled over a node -> class map (fdnn_pool.hip)
fdnn_pool *fdnn_pool_create(const int32_t *class_of, int width, int n_classes) {
  const long long bad = fdnn::pool::check_map(class_of, width, n_classes);
  if (bad < 0) {
    fail(FDNN_E_ARG, "a pool is class_of [width] with 1 <= n_classes <= width <= " + std::to_string(fdnn::pool::kMaxWidth));
    return nullptr;
  }
  if (bad > 0) {
    fail(FDNN_E_ARG, "class_of[" + std::to_string(bad - 1) + "] = " + std::to_string(class_of[bad - 1]) + " is neither -1 nor a class in [0, " + std::to_string(n_classes) + ")");
    return nullptr;
  }
  std::unique_ptr<fdnn_pool> p(new (std::nothrow) fdnn_pool);
  if (!p) {
    fail(FDNN_E_NOMEM, "out of memory");
    return nullptr;
  }
  p->width = width, p->n_classes = n_classes;
  p->csr = fdnn::pool::build_csr(class_of, width, n_classes);
  const size_t words = p->csr.class_ptr.size() + p->csr.member.size();
  hipError_t e = hipGetDevice(&p->device);
  if (e == hipSuccess) e = p->d_csr.reserve(words);
  if (e == hipSuccess) e = hipMemcpy(p->d_csr.p, p->csr.class_ptr.data(), sizeof(int32_t) * p->csr.class_ptr.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess && !p->csr.member.empty())
    e = hipMemcpy(p->d_csr.p + p->csr.class_ptr.size(), p->csr.member.data(), sizeof(int32_t) * p->csr.member.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    fail(e == hipErrorOutOfMemory ? FDNN_E_NOMEM : FDNN_E_DEVICE, std::string("fdnn_pool_create: ") + hipGetErrorString(e));
    return nullptr;
  }
  return p.release();
}

void fdnn_pool_free(fdnn_pool *pool) {
  if (!pool) return;
  DeviceGuard g(pool->device);  // (the CSR is freed on the device it lives on)
  delete pool;
}

int fdnn_pool_width(const fdnn_pool *pool) { return pool ? pool->width : fail(FDNN_E_ARG, "null pool"); }
int fdnn_pool_classes(const fdnn_pool *pool) { return pool ? pool->n_classes : fail(FDNN_E_ARG, "null pool"); }

int fdnn_pool_rows_device(const fdnn_pool *pool, const float *d_rows, int n, float *d_out, void *stream) {
  if (!pool || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!d_rows || !d_out) return fail(FDNN_E_ARG, "null buffer");
  DeviceGuard g(pool->device);
  fdnn::launch_pool(d_rows, n, pool->width, pool->d_class_ptr(), pool->d_member(), pool->n_classes, d_out, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

int fdnn_ctx_output_pool_device(fdnn_ctx *c, const fdnn_pool *pool, float *d_out, void *stream) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  if (int rc = fdnn::check_pool(c->m, pool)) return rc;
  if (int rc = lazy_state(c)) return rc;
  if (c->n == 0) return FDNN_OK;
  if (!d_out) return fail(FDNN_E_ARG, "null buffer");
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  if (!c->d_out) HIP_TRY(c->d_out.reserve(size_t(c->cap) * size_t(c->m->hm.hdr.out_dim)));  // (a lean context)
  if (int rc = run_output(c, {.count = c->n, .d_out = c->d_out}, s)) return rc;
  fdnn::launch_pool(c->d_out, c->n, c->m->hm.hdr.out_dim, pool->d_class_ptr(), pool->d_member(), pool->n_classes, d_out, s);
  return FDNN_OK;
}

int fdnn_ctx_output_pool(fdnn_ctx *c, const fdnn_pool *pool, float *out) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  if (int rc = fdnn::check_pool(c->m, pool)) return rc;
  if (int rc = lazy_state(c)) return rc;
  if (c->n == 0) return FDNN_OK;
  if (!out) return fail(FDNN_E_ARG, "null buffer");
  DeviceGuard g(c->m->device);
  CtxUse use;
  HIP_TRY(use.enter(c, c->stream));
  if (!c->d_out) HIP_TRY(c->d_out.reserve(size_t(c->cap) * size_t(c->m->hm.hdr.out_dim)));  // (a lean context)
  return dense_pass(c, {.pool = pool, .pooled = out}, c->stream, /*hidden=*/false);
}

int fdnn_calculate_pool(fdnn_model *m, const float *x, int n, int dim, const fdnn_pool *pool, float *out) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = fdnn::check_pool(m, pool)) return rc;
  if (n == 0) return FDNN_OK;
  if (!x || !out) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::host_pool("fdnn_calculate_pool", x, pool, pool->n_classes, out));
}

int fdnn_calculate_pool_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_pool *pool, float *out) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  if (int rc = fdnn::splice_check(spec, raw_dim)) return rc;
  if (int rc = fdnn::check_pool(m, pool)) return rc;
  if (n == 0) return FDNN_OK;
  if (!raw || !out) return fail(FDNN_E_ARG, "null buffer");
  const std::vector<SpliceSeg> segs{SpliceSeg{0, 0, 0, n - 1}};  // (the whole utterance's raw frames travel once, as fdnn_calculate_raw's)
  return score_chunks(m, frame_chunks(n, m), Pass::raw_pool("fdnn_calculate_pool_raw", {spec.get(), &segs, raw, n}, pool, pool->n_classes, out));
}

int fdnn_calculate_pool_device(fdnn_model *m, const float *d_x, int n, const fdnn_pool *pool, float *d_out, void *stream) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = fdnn::check_pool(m, pool)) return rc;
  if (n == 0) return FDNN_OK;
  if (!d_x || !d_out) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_frames_aligned(d_x)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::device_pool("fdnn_calculate_pool_device", d_x, pool, pool->n_classes, d_out), static_cast<hipStream_t>(stream));
}

int fdnn_debug_pool_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 2, fdnn::pool_launch_counts); }

int fdnn_debug_set_pool_kernel(int mode) {
  if (mode < 0 || mode > 2) return fail(FDNN_E_ARG, "mode is 0 (the plan's rule), 1 (resident where the width allows) or 2 (streaming)");
  fdnn::pool_kernel_mode(mode);
  return FDNN_OK;
}

// The pooling in plain C++ (fdnn_pool.hpp: check_map, build_csr, ref), no device
int fdnn_debug_pool_ref(const float *rows, int n, const int32_t *class_of, int width, int n_classes, float *out) {
  if (n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (fdnn::pool::check_map(class_of, width, n_classes) != 0) return fail(FDNN_E_ARG, "class_of [width] holds -1 or a class in [0, n_classes), 1 <= n_classes <= width");
  if (n == 0) return FDNN_OK;
  if (!rows || !out) return fail(FDNN_E_ARG, "null buffer");
  const fdnn::pool::Csr csr = fdnn::pool::build_csr(class_of, width, n_classes);
  fdnn::pool::ref(reinterpret_cast<const uint32_t *>(rows), n, width, csr.class_ptr.data(), csr.member.data(), n_classes, reinterpret_cast<uint32_t *>(out));
  return FDNN_OK;
}

int fdnn_debug_pool_limits(int *lanes, int *resident_width) {
  if (lanes) *lanes = fdnn::pool::kPoolLanes;
  if (resident_width) *resident_width = fdnn::pool::kPoolResidentWidth;
  return FDNN_OK;
}

// ---------------------------------------------------------------- dense output as decoder scores (fdnn_loglik.hip)
fdnn_loglik *fdnn_loglik_create(const float *log_prior, int width, float floor, int type) {
  const long long bad = fdnn::loglik::check_handle(log_prior, width, floor, type);
  if (bad == -1) {
    fail(FDNN_E_ARG, "a score handle is log_prior [width], 1 <= width <= " + std::to_string(fdnn::loglik::kMaxWidth) + ", of type FDNN_LOGLIK_F32 or FDNN_LOGLIK_F16");
    return nullptr;
  }
  if (bad == -2) {
    fail(FDNN_E_ARG, "the floor is -inf (none) or finite, and not below -65504 for FDNN_LOGLIK_F16");
    return nullptr;
  }
  if (bad > 0) {
    fail(FDNN_E_ARG, "log_prior[" + std::to_string(bad - 1) + "] is not finite");
    return nullptr;
  }
  std::unique_ptr<fdnn_loglik> p(new (std::nothrow) fdnn_loglik);
  if (!p) {
    fail(FDNN_E_NOMEM, "out of memory");
    return nullptr;
  }
  p->width = width, p->type = type, p->floor = floor;
  p->log_prior.assign(log_prior, log_prior + width);
  hipError_t e = hipGetDevice(&p->device);
  if (e == hipSuccess) e = p->d_log_prior.reserve(size_t(width));
  if (e == hipSuccess) e = hipMemcpy(p->d_log_prior.p, log_prior, sizeof(float) * size_t(width), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    fail(e == hipErrorOutOfMemory ? FDNN_E_NOMEM : FDNN_E_DEVICE, std::string("fdnn_loglik_create: ") + hipGetErrorString(e));
    return nullptr;
  }
  return p.release();
}

void fdnn_loglik_free(fdnn_loglik *ll) {
  if (!ll) return;
  DeviceGuard g(ll->device);  // (the priors are freed on the device they live on)
  delete ll;
}

int fdnn_loglik_width(const fdnn_loglik *ll) { return ll ? ll->width : fail(FDNN_E_ARG, "null score handle"); }
int fdnn_loglik_type(const fdnn_loglik *ll) { return ll ? ll->type : fail(FDNN_E_ARG, "null score handle"); }

int fdnn_loglik_rows_device(const fdnn_loglik *ll, const float *d_rows, int n, void *d_out, void *stream) {
  if (!ll || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!d_rows || !d_out) return fail(FDNN_E_ARG, "null buffer");
  if ((reinterpret_cast<uintptr_t>(d_rows) & 3) || (reinterpret_cast<uintptr_t>(d_out) & (fdnn::loglik::elem_bytes(ll->type) - 1)))
    return fail(FDNN_E_ARG, "buffers must have their elements' alignment");
  DeviceGuard g(ll->device);
  fdnn::launch_loglik_rows(d_rows, n, ll->width, ll->d_log_prior, ll->floor, ll->type, d_out, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

int fdnn_loglik_entries_device(const fdnn_loglik *ll, const int32_t *d_nodes, const float *d_p, long long count, void *d_out, void *stream) {
  if (!ll || count < 0) return fail(FDNN_E_ARG, "bad argument");
  if (count == 0) return FDNN_OK;
  if (!d_nodes || !d_p || !d_out) return fail(FDNN_E_ARG, "null buffer");
  if (((reinterpret_cast<uintptr_t>(d_nodes) | reinterpret_cast<uintptr_t>(d_p)) & 3) || (reinterpret_cast<uintptr_t>(d_out) & (fdnn::loglik::elem_bytes(ll->type) - 1)))
    return fail(FDNN_E_ARG, "buffers must have their elements' alignment");
  DeviceGuard g(ll->device);
  fdnn::launch_loglik_entries(d_nodes, d_p, count, ll->width, ll->d_log_prior, ll->floor, ll->type, d_out, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

int fdnn_ctx_output_loglik_device(fdnn_ctx *c, const fdnn_loglik *ll, void *d_out, void *stream) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  if (int rc = fdnn::check_loglik(c->m, ll)) return rc;
  if (int rc = lazy_state(c)) return rc;
  if (c->n == 0) return FDNN_OK;
  if (!d_out) return fail(FDNN_E_ARG, "null buffer");
  DeviceGuard g(c->m->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  if (!c->d_out) HIP_TRY(c->d_out.reserve(size_t(c->cap) * size_t(c->m->hm.hdr.out_dim)));  // (a lean context)
  if (int rc = run_output(c, {.count = c->n, .d_out = c->d_out}, s)) return rc;
  fdnn::launch_loglik_rows(c->d_out, c->n, c->m->hm.hdr.out_dim, ll->d_log_prior, ll->floor, ll->type, d_out, s);
  return FDNN_OK;
}

int fdnn_ctx_output_loglik(fdnn_ctx *c, const fdnn_loglik *ll, void *out) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  if (int rc = fdnn::check_loglik(c->m, ll)) return rc;
  if (int rc = lazy_state(c)) return rc;
  if (c->n == 0) return FDNN_OK;
  if (!out) return fail(FDNN_E_ARG, "null buffer");
  DeviceGuard g(c->m->device);
  CtxUse use;
  HIP_TRY(use.enter(c, c->stream));
  if (!c->d_out) HIP_TRY(c->d_out.reserve(size_t(c->cap) * size_t(c->m->hm.hdr.out_dim)));  // (a lean context)
  return dense_pass(c, {.loglik = ll, .scores = out}, c->stream, /*hidden=*/false);
}

int fdnn_calculate_loglik(fdnn_model *m, const float *x, int n, int dim, const fdnn_loglik *ll, void *out) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = fdnn::check_loglik(m, ll)) return rc;
  if (n == 0) return FDNN_OK;
  if (!x || !out) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::host_loglik("fdnn_calculate_loglik", x, ll, fdnn::loglik::elem_bytes(ll->type), out));
}

int fdnn_calculate_loglik_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_loglik *ll, void *out) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  if (int rc = fdnn::splice_check(spec, raw_dim)) return rc;
  if (int rc = fdnn::check_loglik(m, ll)) return rc;
  if (n == 0) return FDNN_OK;
  if (!raw || !out) return fail(FDNN_E_ARG, "null buffer");
  const std::vector<SpliceSeg> segs{SpliceSeg{0, 0, 0, n - 1}};  // (the whole utterance's raw frames travel once, as fdnn_calculate_raw's)
  return score_chunks(m, frame_chunks(n, m), Pass::raw_loglik("fdnn_calculate_loglik_raw", {spec.get(), &segs, raw, n}, ll, fdnn::loglik::elem_bytes(ll->type), out));
}

int fdnn_calculate_loglik_device(fdnn_model *m, const float *d_x, int n, const fdnn_loglik *ll, void *d_out, void *stream) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (int rc = fdnn::check_loglik(m, ll)) return rc;
  if (n == 0) return FDNN_OK;
  if (!d_x || !d_out) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_frames_aligned(d_x)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::device_loglik("fdnn_calculate_loglik_device", d_x, ll, fdnn::loglik::elem_bytes(ll->type), d_out), static_cast<hipStream_t>(stream));
}

int fdnn_debug_loglik_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 3, fdnn::loglik_launch_counts); }

int fdnn_debug_set_loglik_kernel(int mode) {
  if (mode < 0 || mode > 2) return fail(FDNN_E_ARG, "mode is 0 (the plan's rule), 1 (vector where allowed) or 2 (scalar access)");
  fdnn::loglik_kernel_mode(mode);
  return FDNN_OK;
}

// The scores in plain C++ (fdnn_loglik.hpp: check_handle, ref, ref_entries, ln), no device
int fdnn_debug_loglik_ref(const float *rows, int n, const float *log_prior, int width, float floor, int type, void *out) {
  if (n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (fdnn::loglik::check_handle(log_prior, width, floor, type) != 0) return fail(FDNN_E_ARG, "log_prior [width] finite, the floor -inf or finite (F16: not below -65504), the type F32 or F16");
  if (n == 0) return FDNN_OK;
  if (!rows || !out) return fail(FDNN_E_ARG, "null buffer");
  fdnn::loglik::ref(reinterpret_cast<const uint32_t *>(rows), n, width, log_prior, floor, type, out);
  return FDNN_OK;
}

int fdnn_debug_loglik_entries_ref(const int32_t *nodes, const float *p, long long count, const float *log_prior, int width, float floor, int type, void *out) {
  if (count < 0) return fail(FDNN_E_ARG, "bad argument");
  if (fdnn::loglik::check_handle(log_prior, width, floor, type) != 0) return fail(FDNN_E_ARG, "log_prior [width] finite, the floor -inf or finite (F16: not below -65504), the type F32 or F16");
  if (count == 0) return FDNN_OK;
  if (!nodes || !p || !out) return fail(FDNN_E_ARG, "null buffer");
  fdnn::loglik::ref_entries(nodes, reinterpret_cast<const uint32_t *>(p), size_t(count), width, log_prior, floor, type, out);
  return FDNN_OK;
}

int fdnn_debug_ln_ref(const float *x, long long count, float *out) {
  if (count < 0) return fail(FDNN_E_ARG, "bad argument");
  if (count == 0) return FDNN_OK;
  if (!x || !out) return fail(FDNN_E_ARG, "null buffer");
  for (long long i = 0; i < count; ++i) out[i] = fdnn::loglik::ln(x[i]);
  return FDNN_OK;
}

// ---------------------------------------------------------------- forced alignment (fdnn_align.hip)
// The recursion alone.  The tables are host memory and are checked (the plan is made from them); what they index is on the
// device and is not: a column or node out of range gives a NaN emission, so a total that is not finite and an all -1 path.
static int align_rows_tables(const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr, int n_segs) {
  if (n_segs < 0) return fail(FDNN_E_ARG, "negative segment count");
  if (n_segs == 0) return FDNN_OK;
  if (!seg_T || !row_off || !row_ld || !state_ptr || state_ptr[0] != 0) return fail(FDNN_E_ARG, "align, segment 0: malformed tables");
  long long rows = 0;
  for (int s = 0; s < n_segs; ++s) {
    const long long S = static_cast<long long>(state_ptr[s + 1]) - state_ptr[s];
    if (seg_T[s] < 1 || row_ld[s] < 1 || row_off[s] < 0 || S < 1 || S > fdnn::align::kMaxStates || (rows += seg_T[s]) > INT32_MAX)
      return fail(FDNN_E_ARG, "align, segment " + std::to_string(s) + ": a segment has T >= 1 rows of stride >= 1 at an offset >= 0 and 1 .. " +
                                  std::to_string(fdnn::align::kMaxStates) + " states");
  }
  return FDNN_OK;
}

int fdnn_align_scratch_words(const int32_t *seg_T, const int32_t *state_ptr, int n_segs, long long *words) {
  if (!words) return fail(FDNN_E_ARG, "null argument");
  const std::vector<long long> off(size_t(std::max(n_segs, 0)), 0);
  const std::vector<int32_t> ld(size_t(std::max(n_segs, 0)), 1);
  if (int rc = align_rows_tables(seg_T, off.data(), ld.data(), state_ptr, n_segs)) return rc;
  *words = fdnn::align::plan(seg_T, off.data(), ld.data(), state_ptr, n_segs, fdnn::align_kernel_mode()).scratch_words;
  return FDNN_OK;
}

int fdnn_align_rows_device(const fdnn_loglik *ll, const float *d_rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld,
                           const int32_t *state_ptr, int n_segs, const int32_t *d_col, const int32_t *d_state_node, const float *d_self_lp,
                           const float *d_next_lp, void *d_scratch, long long scratch_words, int32_t *d_path, float *d_total, void *stream) {
  if (int rc = align_rows_tables(seg_T, row_off, row_ld, state_ptr, n_segs)) return rc;
  if (n_segs == 0) return FDNN_OK;
  if (!d_rows || !d_col || !d_path || !d_total || (ll && !d_state_node)) return fail(FDNN_E_ARG, "null buffer");
  const uintptr_t all = reinterpret_cast<uintptr_t>(d_rows) | reinterpret_cast<uintptr_t>(d_col) | reinterpret_cast<uintptr_t>(d_state_node) |
                        reinterpret_cast<uintptr_t>(d_self_lp) | reinterpret_cast<uintptr_t>(d_next_lp) | reinterpret_cast<uintptr_t>(d_path) |
                        reinterpret_cast<uintptr_t>(d_total);
  if ((all & 3) || (reinterpret_cast<uintptr_t>(d_scratch) & 7)) return fail(FDNN_E_ARG, "buffers must have their elements' alignment, the scratch 8 bytes");
  const fdnn::align::Plan p = fdnn::align::plan(seg_T, row_off, row_ld, state_ptr, n_segs, fdnn::align_kernel_mode());
  if (p.scratch_words * 4 > fdnn::align::kMaxScratchBytes)
    return fail(FDNN_E_ARG, "align: the back-pointer words of the call are above " + std::to_string(fdnn::align::kMaxScratchBytes) + " bytes");
  if (p.scratch_words > 0 && (!d_scratch || scratch_words < p.scratch_words))
    return fail(FDNN_E_ARG, "align: the call needs " + std::to_string(p.scratch_words) + " scratch words (fdnn_align_scratch_words)");
  fdnn::AlignArgs a;
  a.d_rows = d_rows, a.d_col = d_col, a.d_state_node = d_state_node, a.d_self_lp = d_self_lp, a.d_next_lp = d_next_lp;
  a.d_scratch = static_cast<uint32_t *>(d_scratch), a.d_path = d_path, a.d_total = d_total;
  if (ll) a.d_log_prior = ll->d_log_prior, a.width = ll->width, a.floor = ll->floor, a.type = ll->type;
  int dev = 0;
  if (ll) dev = ll->device;
  else if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  DeviceGuard g(dev);
  fdnn::launch_align(p, a, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

// The front of every align call through a model: the handle, then the tables (align_prepare names the first bad segment)
static int align_front(const fdnn_model *m, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                       const float *self_lp, const float *next_lp, int ctx_rows, fdnn::AlignJob *j) {
  if (int rc = fdnn::check_loglik(m, ll)) return rc;
  if (n_segs < 0) return fail(FDNN_E_ARG, "negative segment count");
  j->ll = ll, j->seg_rows = seg_rows, j->state_ptr = state_ptr, j->states = states, j->self_lp = self_lp, j->next_lp = next_lp, j->n_segs = n_segs;
  return fdnn::align_prepare(j, m->hm.hdr.out_dim, ctx_rows);
}

static int ctx_align(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                     const float *self_lp, const float *next_lp, int32_t *path, float *total, bool host, hipStream_t s) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  fdnn::AlignJob j;
  if (int rc = align_front(c->m, ll, seg_rows, state_ptr, n_segs, states, self_lp, next_lp, c->n, &j)) return rc;
  if (int rc = lazy_state(c)) return rc;
  if (n_segs == 0) return FDNN_OK;
  if (!path || !total) return fail(FDNN_E_ARG, "null result buffer");
  const std::vector<sets::Seg> segs = sets::slice(j.tables(), seg_rows[0], seg_rows[n_segs]);
  DeviceGuard g(c->m->device);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  int rc = fdnn::align_stage(c, j, s);
  SetsCall sc;
  sc.first = seg_rows[0], sc.segs = &segs, sc.d_nodes = c->d_al_int, sc.d_probs = c->d_al_probs, sc.d_inactive = c->d_al_inact;
  if (!rc) rc = run_sets(c, sc, s);
  if (!rc) rc = fdnn::align_finish(c, j, path, total, host, s);
  if (rc && host) hipStreamSynchronize(s);
  return rc;
}

int fdnn_ctx_align(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                   const float *self_lp, const float *next_lp, int32_t *path, float *total) {
  return ctx_align(c, ll, seg_rows, state_ptr, n_segs, states, self_lp, next_lp, path, total, true, c ? c->stream : nullptr);
}

int fdnn_ctx_align_device(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                          const float *self_lp, const float *next_lp, int32_t *d_path, float *d_total, void *stream) {
  return ctx_align(c, ll, seg_rows, state_ptr, n_segs, states, self_lp, next_lp, d_path, d_total, false, static_cast<hipStream_t>(stream));
}

// One-call forms: hidden layers + the transcripts' sets chunk by chunk into the context's buffers (a segment cut by a chunk
// keeps its set), the recursion ONCE behind the last chunk, inside the same use of the context.
static int calculate_align(fdnn_model *m, const Pass &p, fdnn::AlignJob &j, int32_t *path, float *total, int n) {
  return score_chunks(m, frame_chunks(n, m), p, nullptr, [&](fdnn_ctx *c, hipStream_t s) { return fdnn::align_stage(c, j, s); },
                      [&](fdnn_ctx *c, hipStream_t s) {
                        const int rc = fdnn::align_finish(c, j, path, total, true, s);
                        if (rc) hipStreamSynchronize(s);
                        return rc;
                      });
}

int fdnn_calculate_align(fdnn_model *m, const float *x, int n, int dim, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr,
                         int n_segs, const int32_t *states, const float *self_lp, const float *next_lp, int32_t *path, float *total) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  fdnn::AlignJob j;
  if (int rc = align_front(m, ll, seg_rows, state_ptr, n_segs, states, self_lp, next_lp, n, &j)) return rc;
  if (n_segs == 0 ? n != 0 : (seg_rows[0] != 0 || seg_rows[n_segs] != n)) return fail(FDNN_E_ARG, "seg_rows must cover the rows [0, n)");
  if (n == 0) return FDNN_OK;
  if (!x || !path || !total) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  const sets::Tables t = j.tables();
  return calculate_align(m, Pass::host_align("fdnn_calculate_align", x, t), j, path, total, n);
}

int fdnn_calculate_align_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_loglik *ll, const int32_t *seg_rows,
                             const int32_t *state_ptr, int n_segs, const int32_t *states, const float *self_lp, const float *next_lp, int32_t *path,
                             float *total) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  if (int rc = fdnn::splice_check(spec, raw_dim)) return rc;
  fdnn::AlignJob j;
  if (int rc = align_front(m, ll, seg_rows, state_ptr, n_segs, states, self_lp, next_lp, n, &j)) return rc;
  if (n_segs == 0 ? n != 0 : (seg_rows[0] != 0 || seg_rows[n_segs] != n)) return fail(FDNN_E_ARG, "seg_rows must cover the rows [0, n)");
  if (n == 0) return FDNN_OK;
  if (!raw || !path || !total) return fail(FDNN_E_ARG, "null buffer");
  // every segment is an utterance of its own: its edges repeat its own first and last frame
  std::vector<SpliceSeg> segs;
  for (int s = 0; s < n_segs; ++s) segs.push_back(SpliceSeg{seg_rows[s], seg_rows[s], seg_rows[s], seg_rows[s + 1] - 1});
  const sets::Tables t = j.tables();
  return calculate_align(m, Pass::raw_align("fdnn_calculate_align_raw", {spec.get(), &segs, raw, n}, t), j, path, total, n);
}

int fdnn_debug_align_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 2, fdnn::align_launch_counts); }

int fdnn_debug_set_align_kernel(int mode) {
  if (mode < 0 || mode > 2) return fail(FDNN_E_ARG, "mode is 0 (the plan's rule), 1 (the wave form where allowed) or 2 (the workgroup form)");
  fdnn::align_kernel_mode(mode);
  return FDNN_OK;
}

int fdnn_debug_align_limits(int *out, int cap) {
  if (!out || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  const int v[6] = {fdnn::align::kMaxStates, fdnn::align::kMaxSegs, fdnn::align::kWaveStates, fdnn::align::kFramesInFlight, fdnn::align::kBpLdsWords,
                    int(fdnn::align::kMaxScratchBytes >> 20)};
  for (int i = 0; i < 6 && i < cap; ++i) out[i] = v[i];
  return 6;
}

// The recursion in plain C++ (fdnn_align.hpp: ref), no device: segment s = rows [T_s] of stride row_ld[s] at row_off[s].
// type: FDNN_LOGLIK_F32 / _F16 with log_prior [width], floor and state_node, or -1: the rows are scores.
int fdnn_debug_align_ref(const float *rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr, int n_segs,
                         const int32_t *col, const int32_t *state_node, const float *log_prior, int width, float floor, int type, const float *self_lp,
                         const float *next_lp, int32_t *path, float *total) {
  if (int rc = align_rows_tables(seg_T, row_off, row_ld, state_ptr, n_segs)) return rc;
  if (n_segs == 0) return FDNN_OK;
  if (type != fdnn::align::kScores && (fdnn::loglik::check_handle(log_prior, width, floor, type) != 0 || !state_node))
    return fail(FDNN_E_ARG, "log_prior [width] finite, the floor -inf or finite (F16: not below -65504), the type F32, F16 or -1 (scores)");
  if (!rows || !col || !path || !total) return fail(FDNN_E_ARG, "null buffer");
  size_t at = 0;
  for (int s = 0; s < n_segs; ++s) {
    const int b = state_ptr[s], S = state_ptr[s + 1] - b;
    uint32_t tb;
    fdnn::align::ref(reinterpret_cast<const uint32_t *>(rows) + row_off[s], seg_T[s], row_ld[s], col + b, state_node ? state_node + b : nullptr, S, log_prior,
                     width, floor, type, self_lp ? self_lp + b : nullptr, next_lp ? next_lp + b : nullptr, path + at, &tb);
    std::memcpy(total + s, &tb, 4);
    at += size_t(seg_T[s]);
  }
  return FDNN_OK;
}

int fdnn_debug_align_sets(const int32_t *state_ptr, const int32_t *states, int n_segs, int32_t *set_ptr, int32_t *nodes, int32_t *col) {
  if (n_segs < 0 || !state_ptr || !set_ptr || state_ptr[0] != 0) return fail(FDNN_E_ARG, "bad argument");
  for (int s = 0; s < n_segs; ++s)
    if (state_ptr[s + 1] < state_ptr[s]) return fail(FDNN_E_ARG, "state_ptr must not decrease");
  if (n_segs && state_ptr[n_segs] > 0 && (!states || !nodes || !col)) return fail(FDNN_E_ARG, "null buffer");
  const fdnn::align::Sets st = fdnn::align::build_sets(state_ptr, states, n_segs);
  std::copy(st.set_ptr.begin(), st.set_ptr.end(), set_ptr);
  std::copy(st.nodes.begin(), st.nodes.end(), nodes);  // (nodes holds state_ptr[n_segs] entries: a set is no longer than its transcript)
  std::copy(st.col.begin(), st.col.end(), col);
  return FDNN_OK;
}

// ---------------------------------------------------------------- alignment graphs (fdnn_align_graph.hip)
// The recursion alone.  The tables are host memory and are checked (the plan is made from them, and its arc counts bound
// every arc index on the device); what they index is on the device and is not: a source, column or node out of range gives a
// NaN, which is never taken.
static int align_graph_rows_tables(const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr, const int32_t *arc_ptr,
                                   int n_segs) {
  if (int rc = align_rows_tables(seg_T, row_off, row_ld, state_ptr, n_segs)) return rc;
  if (n_segs == 0 || !arc_ptr) return FDNN_OK;  // (fdnn_align_graph_scratch_words: the scratch does not depend on the arcs)
  if (arc_ptr[0] != 0) return fail(FDNN_E_ARG, "align graph, segment 0: arc_ptr begins at 0");
  for (int s = 0; s < n_segs; ++s) {
    for (int i = state_ptr[s]; i < state_ptr[s + 1]; ++i)
      if (arc_ptr[i + 1] < arc_ptr[i]) return fail(FDNN_E_ARG, "align graph, segment " + std::to_string(s) + ": arc_ptr must not decrease");
    if (arc_ptr[state_ptr[s + 1]] - arc_ptr[state_ptr[s]] > fdnn::align_graph::kMaxArcs)
      return fail(FDNN_E_ARG, "align graph, segment " + std::to_string(s) + ": a segment has at most " + std::to_string(fdnn::align_graph::kMaxArcs) + " arcs");
  }
  return FDNN_OK;
}

int fdnn_align_graph_scratch_words(const int32_t *seg_T, const int32_t *state_ptr, int n_segs, long long *words) {
  if (!words) return fail(FDNN_E_ARG, "null argument");
  const std::vector<long long> off(size_t(std::max(n_segs, 0)), 0);
  const std::vector<int32_t> ld(size_t(std::max(n_segs, 0)), 1);
  if (int rc = align_graph_rows_tables(seg_T, off.data(), ld.data(), state_ptr, nullptr, n_segs)) return rc;
  *words = fdnn::align_graph::plan(seg_T, off.data(), ld.data(), state_ptr, nullptr, n_segs, fdnn::align_graph_kernel_mode()).scratch_words;
  return FDNN_OK;
}

int fdnn_align_graph_rows_device(const fdnn_loglik *ll, const float *d_rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld,
                                 const int32_t *state_ptr, const int32_t *arc_ptr, int n_segs, const int32_t *d_col, const int32_t *d_state_node,
                                 const int32_t *d_arc_ptr, const int32_t *d_arc_src, const float *d_arc_lp, const float *d_start_lp,
                                 const float *d_final_lp, void *d_scratch, long long scratch_words, int32_t *d_path, float *d_total, void *stream) {
  if (n_segs > 0 && !arc_ptr) return fail(FDNN_E_ARG, "align graph, segment 0: malformed tables");
  if (int rc = align_graph_rows_tables(seg_T, row_off, row_ld, state_ptr, arc_ptr, n_segs)) return rc;
  if (n_segs == 0) return FDNN_OK;
  const bool arcs = arc_ptr[state_ptr[n_segs]] > 0;
  if (!d_rows || !d_col || !d_arc_ptr || (arcs && (!d_arc_src || !d_arc_lp)) || !d_path || !d_total || (ll && !d_state_node))
    return fail(FDNN_E_ARG, "null buffer");
  const uintptr_t all = reinterpret_cast<uintptr_t>(d_rows) | reinterpret_cast<uintptr_t>(d_col) | reinterpret_cast<uintptr_t>(d_state_node) |
                        reinterpret_cast<uintptr_t>(d_arc_ptr) | reinterpret_cast<uintptr_t>(d_arc_src) | reinterpret_cast<uintptr_t>(d_arc_lp) |
                        reinterpret_cast<uintptr_t>(d_start_lp) | reinterpret_cast<uintptr_t>(d_final_lp) | reinterpret_cast<uintptr_t>(d_scratch) |
                        reinterpret_cast<uintptr_t>(d_path) | reinterpret_cast<uintptr_t>(d_total);
  if (all & 3) return fail(FDNN_E_ARG, "buffers must have their elements' alignment, the scratch 4 bytes");
  const fdnn::align_graph::Plan p = fdnn::align_graph::plan(seg_T, row_off, row_ld, state_ptr, arc_ptr, n_segs, fdnn::align_graph_kernel_mode());
  if (p.scratch_words * 4 > fdnn::align_graph::kMaxScratchBytes)
    return fail(FDNN_E_ARG, "align graph: the back-pointers of the call are above " + std::to_string(fdnn::align_graph::kMaxScratchBytes) + " bytes");
  if (p.scratch_words > 0 && (!d_scratch || scratch_words < p.scratch_words))
    return fail(FDNN_E_ARG, "align graph: the call needs " + std::to_string(p.scratch_words) + " scratch words (fdnn_align_graph_scratch_words)");
  fdnn::AlignGraphArgs a;
  a.d_rows = d_rows, a.d_col = d_col, a.d_state_node = d_state_node, a.d_arc_ptr = d_arc_ptr, a.d_arc_src = d_arc_src, a.d_arc_lp = d_arc_lp;
  a.d_start_lp = d_start_lp, a.d_final_lp = d_final_lp;
  a.d_scratch = static_cast<uint32_t *>(d_scratch), a.d_path = d_path, a.d_total = d_total;
  if (ll) a.d_log_prior = ll->d_log_prior, a.width = ll->width, a.floor = ll->floor, a.type = ll->type;
  int dev = 0;
  if (ll) dev = ll->device;
  else if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  DeviceGuard g(dev);
  fdnn::launch_align_graph(p, a, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

// The front of every align-graph call through a model: the handle, then the tables (align_graph_prepare names the first bad segment)
static int align_graph_front(const fdnn_model *m, const fdnn_loglik *ll, const fdnn::align_graph::Tables &t, int ctx_rows, fdnn::AlignGraphJob *j) {
  if (int rc = fdnn::check_loglik(m, ll)) return rc;
  if (t.n_segs < 0) return fail(FDNN_E_ARG, "negative segment count");
  j->ll = ll, j->t = t;
  return fdnn::align_graph_prepare(j, m->hm.hdr.out_dim, ctx_rows);
}

static fdnn::align_graph::Tables graph_tables(const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states, const int32_t *arc_ptr,
                                              const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp) {
  fdnn::align_graph::Tables t;
  t.seg_rows = seg_rows, t.state_ptr = state_ptr, t.states = states, t.arc_ptr = arc_ptr, t.arc_src = arc_src, t.arc_lp = arc_lp;
  t.start_lp = start_lp, t.final_lp = final_lp, t.n_segs = n_segs;
  return t;
}

static int ctx_align_graph(fdnn_ctx *c, const fdnn_loglik *ll, const fdnn::align_graph::Tables &t, int32_t *path, float *total, bool host, hipStream_t s) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  fdnn::AlignGraphJob j;
  if (int rc = align_graph_front(c->m, ll, t, c->n, &j)) return rc;
  if (int rc = lazy_state(c)) return rc;
  if (t.n_segs == 0) return FDNN_OK;
  if (!path || !total) return fail(FDNN_E_ARG, "null result buffer");
  const std::vector<sets::Seg> segs = sets::slice(j.tables(), t.seg_rows[0], t.seg_rows[t.n_segs]);
  DeviceGuard g(c->m->device);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  int rc = fdnn::align_graph_stage(c, j, s);
  SetsCall sc;
  sc.first = t.seg_rows[0], sc.segs = &segs, sc.d_nodes = c->d_al_int, sc.d_probs = c->d_al_probs, sc.d_inactive = c->d_al_inact;
  if (!rc) rc = run_sets(c, sc, s);
  if (!rc) rc = fdnn::align_graph_finish(c, j, path, total, host, s);
  if (rc && host) hipStreamSynchronize(s);
  return rc;
}

int fdnn_ctx_align_graph(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                         const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp, int32_t *path,
                         float *total) {
  return ctx_align_graph(c, ll, graph_tables(seg_rows, state_ptr, n_segs, states, arc_ptr, arc_src, arc_lp, start_lp, final_lp), path, total, true,
                         c ? c->stream : nullptr);
}

int fdnn_ctx_align_graph_device(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                                const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp,
                                int32_t *d_path, float *d_total, void *stream) {
  return ctx_align_graph(c, ll, graph_tables(seg_rows, state_ptr, n_segs, states, arc_ptr, arc_src, arc_lp, start_lp, final_lp), d_path, d_total, false,
                         static_cast<hipStream_t>(stream));
}

// One-call forms: hidden layers + the graphs' node sets chunk by chunk into the context's buffers (the sibling's sink), the
// recursion ONCE behind the last chunk, inside the same use of the context.
static int calculate_align_graph(fdnn_model *m, const Pass &p, fdnn::AlignGraphJob &j, int32_t *path, float *total, int n) {
  return score_chunks(m, frame_chunks(n, m), p, nullptr, [&](fdnn_ctx *c, hipStream_t s) { return fdnn::align_graph_stage(c, j, s); },
                      [&](fdnn_ctx *c, hipStream_t s) {
                        const int rc = fdnn::align_graph_finish(c, j, path, total, true, s);
                        if (rc) hipStreamSynchronize(s);
                        return rc;
                      });
}

int fdnn_calculate_align_graph(fdnn_model *m, const float *x, int n, int dim, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr,
                               int n_segs, const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp,
                               const float *start_lp, const float *final_lp, int32_t *path, float *total) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  fdnn::AlignGraphJob j;
  if (int rc = align_graph_front(m, ll, graph_tables(seg_rows, state_ptr, n_segs, states, arc_ptr, arc_src, arc_lp, start_lp, final_lp), n, &j)) return rc;
  if (n_segs == 0 ? n != 0 : (seg_rows[0] != 0 || seg_rows[n_segs] != n)) return fail(FDNN_E_ARG, "seg_rows must cover the rows [0, n)");
  if (n == 0) return FDNN_OK;
  if (!x || !path || !total) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  const sets::Tables t = j.tables();
  return calculate_align_graph(m, Pass::host_align("fdnn_calculate_align_graph", x, t), j, path, total, n);
}

int fdnn_calculate_align_graph_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_loglik *ll, const int32_t *seg_rows,
                                   const int32_t *state_ptr, int n_segs, const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src,
                                   const float *arc_lp, const float *start_lp, const float *final_lp, int32_t *path, float *total) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  if (int rc = fdnn::splice_check(spec, raw_dim)) return rc;
  fdnn::AlignGraphJob j;
  if (int rc = align_graph_front(m, ll, graph_tables(seg_rows, state_ptr, n_segs, states, arc_ptr, arc_src, arc_lp, start_lp, final_lp), n, &j)) return rc;
  if (n_segs == 0 ? n != 0 : (seg_rows[0] != 0 || seg_rows[n_segs] != n)) return fail(FDNN_E_ARG, "seg_rows must cover the rows [0, n)");
  if (n == 0) return FDNN_OK;
  if (!raw || !path || !total) return fail(FDNN_E_ARG, "null buffer");
  // every segment is an utterance of its own: its edges repeat its own first and last frame
  std::vector<SpliceSeg> segs;
  for (int s = 0; s < n_segs; ++s) segs.push_back(SpliceSeg{seg_rows[s], seg_rows[s], seg_rows[s], seg_rows[s + 1] - 1});
  const sets::Tables t = j.tables();
  return calculate_align_graph(m, Pass::raw_align("fdnn_calculate_align_graph_raw", {spec.get(), &segs, raw, n}, t), j, path, total, n);
}

int fdnn_debug_align_graph_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 2, fdnn::align_graph_launch_counts); }

int fdnn_debug_set_align_graph_kernel(int mode) {
  if (mode < 0 || mode > 2) return fail(FDNN_E_ARG, "mode is 0 (the plan's rule), 1 (the wave form where allowed) or 2 (the workgroup form)");
  fdnn::align_graph_kernel_mode(mode);
  return FDNN_OK;
}

int fdnn_debug_align_graph_limits(int *out, int cap) {
  if (!out || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  const int v[8] = {fdnn::align_graph::kMaxStates, fdnn::align_graph::kMaxSegs, fdnn::align_graph::kWaveStates, fdnn::align_graph::kMaxArcs,
                    fdnn::align_graph::kArcLdsArcs, fdnn::align_graph::kBpLdsWords, int(fdnn::align_graph::kMaxScratchBytes >> 20),
                    fdnn::align_graph::kWaveRuleStates};
  for (int i = 0; i < 8 && i < cap; ++i) out[i] = v[i];
  return 8;
}

// The recursion in plain C++ (fdnn_align_graph.hpp: ref), no device: rows, tables and handle values as fdnn_debug_align_ref,
// the graph's tables as fdnn_align_graph_rows_device takes them, all on the host.
int fdnn_debug_align_graph_ref(const float *rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr,
                               int n_segs, const int32_t *col, const int32_t *state_node, const float *log_prior, int width, float floor, int type,
                               const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp,
                               int32_t *path, float *total) {
  if (n_segs > 0 && !arc_ptr) return fail(FDNN_E_ARG, "align graph, segment 0: malformed tables");
  if (int rc = align_graph_rows_tables(seg_T, row_off, row_ld, state_ptr, arc_ptr, n_segs)) return rc;
  if (n_segs == 0) return FDNN_OK;
  if (type != fdnn::align::kScores && (fdnn::loglik::check_handle(log_prior, width, floor, type) != 0 || !state_node))
    return fail(FDNN_E_ARG, "log_prior [width] finite, the floor -inf or finite (F16: not below -65504), the type F32, F16 or -1 (scores)");
  if (!rows || !col || !path || !total || (arc_ptr[state_ptr[n_segs]] > 0 && (!arc_src || !arc_lp))) return fail(FDNN_E_ARG, "null buffer");
  size_t at = 0;
  for (int s = 0; s < n_segs; ++s) {
    const int b = state_ptr[s], S = state_ptr[s + 1] - b;
    uint32_t tb;
    fdnn::align_graph::ref(reinterpret_cast<const uint32_t *>(rows) + row_off[s], seg_T[s], row_ld[s], col + b, state_node ? state_node + b : nullptr, S,
                           log_prior, width, floor, type, arc_ptr + b, arc_src, arc_lp, start_lp ? start_lp + b : nullptr,
                           final_lp ? final_lp + b : nullptr, path + at, &tb);
    std::memcpy(total + s, &tb, 4);
    at += size_t(seg_T[s]);
  }
  return FDNN_OK;
}

// ---------------------------------------------------------------- alignment graphs, summed (fdnn_fb.hip)
// The sweeps alone.  The host tables are checked as the sibling's (the plan is made from them, and its arc counts bound every
// arc index on the device, either direction); what they index is on the device and is not.
static int fb_t_ptr_ok(const int32_t *state_ptr, const int32_t *arc_ptr, const int32_t *t_ptr, int n_segs) {
  if (t_ptr[0] != 0) return fail(FDNN_E_ARG, "forward-backward, segment 0: t_ptr begins at 0");
  for (int s = 0; s < n_segs; ++s) {
    for (int i = state_ptr[s]; i < state_ptr[s + 1]; ++i)
      if (t_ptr[i + 1] < t_ptr[i]) return fail(FDNN_E_ARG, "forward-backward, segment " + std::to_string(s) + ": t_ptr must not decrease");
    if (t_ptr[state_ptr[s]] != arc_ptr[state_ptr[s]] || t_ptr[state_ptr[s + 1]] != arc_ptr[state_ptr[s + 1]])
      return fail(FDNN_E_ARG, "forward-backward, segment " + std::to_string(s) + ": a segment's transposed arcs occupy the range of its arcs");
  }
  return FDNN_OK;
}

int fdnn_fb_scratch_words(const int32_t *seg_T, const int32_t *state_ptr, int n_segs, int want_gamma, long long *words) {
  if (!words) return fail(FDNN_E_ARG, "null argument");
  const std::vector<long long> off(size_t(std::max(n_segs, 0)), 0);
  const std::vector<int32_t> ld(size_t(std::max(n_segs, 0)), 1);
  if (int rc = align_graph_rows_tables(seg_T, off.data(), ld.data(), state_ptr, nullptr, n_segs)) return rc;
  const long long w = fdnn::fb::plan(seg_T, off.data(), ld.data(), state_ptr, nullptr, n_segs, want_gamma != 0, fdnn::fb_kernel_mode()).scratch_words;
  if (w * 4 > fdnn::fb::kMaxScratchBytes)
    return fail(FDNN_E_ARG, "forward-backward: the lattice of the call is above " + std::to_string(fdnn::fb::kMaxScratchBytes) + " bytes");
  *words = w;
  return FDNN_OK;
}

int fdnn_fb_transpose(const int32_t *state_ptr, int n_segs, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, int32_t *t_ptr,
                      int32_t *t_src, float *t_lp) {
  if (n_segs < 0 || !state_ptr || !arc_ptr || !t_ptr || state_ptr[0] != 0 || arc_ptr[0] != 0) return fail(FDNN_E_ARG, "bad argument");
  for (int s = 0; s < n_segs; ++s)
    if (state_ptr[s + 1] < state_ptr[s]) return fail(FDNN_E_ARG, "state_ptr must not decrease");
  t_ptr[0] = 0;
  if (n_segs == 0) return FDNN_OK;
  for (int i = 0; i < state_ptr[n_segs]; ++i)
    if (arc_ptr[i + 1] < arc_ptr[i]) return fail(FDNN_E_ARG, "arc_ptr must not decrease");
  if (arc_ptr[state_ptr[n_segs]] > 0 && (!arc_src || !arc_lp || !t_src || !t_lp)) return fail(FDNN_E_ARG, "null buffer");
  const int bad = fdnn::fb::transpose(state_ptr, n_segs, arc_ptr, arc_src, arc_lp, t_ptr, t_src, t_lp);
  if (bad) return fail(FDNN_E_ARG, "forward-backward, segment " + std::to_string(-bad - 1) + ": an arc's source is outside [0, S)");
  return FDNN_OK;
}

int fdnn_fb_rows_device(const fdnn_loglik *ll, const float *d_rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld,
                        const int32_t *state_ptr, const int32_t *arc_ptr, const int32_t *t_ptr, int n_segs, const int32_t *d_col,
                        const int32_t *d_state_node, const int32_t *d_arc_ptr, const int32_t *d_arc_src, const float *d_arc_lp, const float *d_start_lp,
                        const float *d_final_lp, const int32_t *d_t_ptr, const int32_t *d_t_src, const float *d_t_lp, void *d_scratch,
                        long long scratch_words, float *d_total, float *d_gamma, void *stream) {
  if (n_segs > 0 && !arc_ptr) return fail(FDNN_E_ARG, "forward-backward, segment 0: malformed tables");
  if (int rc = align_graph_rows_tables(seg_T, row_off, row_ld, state_ptr, arc_ptr, n_segs)) return rc;
  if (n_segs == 0) return FDNN_OK;
  const bool arcs = arc_ptr[state_ptr[n_segs]] > 0, want = d_gamma != nullptr;
  if (want) {
    if (!t_ptr) return fail(FDNN_E_ARG, "forward-backward: gamma needs the transposed tables (fdnn_fb_transpose)");
    if (int rc = fb_t_ptr_ok(state_ptr, arc_ptr, t_ptr, n_segs)) return rc;
  }
  if (!d_rows || !d_col || !d_arc_ptr || (arcs && (!d_arc_src || !d_arc_lp)) || !d_total || (ll && !d_state_node) ||
      (want && (!d_t_ptr || (arcs && (!d_t_src || !d_t_lp)))))
    return fail(FDNN_E_ARG, "null buffer");
  const uintptr_t all = reinterpret_cast<uintptr_t>(d_rows) | reinterpret_cast<uintptr_t>(d_col) | reinterpret_cast<uintptr_t>(d_state_node) |
                        reinterpret_cast<uintptr_t>(d_arc_ptr) | reinterpret_cast<uintptr_t>(d_arc_src) | reinterpret_cast<uintptr_t>(d_arc_lp) |
                        reinterpret_cast<uintptr_t>(d_start_lp) | reinterpret_cast<uintptr_t>(d_final_lp) | reinterpret_cast<uintptr_t>(d_t_ptr) |
                        reinterpret_cast<uintptr_t>(d_t_src) | reinterpret_cast<uintptr_t>(d_t_lp) | reinterpret_cast<uintptr_t>(d_scratch) |
                        reinterpret_cast<uintptr_t>(d_total) | reinterpret_cast<uintptr_t>(d_gamma);
  if (all & 3) return fail(FDNN_E_ARG, "buffers must have their elements' alignment, the scratch 4 bytes");
  fdnn::fb::Plan p = fdnn::fb::plan(seg_T, row_off, row_ld, state_ptr, arc_ptr, n_segs, want, fdnn::fb_kernel_mode());
  if (p.scratch_words * 4 > fdnn::fb::kMaxScratchBytes)
    return fail(FDNN_E_ARG, "forward-backward: the lattice of the call is above " + std::to_string(fdnn::fb::kMaxScratchBytes) + " bytes");
  if (p.scratch_words > 0 && (!d_scratch || scratch_words < p.scratch_words))
    return fail(FDNN_E_ARG, "forward-backward: the call needs " + std::to_string(p.scratch_words) + " scratch words (fdnn_fb_scratch_words)");
  fdnn::FbArgs a;
  a.d_rows = d_rows, a.d_col = d_col, a.d_state_node = d_state_node, a.d_arc_ptr = d_arc_ptr, a.d_arc_src = d_arc_src, a.d_arc_lp = d_arc_lp;
  a.d_start_lp = d_start_lp, a.d_final_lp = d_final_lp, a.d_t_ptr = d_t_ptr, a.d_t_src = d_t_src, a.d_t_lp = d_t_lp;
  a.d_scratch = static_cast<float *>(d_scratch), a.d_total = d_total, a.d_gamma = d_gamma;
  if (ll) a.d_log_prior = ll->d_log_prior, a.width = ll->width, a.floor = ll->floor, a.type = ll->type;
  int dev = 0;
  if (ll) dev = ll->device;
  else if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  DeviceGuard g(dev);
  fdnn::launch_fb(p, a, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

// The front of every forward-backward call through a model: the handle, then the tables (fb_prepare names the first bad segment)
static int fb_front(const fdnn_model *m, const fdnn_loglik *ll, const fdnn::align_graph::Tables &t, bool want_gamma, int ctx_rows, fdnn::FbJob *j) {
  if (int rc = fdnn::check_loglik(m, ll)) return rc;
  if (t.n_segs < 0) return fail(FDNN_E_ARG, "negative segment count");
  j->ll = ll, j->t = t, j->want_gamma = want_gamma;
  return fdnn::fb_prepare(j, m->hm.hdr.out_dim, ctx_rows);
}

static int ctx_fb(fdnn_ctx *c, const fdnn_loglik *ll, const fdnn::align_graph::Tables &t, float *total, float *gamma, bool host, hipStream_t s) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  fdnn::FbJob j;
  if (int rc = fb_front(c->m, ll, t, gamma != nullptr, c->n, &j)) return rc;
  if (int rc = lazy_state(c)) return rc;
  if (t.n_segs == 0) return FDNN_OK;
  if (!total) return fail(FDNN_E_ARG, "null result buffer");
  const std::vector<sets::Seg> segs = sets::slice(j.tables(), t.seg_rows[0], t.seg_rows[t.n_segs]);
  DeviceGuard g(c->m->device);
  CtxUse use;
  HIP_TRY(use.enter(c, s));
  int rc = fdnn::fb_stage(c, j, s);
  SetsCall sc;
  sc.first = t.seg_rows[0], sc.segs = &segs, sc.d_nodes = c->d_al_int, sc.d_probs = c->d_al_probs, sc.d_inactive = c->d_al_inact;
  if (!rc) rc = run_sets(c, sc, s);
  if (!rc) rc = fdnn::fb_finish(c, j, total, gamma, host, s);
  if (rc && host) hipStreamSynchronize(s);
  return rc;
}

int fdnn_ctx_fb(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp, float *total,
                float *gamma) {
  return ctx_fb(c, ll, graph_tables(seg_rows, state_ptr, n_segs, states, arc_ptr, arc_src, arc_lp, start_lp, final_lp), total, gamma, true,
                c ? c->stream : nullptr);
}

int fdnn_ctx_fb_device(fdnn_ctx *c, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs, const int32_t *states,
                       const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp, float *d_total,
                       float *d_gamma, void *stream) {
  return ctx_fb(c, ll, graph_tables(seg_rows, state_ptr, n_segs, states, arc_ptr, arc_src, arc_lp, start_lp, final_lp), d_total, d_gamma, false,
                static_cast<hipStream_t>(stream));
}

// One-call forms: hidden layers + the graphs' node sets chunk by chunk into the context's buffers (the sibling's sink), the
// sweeps ONCE behind the last chunk, inside the same use of the context.
static int calculate_fb(fdnn_model *m, const Pass &p, fdnn::FbJob &j, float *total, float *gamma, int n) {
  return score_chunks(m, frame_chunks(n, m), p, nullptr, [&](fdnn_ctx *c, hipStream_t s) { return fdnn::fb_stage(c, j, s); },
                      [&](fdnn_ctx *c, hipStream_t s) {
                        const int rc = fdnn::fb_finish(c, j, total, gamma, true, s);
                        if (rc) hipStreamSynchronize(s);
                        return rc;
                      });
}

int fdnn_calculate_fb(fdnn_model *m, const float *x, int n, int dim, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr, int n_segs,
                      const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp,
                      const float *final_lp, float *total, float *gamma) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  fdnn::FbJob j;
  if (int rc = fb_front(m, ll, graph_tables(seg_rows, state_ptr, n_segs, states, arc_ptr, arc_src, arc_lp, start_lp, final_lp), gamma != nullptr, n, &j))
    return rc;
  if (n_segs == 0 ? n != 0 : (seg_rows[0] != 0 || seg_rows[n_segs] != n)) return fail(FDNN_E_ARG, "seg_rows must cover the rows [0, n)");
  if (n == 0) return FDNN_OK;
  if (!x || !total) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  const sets::Tables t = j.tables();
  return calculate_fb(m, Pass::host_align("fdnn_calculate_fb", x, t), j, total, gamma, n);
}

int fdnn_calculate_fb_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const fdnn_loglik *ll, const int32_t *seg_rows, const int32_t *state_ptr,
                          int n_segs, const int32_t *states, const int32_t *arc_ptr, const int32_t *arc_src, const float *arc_lp, const float *start_lp,
                          const float *final_lp, float *total, float *gamma) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  if (int rc = fdnn::splice_check(spec, raw_dim)) return rc;
  fdnn::FbJob j;
  if (int rc = fb_front(m, ll, graph_tables(seg_rows, state_ptr, n_segs, states, arc_ptr, arc_src, arc_lp, start_lp, final_lp), gamma != nullptr, n, &j))
    return rc;
  if (n_segs == 0 ? n != 0 : (seg_rows[0] != 0 || seg_rows[n_segs] != n)) return fail(FDNN_E_ARG, "seg_rows must cover the rows [0, n)");
  if (n == 0) return FDNN_OK;
  if (!raw || !total) return fail(FDNN_E_ARG, "null buffer");
  // every segment is an utterance of its own: its edges repeat its own first and last frame
  std::vector<SpliceSeg> segs;
  for (int s = 0; s < n_segs; ++s) segs.push_back(SpliceSeg{seg_rows[s], seg_rows[s], seg_rows[s], seg_rows[s + 1] - 1});
  const sets::Tables t = j.tables();
  return calculate_fb(m, Pass::raw_align("fdnn_calculate_fb_raw", {spec.get(), &segs, raw, n}, t), j, total, gamma, n);
}

int fdnn_debug_fb_launches(unsigned long long *out, int cap) { return counts_out(out, cap, 4, fdnn::fb_launch_counts); }

int fdnn_debug_set_fb_kernel(int mode) {
  if (mode < 0 || mode > 2) return fail(FDNN_E_ARG, "mode is 0 (the plan's rule), 1 (the wave form where allowed) or 2 (the workgroup form)");
  fdnn::fb_kernel_mode(mode);
  return FDNN_OK;
}

int fdnn_debug_fb_limits(int *out, int cap) {
  if (!out || cap < 0) return fail(FDNN_E_ARG, "bad argument");
  const int v[8] = {fdnn::fb::kMaxStates, fdnn::fb::kMaxSegs, fdnn::fb::kWaveStates, fdnn::fb::kMaxArcs, fdnn::fb::kArcLdsArcs, fdnn::fb::kPartials,
                    int(fdnn::fb::kMaxScratchBytes >> 20), fdnn::fb::kWaveRuleStates};
  for (int i = 0; i < 8 && i < cap; ++i) out[i] = v[i];
  return 8;
}

// The recursion in plain C++ (fdnn_fb.hpp: ref), no device: rows, tables and handle values as fdnn_debug_align_graph_ref, the
// transposed tables as fdnn_fb_rows_device takes them, all on the host; gamma (and then the transposed tables) may be null.
int fdnn_debug_fb_ref(const float *rows, const int32_t *seg_T, const long long *row_off, const int32_t *row_ld, const int32_t *state_ptr, int n_segs,
                      const int32_t *col, const int32_t *state_node, const float *log_prior, int width, float floor, int type, const int32_t *arc_ptr,
                      const int32_t *arc_src, const float *arc_lp, const float *start_lp, const float *final_lp, const int32_t *t_ptr,
                      const int32_t *t_src, const float *t_lp, float *total, float *gamma) {
  if (n_segs > 0 && !arc_ptr) return fail(FDNN_E_ARG, "forward-backward, segment 0: malformed tables");
  if (int rc = align_graph_rows_tables(seg_T, row_off, row_ld, state_ptr, arc_ptr, n_segs)) return rc;
  if (n_segs == 0) return FDNN_OK;
  if (type != fdnn::align::kScores && (fdnn::loglik::check_handle(log_prior, width, floor, type) != 0 || !state_node))
    return fail(FDNN_E_ARG, "log_prior [width] finite, the floor -inf or finite (F16: not below -65504), the type F32, F16 or -1 (scores)");
  const bool arcs = arc_ptr[state_ptr[n_segs]] > 0;
  if (!rows || !col || !total || (arcs && (!arc_src || !arc_lp))) return fail(FDNN_E_ARG, "null buffer");
  if (gamma) {
    if (!t_ptr || (arcs && (!t_src || !t_lp))) return fail(FDNN_E_ARG, "forward-backward: gamma needs the transposed tables (fdnn_fb_transpose)");
    if (int rc = fb_t_ptr_ok(state_ptr, arc_ptr, t_ptr, n_segs)) return rc;
  }
  size_t at = 0;
  for (int s = 0; s < n_segs; ++s) {
    const int b = state_ptr[s], S = state_ptr[s + 1] - b;
    uint32_t tb;
    fdnn::fb::ref(reinterpret_cast<const uint32_t *>(rows) + row_off[s], seg_T[s], row_ld[s], col + b, state_node ? state_node + b : nullptr, S, log_prior,
                  width, floor, type, arc_ptr + b, arc_src, arc_lp, start_lp ? start_lp + b : nullptr, final_lp ? final_lp + b : nullptr,
                  gamma ? t_ptr + b : nullptr, t_src, t_lp, &tb, gamma ? reinterpret_cast<uint32_t *>(gamma) + at : nullptr);
    std::memcpy(total + s, &tb, 4);
    at += size_t(seg_T[s]) * size_t(S);
  }
  return FDNN_OK;
}

// op 0: out[i] = exp_neg(a[i]) (b is not read); op 1: out[i] = ladd(a[i], b[i]) -- the header's functions on the host
int fdnn_debug_fb_math_ref(int op, const float *a, const float *b, float *out, long long n) {
  if ((op != 0 && op != 1) || n < 0 || (n && (!a || !out || (op == 1 && !b)))) return fail(FDNN_E_ARG, "bad argument");
  for (long long i = 0; i < n; ++i) out[i] = op == 0 ? fdnn::fb::exp_neg(a[i]) : fdnn::fb::ladd(a[i], b[i]);
  return FDNN_OK;
}

// the same in a trivial kernel over device arrays, enqueued on `stream`
int fdnn_debug_fb_math_device(int op, const float *d_a, const float *d_b, float *d_out, long long n, void *stream) {
  if ((op != 0 && op != 1) || n < 0 || n > (1ll << 31) || (n && (!d_a || !d_out || (op == 1 && !d_b)))) return fail(FDNN_E_ARG, "bad argument");
  fdnn::launch_fb_math(op, d_a, d_b, d_out, n, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return FDNN_OK;
}

int fdnn_ctx_read_hidden(fdnn_ctx *c, uint8_t *out) {
  if (!c || !out) return fail(FDNN_E_ARG, "null argument");
  if (c->last < 0) return fail(FDNN_E_STATE, "hidden layers not computed yet");
  if (c->n == 0) return FDNN_OK;
  DeviceGuard g(c->m->device);
  std::vector<int8_t> tmp(size_t(c->n) * c->act_ld);
  HIP_TRY(ctx_enter(c, c->stream));  // the hidden layers may have been enqueued on a caller's stream
  HIP_TRY(hipMemcpyAsync(tmp.data(), c->d_act[c->last], tmp.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  unpack_act_rows(tmp.data(), size_t(c->act_ld), c->n, c->m->hm.hdr.hidden, out);
  return FDNN_OK;
}

// ---------------------------------------------------------------- dense path
int fdnn_calculate_device(fdnn_model *m, const float *d_x, int n, float *d_out, void *stream) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!d_x || !d_out) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_frames_aligned(d_x)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::device_dense("fdnn_calculate_device", d_x, d_out), static_cast<hipStream_t>(stream));
}

int fdnn_calculate(fdnn_model *m, const float *x, int n, int dim, int batch_hint, float *out) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;  // QuantizedDnn.java:154-156
  if (!x || !out) return fail(FDNN_E_ARG, "null buffer");
  if (m->group) return fdnn_group_calculate(m->group, x, n, dim, batch_hint, out);  // sharded over the node's devices
  return fdnn::calculate_on_one_device(m, x, n, dim, batch_hint, out);
}

// One-call lazy scoring: hidden layers + masked output + compacted return in ONE call and ONE stream synchronisation
// (a LazyContext costs two calls and two synchronisations per utterance: calculateUntilOutput, then the masked rows).
int fdnn_calculate_lazy_bits(fdnn_model *m, const float *x, int n, int dim, const uint64_t *bits, float *out) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!x || !out || !bits) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_input_width(m, dim)) return rc;
  if (m->batcher) {  // coalesced with the other callers' lazy utterances (fdnn_server.cpp), rows back compacted
    uint64_t ticket = 0;
    return batcher_wait(m->batcher, fdnn_server_submit_lazy_bits(m->batcher, x, n, bits, out, &ticket), &ticket);
  }
  // (very large calls: chunk by chunk, as the dense call)
  return score_chunks(m, fdnn::pass::stride_chunks(n), Pass::host_bits("fdnn_calculate_lazy_bits", x, bits, out));
}

int fdnn_calculate_lazy(fdnn_model *m, const float *x, int n, int dim, const int8_t *masks, float *out) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!masks) return fail(FDNN_E_ARG, "null buffer");
  const size_t O = size_t(m->hm.hdr.out_dim), wpr = (O + 63) / 64;
  std::vector<uint64_t> hb(size_t(n) * wpr);
  pack_mask_rows(masks, n, O, hb.data());
  return fdnn_calculate_lazy_bits(m, x, n, dim, hb.data(), out);
}

int fdnn_calculate_lazy_bits_device(fdnn_model *m, const float *d_x, int n, const uint64_t *d_bits, float *d_out, void *stream) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  if (n == 0) return FDNN_OK;
  if (!d_x || !d_out || !d_bits) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = check_frames_aligned(d_x)) return rc;
  return score_chunks(m, frame_chunks(n, m), Pass::device_bits("fdnn_calculate_lazy_bits_device", d_x, d_bits, d_out), static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------- raw feature frames (the <Splice> block on the device)
int fdnn_model_set_splice(fdnn_model *m, const int *offsets, int count, int raw_dim) {
  if (!m) return fail(FDNN_E_ARG, "null model");
  fdnn::SpliceRef spec;  // (a new object: streams, queued submissions and calls in progress keep the one they hold)
  if (count != 0 || raw_dim != 0) {  // (count == 0 with raw_dim == 0 clears the spec; an empty spec of some width is an error)
    if (count < 1 || count > fdnn::kSpliceMaxOffsets) return fail(FDNN_E_ARG, "a splice spec has 1 .. 64 offsets");
    if (!offsets) return fail(FDNN_E_ARG, "null offsets");
    for (int i = 0; i < count; ++i)
      if (offsets[i] < -64 || offsets[i] > 64) return fail(FDNN_E_ARG, "splice offsets must lie in -64 .. 64");
    const int in_dim = m->hm.hdr.in_dim;
    if (raw_dim < 1 || (long long)count * raw_dim > in_dim)
      return fail(FDNN_E_ARG, std::to_string(count) + " x " + std::to_string(raw_dim) + " spliced values do not fit the input width " +
                                  std::to_string(in_dim));
    auto sp = std::make_shared<fdnn::SpliceSpec>();
    sp->offsets.assign(offsets, offsets + count);
    sp->raw_dim = raw_dim;
    for (int o : sp->offsets) {
      sp->left = std::max(sp->left, -o);
      sp->right = std::max(sp->right, o);
    }
    spec = sp;
  }
  // one spec for the whole group when the model leads one (the replicas score its shards; fdnn_group_attach copies the
  // leader's spec to them as well, and a sharded call hands every replica the leader's)
  const int replicas = m->group ? fdnn_group_size(m->group) : 1;
  for (int r = 0; r < replicas; ++r) (m->group ? fdnn_group_model(m->group, r) : m)->splice = spec;
  return FDNN_OK;
}

int fdnn_model_get_splice(const fdnn_model *m, int *offsets, int cap, int *raw_dim) {
  if (!m || cap < 0 || (cap > 0 && !offsets)) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  const int count = spec ? int(spec->offsets.size()) : 0;
  for (int i = 0; i < cap && i < count; ++i) offsets[i] = spec->offsets[size_t(i)];
  if (raw_dim) *raw_dim = spec ? spec->raw_dim : 0;
  return count;
}

int fdnn_calculate_raw(fdnn_model *m, const float *raw, int n, int raw_dim, float *out) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  int rc = fdnn::splice_check(spec, raw_dim);
  if (rc) return rc;
  if (n == 0) return FDNN_OK;
  if (!raw || !out) return fail(FDNN_E_ARG, "null buffer");
  // as fdnn_calculate: sharded over an attached group first (each replica uploads its shard + halo, through its own batcher
  // when it has one), else through the model's batcher, else on the model's device
  if (m->group) return fdnn::group_calculate_raw(m->group, spec, raw, n, out);
  return fdnn::calculate_raw_rows(m, spec, raw, n, 0, n, out);
}

int fdnn_calculate_raw_device(fdnn_model *m, const float *d_raw, int n, const int *seg_starts, int n_segs, float *d_out, void *stream) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  int rc = fdnn::splice_check(spec, -1);
  if (rc) return rc;
  if (n == 0) return FDNN_OK;
  if (!d_raw || !d_out) return fail(FDNN_E_ARG, "null buffer");
  std::vector<fdnn::SpliceSeg> segs;
  if (!seg_starts) {
    segs.push_back(fdnn::SpliceSeg{0, 0, 0, n - 1});
  } else {
    if (n_segs < 1 || seg_starts[0] != 0) return fail(FDNN_E_ARG, "a segment table starts with 0");
    for (int k = 0; k < n_segs; ++k) {
      const int a = seg_starts[k], b = k + 1 < n_segs ? seg_starts[k + 1] : n;
      if (b <= a || b > n) return fail(FDNN_E_ARG, "segment starts must ascend strictly and lie below n");
      segs.push_back(fdnn::SpliceSeg{a, a, a, b - 1});
    }
  }
  // each chunk's rows spliced into the context's frame buffer, then scored as usual
  return score_chunks(m, frame_chunks(n, m), Pass::raw_device_dense("fdnn_calculate_raw_device", {spec.get(), &segs, d_raw, n}, d_out), static_cast<hipStream_t>(stream));
}

int fdnn_calculate_lazy_bits_raw(fdnn_model *m, const float *raw, int n, int raw_dim, const uint64_t *bits, float *out) {
  if (!m || n < 0) return fail(FDNN_E_ARG, "bad argument");
  const fdnn::SpliceRef spec = m->splice;
  int rc = fdnn::splice_check(spec, raw_dim);
  if (rc) return rc;
  if (n == 0) return FDNN_OK;
  if (!raw || !out || !bits) return fail(FDNN_E_ARG, "null buffer");
  if (m->batcher) {
    uint64_t ticket = 0;
    return batcher_wait(m->batcher, server_submit_raw_rows(m->batcher, spec, raw, n, 0, n, bits, out, &ticket), &ticket);
  }
  const std::vector<SpliceSeg> segs{SpliceSeg{0, 0, 0, n - 1}};
  return score_chunks(m, fdnn::pass::stride_chunks(n),  // (chunks as fdnn_calculate_lazy_bits)
                      Pass::raw_bits("fdnn_calculate_lazy_bits_raw", {spec.get(), &segs, raw, n}, bits, out));
}

int fdnn_ctx_forward_hidden_raw(fdnn_ctx *c, const float *raw) {
  if (!c) return fail(FDNN_E_ARG, "null argument");
  const fdnn::SpliceRef spec = c->m->splice;
  int rc = fdnn::splice_check(spec, -1);
  if (rc) return rc;
  if (c->n == 0) {
    c->last = 0;
    return FDNN_OK;
  }
  if (!raw) return fail(FDNN_E_ARG, "null argument");
  DeviceGuard g(c->m->device);
  const size_t D = size_t(spec->raw_dim);
  CtxUse use;
  HIP_TRY(use.enter(c, c->stream));
  rc = fdnn::ctx_raw_reserve(c, size_t(c->n), spec->raw_dim);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_raw, raw, sizeof(float) * size_t(c->n) * D, hipMemcpyHostToDevice, c->stream));
  fdnn::splice_rows(*spec, c->m->hm.hdr.in_dim, c->d_raw, c->n, {fdnn::SpliceSeg{0, 0, 0, c->n - 1}}, 0, c->n, c->d_x, c->stream);
  rc = run_hidden(c, c->d_x, c->stream, nullptr);
  use.leave();
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return FDNN_OK;
}

}  // extern "C"

// A stream of raw frames (fdnn_stream_*).  Its device buffer holds global frames [base, base + len): the frames still to be
// read by rows not emitted yet -- at most L + R of them between pushes (L / R: the left / right context of the offsets) --
// and the push's new ones.  Before a push the kept frames move to the front of the other buffer of a pair (device to
// device, L + R frames): nothing is uploaded twice.
struct fdnn_stream {
  fdnn_model *m = nullptr;
  fdnn_ctx *c = nullptr;  // the stream's own context: max_chunk + R frames
  fdnn::SpliceRef spec;   // the model's spec when the stream was made: every push splices with it
  int raw_dim = 0, max_chunk = 0, left = 0, right = 0;
  fdnn::DevBuf<float> d_buf[2];
  int cur = 0;
  fdnn::stream::Window w;  // where the utterance stands (fdnn_stream_plan.hpp: the arithmetic shared with the loop's live handles)
};

extern "C" {

int fdnn_stream_create(fdnn_model *m, int max_chunk, fdnn_stream **out) {
  if (!m || !out) return fail(FDNN_E_ARG, "null argument");
  *out = nullptr;
  const fdnn::SpliceRef spec = m->splice;
  int rc = fdnn::splice_check(spec, -1);
  if (rc) return rc;
  if (max_chunk < 1) return fail(FDNN_E_ARG, "max_chunk must be positive");
  DeviceGuard g(m->device);
  fdnn_stream *s = new fdnn_stream();
  s->m = m;
  s->spec = spec;
  s->raw_dim = spec->raw_dim;
  s->max_chunk = max_chunk;
  s->left = spec->left;
  s->right = spec->right;
  rc = fdnn::make_ctx(m, max_chunk + s->right, &s->c);
  const size_t frames = size_t(max_chunk) + size_t(s->left) + size_t(s->right);
  for (int k = 0; k < 2 && !rc; ++k)
    if (s->d_buf[k].reserve(frames * size_t(s->raw_dim)) != hipSuccess)
      rc = fail(FDNN_E_NOMEM, "stream buffer of " + std::to_string(frames) + " raw frames");
  if (rc) {
    fdnn_stream_free(s);
    return rc;
  }
  s->c->n = 0;
  *out = s;
  return FDNN_OK;
}

void fdnn_stream_free(fdnn_stream *s) {
  if (!s) return;
  DeviceGuard g(s->m->device);
  if (s->c) fdnn::destroy_ctx(s->c);  // (synchronises the stream's work)
  delete s;
}

int fdnn_stream_reset(fdnn_stream *s) {
  if (!s) return fail(FDNN_E_ARG, "null stream");
  s->w = fdnn::stream::Window{};
  return FDNN_OK;
}

int fdnn_stream_position(const fdnn_stream *s, int64_t *pushed, int64_t *emitted) {
  if (!s) return fail(FDNN_E_ARG, "null stream");
  if (pushed) *pushed = s->w.pushed;
  if (emitted) *emitted = s->w.emitted;
  return FDNN_OK;
}

fdnn_ctx *fdnn_stream_ctx(fdnn_stream *s) { return s ? s->c : nullptr; }

int fdnn_stream_push(fdnn_stream *s, const float *raw, int n_raw, int end, float *out, int *n_out) {
  if (!s || !n_out) return fail(FDNN_E_ARG, "null argument");
  *n_out = 0;
  if (s->w.ended) return fail(FDNN_E_STATE, "the stream has ended: fdnn_stream_reset starts the next utterance");
  if (n_raw < 0 || n_raw > s->max_chunk) return fail(FDNN_E_ARG, "a push holds 0 .. max_chunk raw frames");
  if (n_raw > 0 && !raw) return fail(FDNN_E_ARG, "null raw frames");
  fdnn_model *m = s->m;
  fdnn_ctx *c = s->c;
  DeviceGuard g(m->device);
  const size_t D = size_t(s->raw_dim);
  hipStream_t st = c->stream;
  CtxUse use;  // (left when the push returns: every way out below has synchronised or failed)
  HIP_TRY(use.enter(c, st));
  // keep what rows not emitted yet still read: frames from emitted - L on
  fdnn::stream::Window &w = s->w;
  const fdnn::stream::Keep k = fdnn::stream::keep_frames(w, s->left);
  if (k.moved) {
    if (k.kept > 0)
      HIP_TRY(hipMemcpyAsync(s->d_buf[s->cur ^ 1], s->d_buf[s->cur] + size_t(k.drop) * D, sizeof(float) * size_t(k.kept) * D,
                             hipMemcpyDeviceToDevice, st));
    s->cur ^= 1;
  }
  const long long at = fdnn::stream::append_frames(w, n_raw);
  if (n_raw > 0)
    HIP_TRY(hipMemcpyAsync(s->d_buf[s->cur] + size_t(at) * D, raw, sizeof(float) * size_t(n_raw) * D, hipMemcpyHostToDevice, st));
  // complete rows: t + R has arrived; at the end of the stream every row, right-clamped to the last frame
  const fdnn::stream::Rows done = fdnn::stream::complete_rows(w, s->right, end != 0);
  const int rows = done.rows;
  int rc = FDNN_OK;
  c->n = rows;
  c->last = rows ? -1 : 0;
  if (rows > 0) {
    const std::vector<fdnn::SpliceSeg> segs{done.seg};
    fdnn::splice_rows(*s->spec, m->hm.hdr.in_dim, s->d_buf[s->cur], int(w.len), segs, 0, rows, c->d_x, st);
    if (out) {
      rc = dense_pass_to_host(c, out, st);  // (synchronises)
    } else {
      rc = run_hidden(c, c->d_x, st, nullptr);  // hidden layers only: the context's lazy entry points take it from here
      if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(FDNN_E_DEVICE, "fdnn_stream_push: stream synchronisation");
    }
  } else if (hipStreamSynchronize(st) != hipSuccess) {  // (the caller's raw frames have been read when the push returns)
    rc = fail(FDNN_E_DEVICE, "fdnn_stream_push: stream synchronisation");
  }
  if (rc) return rc;
  fdnn::stream::commit(w, done, end != 0);
  *n_out = rows;
  return FDNN_OK;
}

// ---------------------------------------------------------------- weight blob exchange
int fdnn_model_blob_size(const fdnn_model *m, size_t *bytes) {
  if (!m || !bytes) return fail(FDNN_E_ARG, "null argument");
  *bytes = m->hm.blob.size();
  return FDNN_OK;
}

int fdnn_model_export_blob(const fdnn_model *m, void *d_dst, size_t capacity, void *stream) {
  if (!m || !d_dst) return fail(FDNN_E_ARG, "null argument");
  if (capacity < m->hm.blob.size()) return fail(FDNN_E_ARG, "destination smaller than the blob");
  DeviceGuard g(m->device);
  HIP_TRY(hipMemcpyAsync(d_dst, m->d_blob, m->hm.blob.size(), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  return FDNN_OK;
}

int fdnn_model_import_blob(const void *d_src, size_t bytes, int device, fdnn_model **out) {
  if (!d_src || !out) return fail(FDNN_E_ARG, "null argument");
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(FDNN_E_DEVICE, "no HIP device available: this library has no CPU path");
  if (device < 0 || device >= count) return fail(FDNN_E_ARG, "device index out of range");
  DeviceGuard g(device);
  std::vector<uint8_t> host(bytes);
  HIP_TRY(hipMemcpy(host.data(), d_src, bytes, hipMemcpyDeviceToHost));
  std::unique_ptr<fdnn_model> own(new fdnn_model());
  fdnn_model *m = own.get();
  std::string msg;
  int rc = fdnn::adopt_blob(std::move(host), &m->hm, &msg);
  if (rc) return fail(rc, msg);
  m->device = device;
  hipError_t e = m->d_blob.reserve(bytes);
  if (e == hipSuccess) e = hipMemcpy(m->d_blob, d_src, bytes, hipMemcpyDeviceToDevice);
  if (e != hipSuccess) return fail(FDNN_E_DEVICE, std::string("blob import: ") + hipGetErrorString(e));
  rc = build_l0_image(m);
  if (rc) return rc;
  *out = own.release();
  return FDNN_OK;
}

}  // extern "C"
