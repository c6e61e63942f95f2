// fdnn_internal.hpp -- what the runtime's translation units share: the model / context objects
// behind the opaque C-ABI handles and the enqueue helpers over them (fdnn_runtime.cpp, fdnn_lazy_entries.cpp), used by
// the scoring C-ABI (fdnn_api.cpp), the debug / profiling / host-model calls (fdnn_debug.cpp),
// the multi-stream server loop (fdnn_server.cpp) and the device group (fdnn_group.cpp).
// Not installed; the boundary is include/fdnn.h.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fdnn.h"
#include "fdnn_buf.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_model.hpp"
#include "fdnn_pass.hpp"
#include "fdnn_splice_spec.hpp"  // SpliceSpec, SpliceRef, SpliceSeg, splice_halo

namespace fdnn {

int fail(int code, const std::string &msg);  // sets fdnn_last_error() of the calling thread, returns code

#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return ::fdnn::fail(FDNN_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));            \
  } while (0)

inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

struct DeviceGuard {
  int prev = 0;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
  }
  ~DeviceGuard() {
    if (ok) hipSetDevice(prev);
  }
};

}  // namespace fdnn

struct fdnn_model {
  fdnn::HostModel hm;  // header + host copy of the blob (kept: export, host queries)
  int device = 0;
  fdnn::DevBuf<uint8_t> d_blob;
  fdnn::DevBuf<float> d_w0t;  // layer-0 weights as a chain-major image [4][l0_j_pad][l0_h_ld] (fdnn_l0.hip)
  fdnn::DevBuf<float> d_w0norm;  // [H] ||w_n||_2 rounded up: the node half of the screened layer-0 path's bound
  fdnn::DevBuf<int8_t> d_w0d;    // int8 screening (fdnn_l0s.hip): the layer-0 weights as three int8 digit planes, MFMA fragment order
  fdnn::DevBuf<float> d_w0stat;  // [3][l0_h_ld]: 2^8 / c_n, ||w_n||_2, 2^8 b_n
  fdnn::DevBuf<uint32_t> d_lutpair;  // the sigmoid table as (round-down, round-up) byte pairs
  // lazy output by lists (fdnn_lists.hip): the output layer's saturating pairs indexed per NODE, built at load from the
  // blob's group-ordered list (fdnn_lists.hpp); both null when the layer has none.  Not part of the blob.
  fdnn::DevBuf<int32_t> d_lfix_off;     // [O + 1]
  fdnn::DevBuf<uint32_t> d_lfix_pairs;  // [n_fix] k | w0 << 16 | w1 << 24
  // the device side of "is somebody else scoring on this GPU?".  A fused soft-max workgroup that
  // sits out its bounded wait (tens of milliseconds: its frame tile's siblings were kept off the chip) raises this
  // host-mapped word; from the next call on the model runs the scale-pass path, for good, and says so once.
  fdnn::Mapped<unsigned long long> h_fuse_fault;  // (.dev: what the kernels get; null where the allocation was refused)
  bool fuse_fault_said = false;
  fdnn::DevBuf<unsigned long long> d_l0_stats;  // [4] device counters: [1] layer-0 outputs recomputed exactly, [2] fused soft-max tiles that gave up waiting
  int l0_jc = 0, l0_j_pad = 0, l0_h_ld = 0;
  int l0_fma = 0;
  int lists_union = 0;  // fdnn_model_set_lists_union: 0 = list calls on the dot-product kernels, g in 1..8 = over unions of 32 g rows
  int l0_kernel = 0;  // fdnn_debug_set_l0_kernel
  int l0_list_cap = 0;  // fdnn_debug_set_l0_list_cap: > 0 caps the flagged-output list of contexts created afterwards (tests)
  fdnn::SpliceRef splice;  // fdnn_model_set_splice (null = no spec: the raw entry points refuse)
  std::mutex mu;
  std::vector<fdnn_ctx *> pool;  // idle contexts owned by the model (fdnn_calculate*)
  struct fdnn_server *batcher = nullptr;  // fdnn_model_enable_batcher: fdnn_calculate goes through it
  struct fdnn_group *group = nullptr;     // fdnn_group_attach: this model leads a device group, fdnn_calculate shards over it
  // per-kernel HIP-event timing (fdnn_profile_begin/end); off in production
  bool profiling = false;
  struct ProfRec {
    int kind;
    hipEvent_t a, b;
  };
  std::vector<ProfRec> prof;
};

// A node -> class map as the pooling reads it (fdnn_pool.hpp: pool::build_csr), on the host and on the device that was
// current at fdnn_pool_create.  Immutable from then on: threads, contexts and scoring loops share it.
struct fdnn_pool {
  int width = 0, n_classes = 0, device = 0;
  fdnn::pool::Csr csr;
  fdnn::DevBuf<int32_t> d_csr;  // class_ptr [C + 1], then member [nnz]
  const int32_t *d_class_ptr() const { return d_csr.p; }
  const int32_t *d_member() const { return d_csr.p + n_classes + 1; }
};

// A decoder-score handle (fdnn_loglik.hpp): the log priors on the host and on the device that was current at
// fdnn_loglik_create, the floor and the output type.  Immutable from then on: threads, contexts and scoring loops share it.
struct fdnn_loglik {
  int width = 0, type = 0, device = 0;
  float floor = 0.0f;
  std::vector<float> log_prior;
  fdnn::DevBuf<float> d_log_prior;  // [width]
};

struct fdnn_ctx {
  fdnn_model *m = nullptr;
  int n = 0;              // frames in use
  int cap = 0;            // frames the scratch was allocated for (padded)
  int act_ld = 0;
  hipStream_t stream = nullptr;   // own stream for the host-pointer entry points
  hipEvent_t done = nullptr;      // last enqueued work (pool hand-over between streams, ctx_enter/ctx_leave)
  hipStream_t done_stream = nullptr;  // the stream `done` was last recorded on
  bool done_valid = false;
  bool done_pending = false;      // work went to done_stream -- a stream that outlives this context's use of it (see
                                  // stream_is_durable) -- after the last record: recorded when ANOTHER stream asks (ctx_enter)
  hipStream_t durable[2] = {nullptr, nullptr};  // streams of the context's owner (the scoring loop's), besides `stream`
  fdnn::DevBuf<float> d_x;        // [n][D]
  fdnn::DevBuf<float> d_raw;      // raw feature frames of the *_raw entry points (first raw call allocates)
  fdnn::DevBuf<float> d_xt;       // [4][l0_j_pad][xt_ld] layer-0 frame image (shifted, scaled, chain-major)
  int xt_ld = 0;
  fdnn::DevBuf<float> d_l0park;   // [xt_ld][l0_h_ld] partial chain sums parked by the layer-0 kernel
  fdnn::DevBuf<uint32_t> d_scr_count;  // [frame tiles x node tiles] flagged outputs per tile (kept zero between launches)
  fdnn::DevBuf<uint16_t> d_scr_list;   // [tiles][kL0ScreenCap]
  fdnn::DevBuf<int8_t> d_xd;        // int8 screening: the frames' digit planes [chunks][3][xt_ld / 32][1024]
  fdnn::DevBuf<float> d_xstat;      // [3][xt_ld] row constants written by the pre-pass
  fdnn::DevBuf<uint2> d_glist;      // int8 screening: {frame, node} of the launch's flagged outputs
  fdnn::DevBuf<uint32_t> d_glist_count;  // [2] entries appended, tiles in the whole-tile path
  fdnn::DevBuf<int8_t> d_act[2];  // [n_pad][act_ld] ping/pong, s8 = u8-128
  fdnn::DevBuf<float> d_out;      // [n][O]
  fdnn::DevBuf<float> d_partial;  // [rows_pad/64][n_pad]
  fdnn::DevBuf<int8_t> d_mask;    // [n][O]
  fdnn::DevBuf<float> d_fuse_s;     // fused soft-max: per-tile row sums [n_pad / tile][rows_pad / 256][tile] floats
  fdnn::DevBuf<uint32_t> d_fuse_cnt;   // {arrived part 0 .., left at [7]} per frame tile; zero between launches
  fdnn::DevBuf<uint32_t> d_fuse_flag;  // per tile: parts a workgroup left unscaled ("gave up waiting"); zero between launches
  fdnn::DevBuf<uint32_t> d_chain_ctl;   // chained hidden layers (fdnn_chain.hip): queue heads [0..7], workgroups that left [8]
  fdnn::DevBuf<uint32_t> d_chain_done;  // [frame tiles][layers of the chain] node tiles finished; zero between launches
  fdnn::DevBuf<long long> d_chain_clk;  // measurement builds only: 8 words + 10 phase clocks per task (fdnn_debug_chain_clocks)
  // A chained launch whose wait ran into its bound has computed on rows that may not have been written: it raises this
  // host-visible word (fine-grained pinned memory, plain store from the kernel).  run_hidden looks at it before every
  // launch -- counters re-zeroed, the context never chains again -- and the calls that synchronise anyway re-run the pass.
  fdnn::Mapped<unsigned long long> h_chain_fault;
  bool chain_broken = false;
  fdnn::DevBuf<float> d_l0_dbg_t, d_l0_dbg_dd;  // fdnn_debug_layer0_screen only: the int8 screening's t~ and Dd per output
  fdnn::DevBuf<uint64_t> d_mask_bits;  // [n][ceil(O/64)] the batched lazy call's mask as bits (launch_mask_pack)
  bool mask_bits_packed = false;    // run_output has packed the current call's byte masks into d_mask_bits
  fdnn::DevBuf<float> d_comp;       // host lazy batches: compacted result rows (allocated on first use)
  fdnn::DevBuf<int32_t> d_topk;     // host top-k calls: [n][k] nodes, then [n][k] values (allocated on first use, fdnn_topk.hip)
  fdnn::DevBuf<float> d_pool;       // host pool calls: [n][C] class sums (allocated on first use, fdnn_pool.hip; not in ctx_layout)
  fdnn::DevBuf<uint32_t> d_loglik;  // host loglik calls: [n][O] scores, fp32 or fp16 (allocated on first use, fdnn_loglik.hip; not in ctx_layout)
  // align calls (fdnn_align.hip; allocated on first use and grown by the largest call, not in ctx_layout): the transcripts'
  // node sets, columns and nodes [n_nodes | n_states | n_states], their transition scores [n_states | n_states], the sets'
  // probabilities (ragged blocks) and inactive values, the take words that do not fit LDS, and the results [sum T | n_segs]
  fdnn::DevBuf<int32_t> d_al_int;
  fdnn::DevBuf<float> d_al_lp, d_al_probs, d_al_inact;
  fdnn::DevBuf<uint32_t> d_al_bp;
  fdnn::DevBuf<int32_t> d_al_res;
  // align-graph calls (fdnn_align_graph.hip) share the align buffers above and add the graphs' tables: arc_ptr [n_states + 1]
  // | arc_src [arcs], and arc_lp [arcs] | start_lp [n_states] | final_lp [n_states]
  fdnn::DevBuf<int32_t> d_ag_int;
  fdnn::DevBuf<float> d_ag_lp;
  // forward-backward calls (fdnn_fb.hip) share both sets of buffers above -- the lattice is the scratch d_al_bp -- and add the
  // transposed tables t_ptr [n_states + 1] | t_src [arcs], t_lp [arcs], and the results total [n_segs] | gamma [sum T S]
  fdnn::DevBuf<int32_t> d_fb_int;
  fdnn::DevBuf<float> d_fb_lp, d_fb_res;
  // host list calls (fdnn_ctx_lazy_output_lists, fdnn_calculate_lazy_lists): staging of the lists and their results,
  // allocated on the first list call and grown by the largest one
  fdnn::DevBuf<int32_t> d_lrow, d_lnodes;   // [count + 1], [nnz]
  fdnn::DevBuf<float> d_lprobs, d_linact;   // [nnz], [count]
  // set calls served by the list kernels (run_set's fallback): the set as lists, row_ptr [count + 1] and nodes [count * len]
  fdnn::DevBuf<int32_t> d_srow, d_snodes;
  // list calls scored over per-frame-group unions (fdnn_model_set_lists_union): unions, ranks, lengths, the work list and
  // its counter in one buffer (lunion::Layout: O(nnz + count) words), allocated on the first such call and grown by the largest
  fdnn::DevBuf<int32_t> d_union;
  int last = -1;                 // d_act index holding the last hidden layer, -1 = not computed
  bool pooled = false;
  bool no_fuse = false;           // this call must not use the fused soft-max
  // per-frame lazy calls (the JNI contract): host-mapped pinned staging for kPinFrames masks and
  // result rows -- the output kernel reads the mask and the scale kernel writes the probabilities
  // straight through these, so a call is two launches and one stream sync, no copy commands
  fdnn::Mapped<int8_t> h_mask_pin;
  fdnn::Mapped<float> h_out_pin;
};


namespace fdnn {

// Brackets one kernel launch with HIP events on the launch stream when profiling is on.
struct ProfScope {
  fdnn_model *m;
  hipStream_t s;
  int kind;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(fdnn_model *m_, hipStream_t s_, int kind_) : m(m_), s(s_), kind(kind_) {
    if (!m->profiling) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
      a = b = nullptr;
      return;
    }
    hipEventRecord(a, s);
  }
  ~ProfScope() {
    if (!a) return;
    hipEventRecord(b, s);
    std::lock_guard<std::mutex> lk(m->mu);
    m->prof.push_back({kind, a, b});
  }
};

struct Taps {
  float *l0_lin = nullptr;
  uint8_t *u8_acts = nullptr;   // device [n_hidden][n][H]
  int32_t *acc_hid = nullptr;   // device [n_hidden-1][n][H]
  int32_t *acc_out = nullptr;   // device [n][O]
  float *logits = nullptr;      // device [n][O]
  int32_t *acc_probe = nullptr; // device [ceil(n / probe_stride)][O]: accumulators of the PRODUCTION output instance (no tap kernels)
  int probe_stride = 1;
};

// lean: a scoring-loop slot -- no frame / result / mask buffers and no per-frame pinned staging of its own (device
// submissions bring their buffers; the host path allocates what it needs in alloc_host_side)
int make_ctx(fdnn_model *m, int n, fdnn_ctx **out, bool lean = false);
void destroy_ctx(fdnn_ctx *c);
// The scratch audit.  ctx_scratch_buf: row `row` of kCtxScratch (fdnn_ctx_layout.hpp) in this context.
// ctx_scratch_dirty: waits for the context's last work (ctx_wait_host), copies every row to the host and counts its non-zero
// words into out[kCtxScratchCount]; the chain rows of a context whose h_chain_fault is raised count as clean (dirty by
// design: run_hidden re-zeroes them), and so does fuse_cnt once a role-split fused launch of the model has left a half unwritten
// (run_output zeroes it before every fused launch from then on).  scratch_audit_event: what release_ctx and destroy_ctx -- a scoring-loop slot's
// teardown among its callers -- do while fdnn_debug_scratch_audit is on: the same count, added to the process's totals.
struct ScratchBuf {
  uint32_t *p;
  size_t words;
};
ScratchBuf ctx_scratch_buf(fdnn_ctx *c, int row);
int ctx_scratch_dirty(fdnn_ctx *c, unsigned long long *out);
void scratch_audit_event(fdnn_ctx *c);
int upload_model(fdnn_model *m);    // blob to the device, division check, then build_l0_image
int build_l0_image(fdnn_model *m);  // the layer-0 weight images and the model's counters, from m->d_blob
// Layer 0 of the context's n frames into d_act[0] (fdnn_debug_layer0* run it alone).
void run_layer0(fdnn_ctx *c, const float *d_x, hipStream_t s, const Taps *taps);
// CalculateUntilLastHiddenLayer (dnn.cc:402-424) enqueued on s.
int run_hidden(fdnn_ctx *c, const float *d_x, hipStream_t s, const Taps *taps);
// CalculateOutput / LazyOutputActivations (dnn.cc:428-454, :355-392) over frames [first, first+count):
// the output GEMM (exp(z) rows + partial sums) on s, then the soft-max scale.  What a call does beyond "all of the
// context's frames, dense, in place" is named in an OutputCall: every field defaults to null / zero.
struct OutputCall {
  int first = 0, count = 0;           // frames [first, first + count) of the context
  const int8_t *d_masks = nullptr;    // [count][O] bytes, non-zero = active (null: dense, or d_bits)
  const uint64_t *d_bits = nullptr;   // the masks of the same frames as BITS, [count][ceil(O / 64)], bit b of word w = node
                                      // 64 w + b; then d_masks may be null -- large batches read the words as they are,
                                      // small ones unpack them into the context's byte mask first
  float *d_out = nullptr;             // [count][O]: exp(z) rows, scaled in place unless d_final says otherwise
  float *d_final = nullptr;           // where the probabilities go (null: in place in d_out)
  const Taps *taps = nullptr;
};
int run_output(fdnn_ctx *c, const OutputCall &oc, hipStream_t s);
// LazyOutputActivations (dnn.cc:355-392) for the LISTED nodes only (fdnn_lists.hip): rows [first, first + count) of the
// context, their lists and results on the device; enqueued on s.  d_acc (parity tests) may be null.
struct ListsCall {
  int first = 0, count = 0;
  const int32_t *d_row_ptr = nullptr;  // [count + 1]
  const int32_t *d_nodes = nullptr;    // [nnz]
  int nnz = 0;
  float *d_probs = nullptr;            // [nnz]
  float *d_inactive = nullptr;         // [count]
  int32_t *d_acc = nullptr;            // [nnz]
};
int run_lists(fdnn_ctx *c, const ListsCall &lc, hipStream_t s);
// The same contract with ONE node set for rows [first, first + count) (fdnn_set.hip): d_nodes [len], d_probs [count][len],
// d_inactive [count]; enqueued on s.  d_acc [count][len] (parity tests) may be null.
struct SetCall {
  int first = 0, count = 0;
  const int32_t *d_nodes = nullptr;
  int len = 0;
  float *d_probs = nullptr;
  float *d_inactive = nullptr;
  int32_t *d_acc = nullptr;
};
int run_set(fdnn_ctx *c, const SetCall &sc, hipStream_t s);
// The same contract with one node set per SEGMENT of rows [first, first + rows of segs) (fdnn_sets.hip): segs as
// sets::slice returns them -- consecutive rows from 0, blocks from 0 --, d_nodes the sets that set_off indexes, d_probs the
// ragged blocks, d_inactive one value per row; enqueued on s.  The launch tables travel as kernel arguments, the row pointer
// of the finish pass through the context's staging buffer (d_srow).  d_acc (parity tests, ragged like d_probs) may be null.
struct SetsCall {
  int first = 0;
  const std::vector<fdnn::sets::Seg> *segs = nullptr;
  const int32_t *d_nodes = nullptr;
  float *d_probs = nullptr;
  float *d_inactive = nullptr;
  int32_t *d_acc = nullptr;
};
int run_sets(fdnn_ctx *c, const SetsCall &sc, hipStream_t s);
// The three above are fdnn_lazy_entries.cpp's one driver with a score step each.  lazy_state: FDNN_E_STATE, in the words the
// device forms return, unless the context's hidden layers have run.
int lazy_state(const fdnn_ctx *c);
// The host form of all three: validated lists (row_ptr), segments (segs: of validated tables, as sets::slice returns them) or
// one set (neither: `len` nodes) for rows [first, first + count) and all `n_nodes` nodes up, results back -- probs: the
// entries in call order, for segments the slice's blocks, one contiguous range -- and s synchronised.  acc (parity tests)
// may be null.
struct HostEntries {
  int first = 0, count = 0;
  const int32_t *row_ptr = nullptr;                    // [count + 1]
  const std::vector<fdnn::sets::Seg> *segs = nullptr;
  int len = 0;
  const int32_t *nodes = nullptr;
  int n_nodes = 0;
  float *probs = nullptr, *inactive = nullptr;
  int32_t *acc = nullptr;
};
int entries_to_host(fdnn_ctx *c, const HostEntries &h, hipStream_t s);
// The union kernels' view of the lists in lc (first is not read) and of a buffer b laid out by l (fdnn_lists_union.hpp)
UnionParams union_params(const lunion::Layout &l, int32_t *b, const ListsCall &lc, int rows, int group_tiles);
int build_lists_index(fdnn_model *m);  // the per-node pair index of the output layer, from m->hm (model load / blob import)
int device_cus(int device);            // CUs of a device, asked once (256 where the runtime cannot say)
// Device -> pageable host memory, pre-faulting large destinations; synchronises s.
int copy_out(void *dst, const void *d_src, size_t bytes, hipStream_t s);
// The dense pass over the context's frames in c->d_x (c->n of them) into the host's `out`, synchronising s; re-runs what a
// fused soft-max or chained launch that sat out its bounded wait left wrong.
int dense_pass_to_host(fdnn_ctx *c, float *out, hipStream_t s);
// The same pass with "what leaves the device" as the step that differs: the whole rows into out (k = 0), or the k
// first-ranked nodes of every row and their values into nodes / probs [n][k] (fdnn_topk.hip), or the rows' class sums under
// `pool` into pooled [n][C] (fdnn_pool.hip), or the rows as decoder scores under `loglik` into scores [n][O] of the handle's
// type (fdnn_loglik.hip) -- the rows stay in c->d_out.
// hidden = false: the context holds the hidden activations already (fdnn_ctx_output_topk); the fused soft-max's re-run
// applies, the chained launch's belongs to whoever ran the hidden layers.
struct DenseTo {
  float *out = nullptr;
  int k = 0;
  int32_t *nodes = nullptr;
  float *probs = nullptr;
  const fdnn_pool *pool = nullptr;
  float *pooled = nullptr;
  const fdnn_loglik *loglik = nullptr;
  void *scores = nullptr;
};
int dense_pass(fdnn_ctx *c, const DenseTo &to, hipStream_t s, bool hidden);
// Lazy results of `count` frames (c->d_out) to a host caller, compacted over PCIe where that pays; d_bits / bits: the
// frames' masks on the device / on the host.  Synchronises s.
int lazy_copy_out(fdnn_ctx *c, int count, const uint64_t *d_bits, const uint64_t *bits, float *out, hipStream_t s);
// Host half of a compacted lazy return: expands `count` compacted rows sitting in the tail of out[count][O] (fdnn_runtime.cpp).
void lazy_expand_rows(float *out, int count, size_t O, size_t stride, const uint64_t *bits);
void lazy_expand_rows_from(float *out, const float *comp, int count, size_t O, size_t stride, const uint64_t *bits);  // rows in a buffer of their own
void lazy_expand_force_scalar(bool on);  // fdnn_debug_lazy_expand: the scalar expansion where AVX-512 would be used
// The chunks of an n-frame pass (fdnn_pass.hpp: pass::frame_chunks).  With a model: a chunk whose hidden layers will not run as
// one chained launch (hidden_layers_chain) gives up to kChunkTailSplit frames past a whole round away as a batch of their own.
// Without: as assume_chained says (fdnn_debug_frame_chunks_for).
pass::Chunks frame_chunks(int n, const fdnn_model *m = nullptr, bool assume_chained = true);
bool hidden_layers_chain(const fdnn_model *m, int n);
// "input vector size ... must be equal with network input size ..." (QuantizedDnn.java:157-161)
int check_input_width(const fdnn_model *m, int dim);
// A caller's device frames [n][in_dim] must start on a 16-byte boundary: layer 0 reads them as 16-byte LDS-DMA pieces
// (l0_small_kernel, fdnn_l0.hip), whose source address nothing establishes as free.  in_dim is a multiple of 4, so every row
// and every chunk of rows keeps the alignment of the base.  FDNN_E_ARG before anything is launched.
int check_frames_aligned(const float *d_x);
// A pool call's handle against the model it is used with: the map's width is the model's output_dim, the CSR lives on the
// model's device, and the model leads no device group.  FDNN_E_ARG before anything is launched.
int check_pool(const fdnn_model *m, const fdnn_pool *pool);
// The same for a decoder-score handle: its width is the model's output_dim, its priors live on the model's device, and the
// model leads no device group.  FDNN_E_ARG before anything is launched.
int check_loglik(const fdnn_model *m, const fdnn_loglik *ll);
// The second half of a call through a model's batcher: `submitted` is what the submit call returned, *ticket what it filled in.
inline int batcher_wait(fdnn_server *b, int submitted, const uint64_t *ticket) { return submitted ? submitted : fdnn_server_wait(b, *ticket); }
// fdnn_calculate on the model's own device (the group path calls this per shard).
int calculate_on_one_device(fdnn_model *m, const float *x, int n, int dim, int batch_hint, float *out);
// [n][ld] s8 activations (u8 - 128, as the kernels keep them) -> [n][H] u8
inline void unpack_act_rows(const int8_t *src, size_t ld, int n, int H, uint8_t *dst) {
  for (int f = 0; f < n; ++f)
    for (int i = 0; i < H; ++i) dst[size_t(f) * H + i] = uint8_t(src[size_t(f) * ld + i]) ^ 0x80;
}
// The soft-max fusing switches (run_output): this process's device marker (1 = ours or cannot tell, 0 = another process's)
// and fdnn_debug_set_fuse's override (-1 = by environment / marker, 0 = never, 1 = always).
int device_marker_state(int device);
// ---------------------------------------------------------------- raw feature frames (fdnn_splice.hip)
// FDNN_E_STATE without a spec, FDNN_E_ARG when raw_dim is not its D (raw_dim < 0: any)
int splice_check(const SpliceRef &spec, int raw_dim);
// Room for `frames` raw frames of width raw_dim (c->d_raw) and, on a lean context, the frame buffer c->d_x; allocated on
// the first raw call.
int ctx_raw_reserve(fdnn_ctx *c, size_t frames, int raw_dim);
// Splices rows [row0, row0 + rows) into d_x [rows][input_dim] (row row0 first) from raw [raw_frames][spec.raw_dim]; segs
// ascending by row, the first at or before row0.  Tables longer than one launch's go as several launches.
void splice_rows(const SpliceSpec &spec, int input_dim, const float *raw, int raw_frames, const std::vector<SpliceSeg> &segs,
                 int row0, int rows, float *d_x, hipStream_t s);
// Splices rows [0, rows) through a segment table that is already in device memory (launch_splice_table: d_segs [n_segs][4],
// d_row_seg [rows]): one launch whatever n_segs is.  The scoring loop's batches with a live piece, and nothing else.
void splice_rows_table(const SpliceSpec &spec, int input_dim, const float *raw, int raw_frames, const int32_t *d_segs,
                       const int32_t *d_row_seg, int n_segs, int rows, float *d_x, hipStream_t s);
// Rows [a, b) of one n-frame utterance (host raw frames) into out[b - a][O], spliced by `spec`: through the model's batcher
// when it has one, else the raw frames those rows reference travel once and are spliced and scored chunk by chunk.
// fdnn_calculate_raw on one device, and a group replica's shard.
int calculate_raw_rows(fdnn_model *m, const SpliceRef &spec, const float *raw, int n, int a, int b, float *out);
int group_calculate_raw(fdnn_group *g, const SpliceRef &spec, const float *raw, int n, float *out);  // fdnn_group.cpp
// Rows [a, b) of an n-frame raw utterance through the scoring loop (fdnn_server.cpp); bits (may be null) and out hold
// those rows only.
int server_submit_raw_rows(fdnn_server *s, const SpliceRef &spec, const float *raw, int n, int a, int b, const uint64_t *bits,
                           float *out, uint64_t *ticket);

// ---------------------------------------------------------------- forced alignment (fdnn_align.hip)
// One align call's validated host tables and what is derived from them before anything is launched (align_prepare): the
// transcripts' node sets and columns (align::build_sets), the sets call's tables over the call's rows and the launch plan.
struct AlignJob {
  const fdnn_loglik *ll = nullptr;
  const int32_t *seg_rows = nullptr, *state_ptr = nullptr, *states = nullptr;
  const float *self_lp = nullptr, *next_lp = nullptr;
  int n_segs = 0;
  align::Sets sets;
  std::vector<int32_t> seg_T, row_ld;
  std::vector<long long> row_off;  // segment s's block in the ragged probabilities
  long long nnz = 0;
  int rows = 0;                    // seg_rows[n_segs] - seg_rows[0]
  align::Plan plan;
  sets::Tables tables() const { return {seg_rows, sets.set_ptr.data(), n_segs}; }
};
// FDNN_E_ARG naming the first bad segment (align::check with need_path: T < S is refused), the sum of rows x len past an
// int32 or the take words past align::kMaxScratchBytes; else fills j from its table pointers.  Nothing is launched.
int align_prepare(AlignJob *j, int output_dim, int ctx_rows);
// The context's align buffers made large enough and the tables uploaded on s (the host tables are read before it returns).
int align_stage(fdnn_ctx *c, const AlignJob &j, hipStream_t s);
// The recursion over the probabilities that the sets calls left in c->d_al_probs, then: host = true -- ONE transfer of path
// [rows] and total [n_segs] and s synchronised; false -- both copied to the caller's device buffers on s.
int align_finish(fdnn_ctx *c, const AlignJob &j, int32_t *path, float *total, bool host, hipStream_t s);

// ---------------------------------------------------------------- alignment graphs (fdnn_align_graph.hip)
// One align-graph call's validated host tables and what is derived from them before anything is launched
// (align_graph_prepare): as AlignJob, with the graph's plan.  The sets step is the sibling's (Sink::align_sets into the
// context's align buffers); only the finishing recursion differs.
struct AlignGraphJob {
  const fdnn_loglik *ll = nullptr;
  align_graph::Tables t;
  align::Sets sets;
  std::vector<int32_t> seg_T, row_ld;
  std::vector<long long> row_off;  // segment s's block in the ragged probabilities
  long long nnz = 0;
  int rows = 0;                    // seg_rows[n_segs] - seg_rows[0]
  align_graph::Plan plan;
  sets::Tables tables() const { return {t.seg_rows, sets.set_ptr.data(), t.n_segs}; }
};
// FDNN_E_ARG naming the first bad segment (align_graph::check), the sum of rows x len past an int32 or the back-pointers past
// align_graph::kMaxScratchBytes; else fills j from its table pointers.  Nothing is launched.
int align_graph_prepare(AlignGraphJob *j, int output_dim, int ctx_rows);
// The context's buffers made large enough and the tables uploaded on s (the host tables are read before it returns).
int align_graph_stage(fdnn_ctx *c, const AlignGraphJob &j, hipStream_t s);
// The recursion over the probabilities that the sets calls left in c->d_al_probs, then: host = true -- ONE transfer of path
// [rows] and total [n_segs] and s synchronised; false -- both copied to the caller's device buffers on s.
int align_graph_finish(fdnn_ctx *c, const AlignGraphJob &j, int32_t *path, float *total, bool host, hipStream_t s);

// ---------------------------------------------------------------- alignment graphs, summed (fdnn_fb.hip)
// One forward-backward call's validated host tables and what is derived from them before anything is launched (fb_prepare):
// as AlignGraphJob, with the transposed tables (only where gamma is wanted) and fb's plan.
struct FbJob {
  const fdnn_loglik *ll = nullptr;
  align_graph::Tables t;
  bool want_gamma = false;
  align::Sets sets;
  std::vector<int32_t> seg_T, row_ld, t_ptr, t_src;
  std::vector<float> t_lp;
  std::vector<long long> row_off;  // segment s's block in the ragged probabilities
  long long nnz = 0;
  int rows = 0;                    // seg_rows[n_segs] - seg_rows[0]
  fb::Plan plan;
  sets::Tables tables() const { return {t.seg_rows, sets.set_ptr.data(), t.n_segs}; }
};
// FDNN_E_ARG naming the first bad segment (align_graph::check), the sum of rows x len past an int32 or the lattice past
// fb::kMaxScratchBytes; else fills j from its table pointers and want_gamma.  Nothing is launched.
int fb_prepare(FbJob *j, int output_dim, int ctx_rows);
// The context's buffers made large enough and the tables uploaded on s (the host tables are read before it returns).
int fb_stage(fdnn_ctx *c, const FbJob &j, hipStream_t s);
// The sweeps over the probabilities that the sets calls left in c->d_al_probs, then: host = true -- ONE transfer of total
// [n_segs], and of gamma [sum T S] where asked, and s synchronised; false -- copied to the caller's device buffers on s.
int fb_finish(fdnn_ctx *c, const FbJob &j, float *total, float *gamma, bool host, hipStream_t s);

// ---------------------------------------------------------------- one scoring pass, one chunk loop
// Hidden layers + what the pass's sink asks for, chunk by chunk, on context c and stream s; every pointer a chunk uses comes
// from pass::chunk_view.  Per chunk: the rows in (spliced / uploaded / as they are), host bits up, the hidden layers, the sink's
// step.  Host sinks synchronise s per chunk (also when they fail).  c->n is left at the last chunk's count.
int run_chunks(fdnn_ctx *c, hipStream_t s, const pass::Chunks &chunks, const pass::Pass &p);
// The pooled entry points: ONE pooled context, large enough for the largest chunk; the stream is the caller's where the
// sink is on the device (pass::on_callers_stream), else the context's own; host raw frames travel once, before the loop.
// before / after: steps on the same context and stream inside the same use of it, ahead of the first chunk and behind the
// last (the align calls: tables up, recursion and results down).
using CtxStep = std::function<int(fdnn_ctx *, hipStream_t)>;
int score_chunks(fdnn_model *m, const pass::Chunks &chunks, const pass::Pass &p, hipStream_t callers = nullptr, const CtxStep &before = {},
                 const CtxStep &after = {});

// Ordering between the streams a context is used on.  An event record costs 3-4 us of queue time behind the kernel it
// follows, so a context whose work went to a stream that is certain to exist later -- its own, its owner's, or the null
// stream -- only NOTES that (done_pending); the record is made when a different stream next needs the order (ctx_enter),
// or never.  Work on a caller's stream, which the caller may destroy, is recorded at once as before.
hipError_t ctx_enter(fdnn_ctx *c, hipStream_t s);
void ctx_leave(fdnn_ctx *c, hipStream_t s);
bool stream_is_durable(const fdnn_ctx *c, hipStream_t s);
void ctx_wait_host(fdnn_ctx *c);  // host-side wait for everything ctx_leave covered
void release_ctx(fdnn_ctx *c);    // a pooled context (score_chunks) back to its model's pool
// One use of a context on a stream: enter() is ctx_enter; whichever way the scope is left, the work enqueued in between is
// noted as the context's last (ctx_leave on `s`: a use that ends on another stream than it entered on names it first) and
// a pooled context goes back to its pool.  A use whose enter() failed has enqueued nothing and leaves the notes alone.
struct CtxUse {
  fdnn_ctx *c = nullptr;
  hipStream_t s = nullptr;
  int n_after = -1;  // >= 0: the context's frame count on the way out (a pass that went chunk by chunk)
  bool entered = false;
  CtxUse() = default;
  CtxUse(const CtxUse &) = delete;
  CtxUse &operator=(const CtxUse &) = delete;
  hipError_t enter(fdnn_ctx *ctx, hipStream_t stream) {
    c = ctx;
    s = stream;
    const hipError_t e = ctx_enter(c, s);
    entered = e == hipSuccess;
    return e;
  }
  void leave() {  // (the destructor's work, for a use that ends before its scope does: then the destructor does nothing)
    if (!c) return;
    if (n_after >= 0) c->n = n_after;
    if (entered) ctx_leave(c, s);
    if (c->pooled) release_ctx(c);
    c = nullptr;
  }
  ~CtxUse() { leave(); }
};
// The per-device chain of fused soft-max launches (run_output) notes its last launch the same way: a stream that is about
// to be destroyed must be retired from it first.
void fuse_chain_retire_stream(int device, hipStream_t s);

}  // namespace fdnn
