// fdnn_pass.hpp -- what one scoring pass is: where its rows come from, which mask applies and where its results go, each
// part with an explicit kind; the chunks a pass over many frames is cut into; and the one function that advances a caller's
// base pointers by a chunk's offset.  Arithmetic on pointers and counts, free of HIP (streams stay arguments of the driver,
// run_chunks in fdnn_runtime.cpp): tests/host/pass_check.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "fdnn_lists.hpp"  // lists::rebase_rows
#include "fdnn_sets.hpp"   // sets::Tables, sets::Seg, sets::slice
#include "fdnn_splice_spec.hpp"

struct fdnn_pool;    // (fdnn_internal.hpp: a node -> class map's handle; only its address travels here)
struct fdnn_loglik;  // (fdnn_internal.hpp: a decoder-score handle; likewise)

namespace fdnn::pass {

// ---------------------------------------------------------------- chunks
// A pass over a very large batch runs as chunks (frames are independent: a chunk is a batch of its own, and the scratch
// context only has to hold one).  kRoundFrames = 32 frame tiles of 320 = one workgroup per CU in the 2048-wide hidden
// layers; a chunk is two rounds.  Measured, 125 000 frames (the 8-GPU shard of BASELINE configs[4]), fused soft-max:
// 12.09 M frames/s as one batch (4 GB of result rows, 512 MB of activations per layer: the address-translation and Infinity
// caches stop covering the working set), 12.87 M in chunks of one round, 13.14 M in chunks of two (tools/chunk_bench.py).
using Chunks = std::vector<std::pair<int, int>>;  // (offset, count) pairs of the call's rows
constexpr int kRoundFrames = 10240;
constexpr int kChunkFrames = 2 * kRoundFrames;
constexpr int kChunkTailSplit = 2048;

// The chunk size a measurement switch asks for (FDNN_CHUNK_FRAMES): 0 = never chunk, otherwise whole rounds.
inline int chunk_size(bool set, int frames) {
  const int v = set ? frames : kChunkFrames;
  return v <= 0 ? 0 : std::max(kRoundFrames, v / kRoundFrames * kRoundFrames);
}

// Chunks of `chunk` frames, then what is left as one more batch.  chains(cnt): will the hidden layers of a cnt-frame batch
// run as one chained launch (fdnn_chain.hip)?  A batch whose hidden layers run as a launch per layer (chaining off, fewer
// than two int8 hidden layers, a layer without the validated division) pays one more, nearly empty round of workgroups in
// every layer for a few frames past a whole round -- 11 000 frames as one batch 977 us, as 10 240 + 760: 754 + 150 -- so such
// a tail (up to kChunkTailSplit frames) goes as a small batch of its own.  Chained, the partial round is gone (11 000 frames:
// layer 0 + hidden layers 534 -> 459 us) and a tail costs less inside the batch than as a call of its own
// (tools/chain_sweep.py, tools/batch_sweep.py).
template <class Chains>
Chunks frame_chunks(int n, int chunk, Chains &&chains) {
  Chunks out;
  int off = 0;
  if (chunk > 0)
    for (; n - off > chunk; off += chunk) out.emplace_back(off, chunk);
  const int cnt = n - off, tail = cnt % kRoundFrames;
  if (cnt > kRoundFrames && tail > 0 && tail <= kChunkTailSplit && !chains(cnt)) {
    out.emplace_back(off, cnt - tail);
    out.emplace_back(off + cnt - tail, tail);
  } else {
    out.emplace_back(off, cnt);
  }
  return out;
}

inline Chunks stride_chunks(int n) {  // kChunkFrames strides, no tail split: the host lazy forms
  Chunks out;
  for (int first = 0; first < n; first += kChunkFrames) out.emplace_back(first, std::min(kChunkFrames, n - first));
  return out;
}

// ---------------------------------------------------------------- the three parts of a pass
// Raw feature frames and how the call's rows index them: every chunk splices its rows from the whole buffer (frames is
// never advanced), row0 is the splice row of the call's row 0.
struct Raw {
  const SpliceSpec *spec = nullptr;
  const std::vector<SpliceSeg> *segs = nullptr;
  const float *frames = nullptr;
  int n_frames = 0, row0 = 0;
};

struct Rows {
  // device: [n][D] as they are; host: uploaded chunk by chunk; raw_device / raw_host: spliced chunk by chunk into the
  // context's frame buffer, the host's raw frames uploaded once before the first chunk
  enum Kind { device, host, raw_device, raw_host } kind = device;
  const float *x = nullptr;  // device, host: the call's row 0
  Raw raw;                   // raw_device, raw_host
};

struct Mask {
  // device_bytes: [n][O], non-zero = active (the scoring loop's); device_bits / host_bits: [n][wpr] words (host: uploaded
  // chunk by chunk into the context's d_mask_bits)
  enum Kind { none, device_bytes, device_bits, host_bits } kind = none;
  const int8_t *bytes = nullptr;
  const uint64_t *bits = nullptr;
};

struct Sink {
  enum Kind {
    device_rows,       // rows [n][O] on the device
    host_dense,        // rows [n][O] on the host through dense_pass and its re-run rules
    host_behind_bits,  // rows [n][O] on the host behind host bits: lazy_copy_out
    host_topk,         // the k first-ranked nodes of every row and their values, [n][k] each, through dense_pass
    device_topk,       // the same into device buffers; the rows stay in the context
    host_lists,        // row_ptr [n + 1], nodes [nnz] -> probs [nnz], inactive [n]
    host_set,          // ONE set nodes [len] (null when empty) -> probs [n][len], inactive [n]
    host_sets,         // per-segment sets (tables covering [0, n), all nodes) -> probs (ragged blocks), inactive [n]
    device_sets,       // the same with nodes, probs and inactive on the device (the scoring loop's)
    host_pool,         // every row's class sums under a node -> class map, [n][C], through dense_pass
    device_pool,       // the same into a device buffer; the rows stay in the context
    host_loglik,       // every row as decoder scores under a score handle, [n][O] fp32 or fp16, through dense_pass
    device_loglik,     // the same into a device buffer; the rows stay in the context
    align_sets         // per-segment sets (tables covering [0, n)) into the CONTEXT's align buffers: nodes, probs and inactive
                       // are the context's (fdnn_internal.hpp: d_al_*), the recursion runs behind the last chunk
  } kind = device_rows;
  float *rows = nullptr;
  int k = 0;
  int32_t *topk_nodes = nullptr;
  float *topk_probs = nullptr;
  const int32_t *row_ptr = nullptr, *nodes = nullptr;
  int len = 0;
  sets::Tables sets{nullptr, nullptr, 0};
  float *probs = nullptr, *inactive = nullptr;
  const fdnn_pool *pool = nullptr;  // host_pool, device_pool: the map's handle, its class count C ...
  int pool_classes = 0;
  float *pooled = nullptr;          // ... and the class sums [n][C]
  const fdnn_loglik *loglik = nullptr;  // host_loglik, device_loglik: the score handle, the bytes of one score ...
  size_t score_bytes = 0;
  void *scores = nullptr;               // ... and the scores [n][O]
};

// Device sinks are enqueued on the stream the caller names and not synchronised; host sinks run on the context's own stream
// and return with their results in place.
inline bool on_callers_stream(Sink::Kind k) { return k == Sink::device_rows || k == Sink::device_topk || k == Sink::device_sets || k == Sink::device_pool || k == Sink::device_loglik; }

// One supported pairing of the three, built by name only: what the driver cannot serve cannot be written.
class Pass {
  Pass(const char *w, Rows r, Mask m, Sink s) : who(w), rows(r), mask(m), sink(s) {}
  static Rows rows_of(Rows::Kind k, const float *x) { Rows r; r.kind = k, r.x = x; return r; }
  static Rows rows_of(Rows::Kind k, const Raw &raw) { Rows r; r.kind = k, r.raw = raw; return r; }
  static Mask mask_of(Mask::Kind k, const int8_t *bytes, const uint64_t *bits) { Mask m; m.kind = k, m.bytes = bytes, m.bits = bits; return m; }
  static Sink rows_to(Sink::Kind k, float *rows) { Sink s; s.kind = k, s.rows = rows; return s; }
  static Sink topk_to(Sink::Kind k, int n_best, int32_t *nodes, float *probs) { Sink s; s.kind = k, s.k = n_best, s.topk_nodes = nodes, s.topk_probs = probs; return s; }
  static Sink pool_to(Sink::Kind k, const fdnn_pool *pool, int classes, float *pooled) { Sink s; s.kind = k, s.pool = pool, s.pool_classes = classes, s.pooled = pooled; return s; }
  static Sink loglik_to(Sink::Kind k, const fdnn_loglik *ll, size_t score_bytes, void *scores) { Sink s; s.kind = k, s.loglik = ll, s.score_bytes = score_bytes, s.scores = scores; return s; }
  static Sink entries_to(Sink::Kind k, const int32_t *nodes, float *probs, float *inactive) { Sink s; s.kind = k, s.nodes = nodes, s.probs = probs, s.inactive = inactive; return s; }
  static Sink sets_to(Sink::Kind k, const sets::Tables &t, const int32_t *nodes, float *probs, float *inactive) { Sink s = entries_to(k, nodes, probs, inactive); s.sets = t; return s; }

 public:
  const char *who;  // the entry point's name, for the text of a device error
  Rows rows;
  Mask mask;
  Sink sink;
  // host rows
  static Pass host_dense(const char *who, const float *x, float *out) { return {who, rows_of(Rows::host, x), {}, rows_to(Sink::host_dense, out)}; }
  static Pass host_bits(const char *who, const float *x, const uint64_t *bits, float *out) { return {who, rows_of(Rows::host, x), mask_of(Mask::host_bits, nullptr, bits), rows_to(Sink::host_behind_bits, out)}; }
  static Pass host_topk(const char *who, const float *x, int k, int32_t *nodes, float *probs) { return {who, rows_of(Rows::host, x), {}, topk_to(Sink::host_topk, k, nodes, probs)}; }
  static Pass host_pool(const char *who, const float *x, const fdnn_pool *pool, int classes, float *pooled) { return {who, rows_of(Rows::host, x), {}, pool_to(Sink::host_pool, pool, classes, pooled)}; }
  static Pass host_loglik(const char *who, const float *x, const fdnn_loglik *ll, size_t score_bytes, void *scores) { return {who, rows_of(Rows::host, x), {}, loglik_to(Sink::host_loglik, ll, score_bytes, scores)}; }
  static Pass host_lists(const char *who, const float *x, const int32_t *row_ptr, const int32_t *nodes, float *probs, float *inactive) {
    Sink s = entries_to(Sink::host_lists, nodes, probs, inactive);
    s.row_ptr = row_ptr;
    return {who, rows_of(Rows::host, x), {}, s};
  }
  static Pass host_set(const char *who, const float *x, const int32_t *nodes, int len, float *probs, float *inactive) {
    Sink s = entries_to(Sink::host_set, nodes, probs, inactive);
    s.len = len;
    return {who, rows_of(Rows::host, x), {}, s};
  }
  static Pass host_align(const char *who, const float *x, const sets::Tables &t) { return {who, rows_of(Rows::host, x), {}, sets_to(Sink::align_sets, t, nullptr, nullptr, nullptr)}; }
  static Pass raw_align(const char *who, const Raw &raw, const sets::Tables &t) { return {who, rows_of(Rows::raw_host, raw), {}, sets_to(Sink::align_sets, t, nullptr, nullptr, nullptr)}; }
  static Pass host_sets(const char *who, const float *x, const sets::Tables &t, const int32_t *nodes, float *probs, float *inactive) { return {who, rows_of(Rows::host, x), {}, sets_to(Sink::host_sets, t, nodes, probs, inactive)}; }
  // raw frames on the host
  static Pass raw_dense(const char *who, const Raw &raw, float *out) { return {who, rows_of(Rows::raw_host, raw), {}, rows_to(Sink::host_dense, out)}; }
  static Pass raw_bits(const char *who, const Raw &raw, const uint64_t *bits, float *out) { return {who, rows_of(Rows::raw_host, raw), mask_of(Mask::host_bits, nullptr, bits), rows_to(Sink::host_behind_bits, out)}; }
  static Pass raw_topk(const char *who, const Raw &raw, int k, int32_t *nodes, float *probs) { return {who, rows_of(Rows::raw_host, raw), {}, topk_to(Sink::host_topk, k, nodes, probs)}; }
  static Pass raw_pool(const char *who, const Raw &raw, const fdnn_pool *pool, int classes, float *pooled) { return {who, rows_of(Rows::raw_host, raw), {}, pool_to(Sink::host_pool, pool, classes, pooled)}; }
  static Pass raw_loglik(const char *who, const Raw &raw, const fdnn_loglik *ll, size_t score_bytes, void *scores) { return {who, rows_of(Rows::raw_host, raw), {}, loglik_to(Sink::host_loglik, ll, score_bytes, scores)}; }
  // rows or raw frames on the device
  static Pass device_dense(const char *who, const float *d_x, float *d_out) { return {who, rows_of(Rows::device, d_x), {}, rows_to(Sink::device_rows, d_out)}; }
  static Pass device_bits(const char *who, const float *d_x, const uint64_t *d_bits, float *d_out) { return {who, rows_of(Rows::device, d_x), mask_of(Mask::device_bits, nullptr, d_bits), rows_to(Sink::device_rows, d_out)}; }
  static Pass device_topk(const char *who, const float *d_x, int k, int32_t *d_nodes, float *d_probs) { return {who, rows_of(Rows::device, d_x), {}, topk_to(Sink::device_topk, k, d_nodes, d_probs)}; }
  static Pass device_pool(const char *who, const float *d_x, const fdnn_pool *pool, int classes, float *d_pooled) { return {who, rows_of(Rows::device, d_x), {}, pool_to(Sink::device_pool, pool, classes, d_pooled)}; }
  static Pass device_loglik(const char *who, const float *d_x, const fdnn_loglik *ll, size_t score_bytes, void *d_scores) { return {who, rows_of(Rows::device, d_x), {}, loglik_to(Sink::device_loglik, ll, score_bytes, d_scores)}; }
  static Pass raw_device_dense(const char *who, const Raw &d_raw, float *d_out) { return {who, rows_of(Rows::raw_device, d_raw), {}, rows_to(Sink::device_rows, d_out)}; }
  // the scoring loop's batches, already on the device: one mask or none (bits win), or the pieces' sets
  static Pass loop_rows(const float *d_x, const int8_t *d_masks, const uint64_t *d_bits, float *d_out) {
    return {"scoring loop", rows_of(Rows::device, d_x), mask_of(d_bits ? Mask::device_bits : d_masks ? Mask::device_bytes : Mask::none, d_masks, d_bits), rows_to(Sink::device_rows, d_out)};
  }
  static Pass loop_sets(const float *d_x, const sets::Tables &t, const int32_t *d_nodes, float *d_probs, float *d_inactive) { return {"scoring loop", rows_of(Rows::device, d_x), {}, sets_to(Sink::device_sets, t, d_nodes, d_probs, d_inactive)}; }
};

// ---------------------------------------------------------------- one chunk of a pass
struct Dims {
  size_t D, O, wpr;  // input width, output width, mask words per row
};

// Every pointer and count that rows [off, off + cnt) of the call use: the ONLY place where a caller's base pointer is advanced
// by a chunk offset.  Null / zero where the pass has no such part.
struct ChunkView {
  int cnt = 0;
  const float *x = nullptr;  // device, host rows
  int splice_row = 0;        // raw rows: the splice row of the chunk's row 0
  const int8_t *bytes = nullptr;
  const uint64_t *bits = nullptr;
  float *rows = nullptr;
  int32_t *topk_nodes = nullptr;
  float *topk_probs = nullptr;
  float *pooled = nullptr;
  void *scores = nullptr;
  // lists, set, sets: the chunk's entries as a call of its own
  std::vector<int32_t> row_ptr;  // lists: the chunk's slice rebased to 0 (lists::rebase_rows)
  std::vector<sets::Seg> segs;   // sets: the chunk's slice (sets::slice); its blocks are one contiguous range from probs on
  const int32_t *nodes = nullptr;
  int n_nodes = 0;               // nodes that travel with the chunk
  float *probs = nullptr, *inactive = nullptr;
};

inline ChunkView chunk_view(const Pass &p, const Dims &d, int off_, int cnt) {
  const size_t off = size_t(off_);
  const Sink &to = p.sink;
  ChunkView v;
  v.cnt = cnt;
  if (p.rows.kind == Rows::device || p.rows.kind == Rows::host) v.x = p.rows.x + off * d.D;
  else v.splice_row = p.rows.raw.row0 + off_;
  if (p.mask.bytes) v.bytes = p.mask.bytes + off * d.O;
  if (p.mask.bits) v.bits = p.mask.bits + off * d.wpr;
  if (to.rows) v.rows = to.rows + off * d.O;
  if (to.k) v.topk_nodes = to.topk_nodes + off * size_t(to.k), v.topk_probs = to.topk_probs + off * size_t(to.k);
  if (to.pooled) v.pooled = to.pooled + off * size_t(to.pool_classes);
  if (to.scores) v.scores = static_cast<char *>(to.scores) + off * d.O * to.score_bytes;
  if (to.inactive) v.inactive = to.inactive + off;
  if (to.kind == Sink::host_lists) {  // the chunk's slice of the lists as lists of its own
    lists::rebase_rows(to.row_ptr, off_, cnt, &v.row_ptr);
    const size_t e0 = size_t(to.row_ptr[off]);
    v.nodes = to.nodes + e0, v.n_nodes = v.row_ptr[size_t(cnt)], v.probs = to.probs + e0;
  } else if (to.kind == Sink::host_set) {  // one node set for every chunk: the chunk's rows land at probs + off * len
    v.nodes = to.nodes, v.n_nodes = to.len, v.probs = to.probs + off * size_t(to.len);
  } else if (to.kind == Sink::host_sets || to.kind == Sink::device_sets) {  // all nodes travel; set_off indexes them
    v.segs = sets::slice(to.sets, off_, off_ + cnt);
    v.nodes = to.nodes, v.n_nodes = to.sets.set_ptr[to.sets.n_segs];
    v.probs = to.probs + (v.segs.empty() ? 0 : size_t(v.segs[0].src_off));
  } else if (to.kind == Sink::align_sets) {  // the bases are the context's: the driver adds the slice's src_off
    v.segs = sets::slice(to.sets, off_, off_ + cnt);
    v.n_nodes = to.sets.set_ptr[to.sets.n_segs];
  }
  return v;
}

}  // namespace fdnn::pass
