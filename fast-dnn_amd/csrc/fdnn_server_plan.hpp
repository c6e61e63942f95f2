// fdnn_server_plan.hpp -- what one batch of the scoring loop (fdnn_server.cpp) contains: which queued requests, or parts of
// them, share it, each piece's rows and caller pointers, for raw submissions where a piece's raw frames are staged and how
// its rows index them, the batch's FORM -- what goes up beside the frames, which pass runs, what is launched behind it,
// the one transfer that brings the results to the host -- and how a piece's part of that transfer reaches its caller.
// Arithmetic on the queue and on host memory, free of HIP: tests/host/server_plan_check.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <utility>
#include <vector>

#include "fdnn_splice_spec.hpp"

struct fdnn_pool;    // (fdnn_internal.hpp: a node -> class map's handle; only its address travels here)
struct fdnn_loglik;  // (fdnn_internal.hpp: a decoder-score handle; likewise)

namespace fdnn::plan {

// A set submission's node set, copied at submit and shared by the request, its parts and their pieces (as SpliceRef is)
using SetRef = std::shared_ptr<const std::vector<int32_t>>;
// A live push's window of raw frames [frames][raw_dim], copied at the push and shared the same way
using WindowRef = std::shared_ptr<const std::vector<float>>;

// ---------------------------------------------------------------- the two parts of a request
// Where a request's frames come from.  Built by name only.
class Frames {
  Frames() = default;

 public:
  enum Kind { host_rows, raw_frames } kind = host_rows;
  const float *x = nullptr;  // host_rows: [n][D]
  // raw: rows [raw_a, raw_a + n) of the raw_n-frame utterance at `raw`, spliced on the device by the spec the request was
  // submitted with
  const float *raw = nullptr;
  SpliceRef spec;
  int raw_n = 0, raw_a = 0;
  // live pushes (fdnn_server_live_*): the "utterance" is the push's window -- the frames its handle had kept plus the new
  // ones, copied at the push -- and the request, its parts and their batches own it: `raw` points into it.  Null otherwise:
  // the caller keeps its frames valid.
  WindowRef window;
  static Frames rows(const float *x) { Frames f; f.x = x; return f; }
  static Frames raw_rows(const float *raw, const SpliceRef &spec, int raw_n, int raw_a) { Frames f; f.kind = raw_frames, f.raw = raw, f.spec = spec, f.raw_n = raw_n, f.raw_a = raw_a; return f; }
  static Frames live_rows(WindowRef window, const SpliceRef &spec, int raw_n, int raw_a) {
    Frames f = raw_rows(window->data(), spec, raw_n, raw_a);
    f.window = std::move(window);
    return f;
  }
};

// What the caller wants back, for n rows.  One named constructor per kind, as fdnn::pass::Pass has: nothing reads a kind
// off a pointer that is set or null.  The same type describes a request's n rows and a piece's rows (want_at).
class Want {
  Want() = default;

 public:
  enum Kind { rows = 0, rows_behind_bytes = 1, rows_behind_bits = 2, set = 3, topk = 4, pool = 5, loglik = 6 } kind = rows;
  // rows, rows_behind_bytes, rows_behind_bits: soft-max rows out [n][O]; behind byte masks [n][O] (non-zero = active) or bit
  // words [n][ceil(O / 64)], and for bits the largest number of active nodes in any row (widest_row, counted by the submitter)
  float *out = nullptr;
  const int8_t *masks = nullptr;
  const uint64_t *bits = nullptr;
  int most = 0;
  // set: ONE node set for all n rows; probs [n][len] (null when the set is empty), inactive [n]
  SetRef nodes;
  float *probs = nullptr, *inactive = nullptr;
  // topk: the k first-ranked nodes of every row and their values, [n][k] each
  int k = 0;
  int32_t *topk_nodes = nullptr;
  float *topk_probs = nullptr;
  // pool: every row's class sums under the map behind `map`, which has `classes` classes; pooled [n][classes]
  const fdnn_pool *map = nullptr;
  int classes = 0;
  float *pooled = nullptr;
  // loglik: every row as decoder scores under the handle behind `score`, `score_bytes` (4 or 2) a score; scores [n][O]
  const fdnn_loglik *score = nullptr;
  size_t score_bytes = 0;
  void *scores = nullptr;

  static Want rows_to(float *out) { Want w; w.out = out; return w; }
  static Want rows_behind_bytes_to(const int8_t *masks, float *out) { Want w; w.kind = rows_behind_bytes, w.masks = masks, w.out = out; return w; }
  static Want rows_behind_bits_to(const uint64_t *bits, int most, float *out) { Want w; w.kind = rows_behind_bits, w.bits = bits, w.most = most, w.out = out; return w; }
  static Want set_to(SetRef nodes, float *probs, float *inactive) { Want w; w.kind = set, w.nodes = std::move(nodes), w.probs = probs, w.inactive = inactive; return w; }
  static Want topk_to(int k, int32_t *nodes, float *probs) { Want w; w.kind = topk, w.k = k, w.topk_nodes = nodes, w.topk_probs = probs; return w; }
  static Want pool_to(const fdnn_pool *map, int classes, float *pooled) { Want w; w.kind = pool, w.map = map, w.classes = classes, w.pooled = pooled; return w; }
  static Want loglik_to(const fdnn_loglik *score, size_t score_bytes, void *scores) { Want w; w.kind = loglik, w.score = score, w.score_bytes = score_bytes, w.scores = scores; return w; }
};

// The Want of the rows behind the first `taken` of a request: the ONLY place where a caller's destination (and the masks that
// go with its rows) is advanced by the rows that earlier batches took -- the counterpart of fdnn::pass::chunk_view.
inline Want want_at(const Want &w, int taken, size_t O, size_t wpr) {
  Want p = w;
  const size_t t = size_t(taken);
  switch (w.kind) {
    case Want::rows: p.out += t * O; break;
    case Want::rows_behind_bytes: p.out += t * O, p.masks += t * O; break;
    case Want::rows_behind_bits: p.out += t * O, p.bits += t * wpr; break;
    case Want::set:
      if (p.probs) p.probs += t * w.nodes->size();
      p.inactive += t;
      break;
    case Want::topk: p.topk_nodes += t * size_t(w.k), p.topk_probs += t * size_t(w.k); break;
    case Want::pool: p.pooled += t * size_t(w.classes); break;
    case Want::loglik: p.scores = static_cast<char *>(w.scores) + t * O * w.score_bytes; break;
  }
  return p;
}

struct Request {
  uint64_t ticket = 0;  // (given by the scoring loop's submit_host)
  Frames frames;
  Want want;
  int n = 0;
  int taken = 0;  // frames already packed into earlier batches
  Request(Frames f, Want w, int rows) : frames(std::move(f)), want(std::move(w)), n(rows) {}
};

struct Piece {  // one caller's rows inside a coalesced batch
  uint64_t ticket;
  int row0, rows;  // rows [row0, row0 + rows) of the batch
  bool last;       // the ticket's final piece
  Want want;       // of these rows (want_at)
  // set batches: the piece is one segment of the batch's sets call -- where its set is staged among the batch's nodes, and
  // where its block [rows][len] starts inside the batch's probs
  int set_off = 0, block_off = 0;
  int state = 0;  // 0 batch in flight, 1 rows ready in the slot's landing buffer, 2 being copied out, 3 done
};

// raw batches, per piece: the raw frames it references, [first, first + count) of its utterance, at frame `at` of the slot's buffer
struct RawSrc { int first, count, at; };

// The widest row of a bit-mask request, counted on the submitting thread: the batch's compacted row length follows from it.
inline int widest_row(const uint64_t *bits, int n, size_t O) {
  const size_t wpr = (O + 63) / 64;
  const uint64_t tail_mask = (O & 63) ? ((uint64_t(1) << (O & 63)) - 1) : ~uint64_t(0);
  int most = 0;
  for (int f = 0; f < n; ++f) {
    const uint64_t *row = bits + size_t(f) * wpr;
    int k = 0;
    for (size_t w = 0; w + 1 < wpr; ++w) k += __builtin_popcountll(row[w]);
    k += __builtin_popcountll(row[wpr - 1] & tail_mask);
    most = std::max(most, k);
  }
  return most;
}

// ---------------------------------------------------------------- a batch and its form
// What every step behind the plan needs to know of a batch, fixed when the batch is planned: the steps follow it and do not
// ask for the batch's kind again.  `leave` names the row of the table:
//
//   leave             | behind the pass | the one transfer: source        | words (32 bit)
//   by_caller_copies  | nothing         | none (a single caller's whole rows: copied from d_out by whoever waits)
//   whole_rows        | nothing         | d_out                           | rows * O
//   compacted_rows    | compact         | d_comp                          | rows * stride
//   set_blocks        | nothing         | d_out                           | nnz + rows
//   topk_pairs        | select_topk     | the device result buffer        | 2 * rows * topk_k
//   class_sums        | pool_sums       | the device result buffer        | rows * pool_classes
//   scores            | loglik_scores   | the device result buffer        | ceil(rows * O * score_bytes / 4)
struct Form {
  enum Upload { no_upload, byte_masks, bit_words, node_sets } upload = no_upload;  // what goes up beside the frames ...
  size_t upload_bytes = 0;                                                         // ... and how much of it
  enum PassKind { loop_rows, loop_sets } pass = loop_rows;                         // fdnn::pass::Pass::loop_rows / loop_sets
  enum Behind { nothing, compact, select_topk, pool_sums, loglik_scores } behind = nothing;       // launched over all rows behind the chunks
  enum Leave { by_caller_copies, whole_rows, compacted_rows, set_blocks, topk_pairs, class_sums, scores } leave = by_caller_copies;
  size_t words = 0;  // of the one result transfer
};

struct BatchPlan {
  std::vector<Request> taken;  // per piece: the request with .taken = first frame, .n = frames in THIS batch
  std::vector<Piece> pieces;
  std::vector<RawSrc> raw_src;  // raw batches: per piece
  std::vector<SpliceSeg> segs;  // raw batches: per piece (its own utterance's edges)
  SpliceRef spec;               // raw batches: one spec per batch
  Want::Kind kind = Want::rows;  // of all its requests, except that rows ride in a rows_behind_bytes batch (may_join)
  int rows = 0, raw_frames = 0, most = 0, stride = 0;  // stride: floats per compacted row (0: the rows leave whole)
  bool any_mask = false, raw = false;
  bool live = false;  // raw batches: a piece is a live push -- the batch has about one segment per push, hundreds of them, and
                      // is spliced through the segment table in device memory (live_table)
  int nnz = 0, set_nodes = 0;  // set batches: the floats of the batch's probs (sum of rows x len) and the nodes of its pieces' sets
  int topk_k = 0;              // top-k batches: the largest k among its pieces (a smaller k's result is a prefix of it)
  const fdnn_pool *pool = nullptr;  // pool batches: the one handle of all its pieces ...
  int pool_classes = 0;             // ... and its class count
  const fdnn_loglik *score = nullptr;  // loglik batches: the one handle of all its pieces ...
  size_t score_bytes = 0;              // ... and the bytes of one score
  Form form;
};

// May this request join this (non-empty) batch?  Kinds do not share a batch, except that dense callers ride in a byte-mask
// batch (all active), which makes the batch a byte-mask batch
// -- bit-mask requests share only with bit-mask requests (one masked pass, the rows compacted)
// -- set requests (no output layer runs, fdnn_sets.hip scores each piece's set) only with set requests
// -- top-k requests (a dense batch whose rows stay on the device, fdnn_topk.hip selects from them) only with top-k requests
// -- pool requests (a dense batch whose rows stay on the device, fdnn_pool.hip sums them by class) only with pool requests
//    of the SAME handle
// -- loglik requests (a dense batch whose rows stay on the device, fdnn_loglik.hip turns them into decoder scores) only with
//    loglik requests of the SAME handle
// and in every case raw-frame requests only with raw-frame requests, under one spec object.
inline bool may_join(const BatchPlan &b, const Request &r) {
  if ((r.frames.kind == Frames::raw_frames) != b.raw || r.frames.spec != b.spec) return false;
  switch (r.want.kind) {
    case Want::rows:
    case Want::rows_behind_bytes: return b.kind == Want::rows || b.kind == Want::rows_behind_bytes;
    case Want::rows_behind_bits:
    case Want::set:
    case Want::topk: return b.kind == r.want.kind;
    case Want::pool: return b.kind == Want::pool && b.pool == r.want.map;
    case Want::loglik: return b.kind == Want::loglik && b.score == r.want.score;
  }
  return false;
}

// One row of the form table: how the batch's results leave, and with that what runs behind the pass and the transfer's size.
inline void set_leave(BatchPlan &b, Form::Leave leave, size_t O) {
  Form &f = b.form;
  const size_t rows = size_t(b.rows);
  f.leave = leave;
  switch (leave) {
    case Form::by_caller_copies: f.behind = Form::nothing, f.words = 0; break;
    case Form::whole_rows: f.behind = Form::nothing, f.words = rows * O; break;
    case Form::compacted_rows: f.behind = Form::compact, f.words = rows * size_t(b.stride); break;
    case Form::set_blocks: f.behind = Form::nothing, f.words = size_t(b.nnz) + rows; break;
    case Form::topk_pairs: f.behind = Form::select_topk, f.words = 2 * rows * size_t(b.topk_k); break;
    case Form::class_sums: f.behind = Form::pool_sums, f.words = rows * size_t(b.pool_classes); break;
    case Form::scores: f.behind = Form::loglik_scores, f.words = (rows * O * b.score_bytes + 3) / 4; break;
  }
}

// The loop found no room for what the form's transfer needs (the compacted pair, or the pinned landing buffer of whole
// rows): the batch's rows go back whole, copied from the device caller by caller.  Rows batches only.
inline void leave_by_caller_copies(BatchPlan &b) {
  b.stride = 0;
  set_leave(b, Form::by_caller_copies, 0);
}

// Takes requests off the front of the queue, whole or in part, until the batch is full (max_frames rows) or the next one may
// not join it (may_join), and fixes the batch's form.  Request::taken advances in the queue; a finished request leaves it.
inline BatchPlan plan_batch(std::deque<Request> &queue, int max_frames, size_t O) {
  BatchPlan b;
  const size_t wpr = (O + 63) / 64;
  while (!queue.empty() && b.rows < max_frames) {
    Request &r = queue.front();
    if (b.rows == 0) {
      b.kind = r.want.kind;
      b.raw = r.frames.kind == Frames::raw_frames;
      b.spec = r.frames.spec;
      b.pool = r.want.map, b.pool_classes = r.want.classes;
      b.score = r.want.score, b.score_bytes = r.want.score_bytes;
    } else if (!may_join(b, r)) {
      break;
    }
    const int take = std::min(r.n - r.taken, max_frames - b.rows);
    Request part = r;
    part.n = take;  // rows of this request in THIS batch
    b.taken.push_back(part);
    r.taken += take;
    const bool last = r.taken == r.n;
    Piece pc{r.ticket, b.rows, take, last, want_at(r.want, part.taken, O, wpr)};
    switch (r.want.kind) {  // what the batch accumulates across its pieces
      case Want::rows: break;
      case Want::rows_behind_bytes: b.kind = Want::rows_behind_bytes, b.any_mask = true; break;
      case Want::rows_behind_bits: b.most = std::max(b.most, r.want.most); break;
      case Want::set: {
        const int len = int(r.want.nodes->size());
        pc.set_off = b.set_nodes, pc.block_off = b.nnz;
        b.set_nodes += len;
        b.nnz += take * len;
        break;
      }
      case Want::topk: b.topk_k = std::max(b.topk_k, r.want.k); break;
      case Want::pool: break;
      case Want::loglik: break;
    }
    b.pieces.push_back(std::move(pc));
    if (b.raw) {  // the raw frames this piece's rows reference, and where they are staged
      b.live |= r.frames.window != nullptr;
      const int u0 = r.frames.raw_a + part.taken;  // the piece's first row as a frame of its utterance
      int fa, fb;
      splice_halo(*r.frames.spec, r.frames.raw_n, u0, u0 + take, &fa, &fb);
      b.raw_src.push_back(RawSrc{fa, fb - fa, b.raw_frames});
      b.segs.push_back(SpliceSeg{b.rows, b.raw_frames + u0 - fa, b.raw_frames - fa, b.raw_frames + r.frames.raw_n - 1 - fa});
      b.raw_frames += fb - fa;
    }
    b.rows += take;
    if (last) queue.pop_front();
  }
  // Whole rows of a batch that several callers share go to the host in one transfer (1 GB of pinned memory per slot at
  // most); a single caller's batch leaves by per-caller copies from the device.
  const Form::Leave whole = b.taken.size() > 1 && size_t(max_frames) * O * sizeof(float) <= (size_t(1) << 30) ? Form::whole_rows : Form::by_caller_copies;
  const size_t rows = size_t(b.rows);
  Form &f = b.form;
  switch (b.kind) {
    case Want::rows: set_leave(b, whole, O); break;
    case Want::rows_behind_bytes:
      f.upload = Form::byte_masks, f.upload_bytes = rows * O;
      set_leave(b, whole, O);
      break;
    case Want::rows_behind_bits: {
      f.upload = Form::bit_words, f.upload_bytes = rows * wpr * sizeof(uint64_t);
      // compacted return: worth it while a row is at most 3/4 active nodes
      const size_t stride = size_t(b.most) + 1;
      b.stride = stride * 4 <= O * 3 ? int(stride) : 0;
      set_leave(b, b.stride > 0 ? Form::compacted_rows : whole, O);
      break;
    }
    case Want::set:
      f.upload = Form::node_sets, f.upload_bytes = size_t(b.set_nodes) * sizeof(int32_t);
      f.pass = Form::loop_sets;
      set_leave(b, Form::set_blocks, O);
      break;
    case Want::topk: set_leave(b, Form::topk_pairs, O); break;
    case Want::pool: set_leave(b, Form::class_sums, O); break;
    case Want::loglik: set_leave(b, Form::scores, O); break;
  }
  return b;
}

// A live batch's segment table, staged behind the raw frames in the slot's buffer and uploaded with them in the same copy.
// In 32-bit words of that buffer: the raw frames [0, raw_frames * raw_dim); from `segs_at` (the next multiple of four words:
// the kernel reads a segment as one 16-byte load) the segments as (row, center, lo, hi), four words each; from `row_seg_at`
// one word per row of the batch, the index of the row's segment.  `words`: all of it.
struct LiveTable {
  size_t segs_at = 0, row_seg_at = 0, words = 0;
};
inline LiveTable live_table(const BatchPlan &b) {
  LiveTable t;
  t.segs_at = (size_t(b.raw_frames) * size_t(b.spec->raw_dim) + 3) & ~size_t(3);
  t.row_seg_at = t.segs_at + 4 * b.segs.size();
  t.words = t.row_seg_at + size_t(b.rows);
  return t;
}
inline void write_live_table(const BatchPlan &b, const LiveTable &t, int32_t *buffer) {
  for (size_t g = 0; g < b.segs.size(); ++g) {
    const SpliceSeg &sg = b.segs[g];
    int32_t *w = buffer + t.segs_at + 4 * g;
    w[0] = sg.row, w[1] = sg.center, w[2] = sg.lo, w[3] = sg.hi;
    const int end = g + 1 < b.segs.size() ? b.segs[g + 1].row : b.rows;
    for (int r = sg.row; r < end; ++r) buffer[t.row_seg_at + size_t(r)] = int32_t(g);
  }
}

// A piece's part of the batch's one transfer, from the slot's landing buffer (form.words 32-bit words, as the device wrote
// them) into the caller's memory.  Compacted rows are expanded by `expand` -- fdnn::lazy_expand_rows_from's signature -- which
// is handed the piece's first compacted row and the batch's stride.  (by_caller_copies: nothing has landed; the loop copies
// from the device.)
template <class Expand>
inline void scatter(const BatchPlan &b, const Piece &p, const void *landing, size_t O, Expand &&expand) {
  const Want &w = p.want;
  const size_t row0 = size_t(p.row0), rows = size_t(p.rows), word = sizeof(uint32_t);
  const auto at = [&](size_t i) { return static_cast<const char *>(landing) + i * word; };
  switch (b.form.leave) {
    case Form::by_caller_copies: break;
    case Form::whole_rows:  // [rows][O]: this thread moves its own
      std::memcpy(w.out, at(row0 * O), word * rows * O);
      break;
    case Form::compacted_rows: {  // [rows][stride]; THIS thread -- the caller's own, normally -- expands its rows into the caller's block
      const size_t stride = size_t(b.stride);
      expand(w.out, static_cast<const float *>(landing) + row0 * stride, p.rows, O, stride, w.bits);
      break;
    }
    case Form::set_blocks: {  // the pieces' blocks [rows][len] back to back, then one inactive value per row of the batch
      const size_t len = w.nodes->size();
      if (len) std::memcpy(w.probs, at(size_t(p.block_off)), word * rows * len);
      std::memcpy(w.inactive, at(size_t(b.nnz) + row0), word * rows);
      break;
    }
    case Form::topk_pairs: {  // nodes [rows][k_b], then values [rows][k_b]: the piece keeps the first k of its rows' k_b columns
      const size_t kb = size_t(b.topk_k), k = size_t(w.k), all = size_t(b.rows) * kb;
      for (size_t r = 0; r < rows; ++r) {
        std::memcpy(w.topk_nodes + r * k, at((row0 + r) * kb), word * k);
        std::memcpy(w.topk_probs + r * k, at(all + (row0 + r) * kb), word * k);
      }
      break;
    }
    case Form::class_sums: {  // [rows][C]
      const size_t C = size_t(b.pool_classes);
      std::memcpy(w.pooled, at(row0 * C), word * rows * C);
      break;
    }
    case Form::scores:  // [rows][O] scores of score_bytes each: a piece's rows start at a byte, not a word, of the landing buffer
      std::memcpy(w.scores, static_cast<const char *>(landing) + row0 * O * b.score_bytes, rows * O * b.score_bytes);
      break;
  }
}

}  // namespace fdnn::plan
