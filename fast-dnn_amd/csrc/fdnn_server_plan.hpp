// fdnn_server_plan.hpp -- what one batch of the scoring loop (fdnn_server.cpp) contains: which queued requests, or parts of
// them, share it, each piece's rows and caller pointers, and for raw submissions where a piece's raw frames are staged and how
// its rows index them.  Arithmetic on the queue, free of HIP: tests/host/server_plan_check.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <deque>
#include <memory>
#include <vector>

#include "fdnn_splice_spec.hpp"

struct fdnn_pool;  // (fdnn_internal.hpp: a node -> class map's handle; only its address travels here)

namespace fdnn::plan {

// A set submission's node set, copied at submit and shared by the request, its parts and their pieces (as SpliceRef is)
using SetRef = std::shared_ptr<const std::vector<int32_t>>;

struct Piece {  // one caller's rows inside a coalesced batch
  uint64_t ticket;
  float *out;      // caller's destination of these rows
  int row0, rows;  // rows [row0, row0 + rows) of the batch
  bool last;       // the ticket's final piece
  int state = 0;   // 0 batch in flight, 1 rows ready in the slot's pinned buffer, 2 being copied out, 3 done
  const uint64_t *bits = nullptr;  // lazy submissions with bit masks: the caller's words of these rows (compacted return)
  // set submissions (then out is null): the piece is one segment of the batch's sets call -- its set, where the set is
  // staged among the batch's nodes, its block [rows][len] inside the batch's probs, and the caller's destinations of
  // these rows (advanced by the frames earlier batches took)
  SetRef set;
  int set_off = 0, block_off = 0;
  float *probs = nullptr, *inactive = nullptr;
  // top-k submissions (then out is null): the piece's own k and the caller's [rows][k] destinations of these rows (advanced
  // by the frames earlier batches took); the batch selects with its largest k and a piece keeps the first k columns
  int topk = 0;
  int32_t *topk_nodes = nullptr;
  float *topk_probs = nullptr;
  // pool submissions (then out is null): the caller's [rows][C] destination of these rows (advanced by the frames earlier
  // batches took); C is the batch's
  float *pooled = nullptr;
};

struct Request {
  uint64_t ticket = 0;            // (given by the scoring loop's submit_host)
  const float *x = nullptr;
  const int8_t *masks = nullptr;  // may be null
  float *out = nullptr;
  int n = 0;
  int taken = 0;  // frames already packed into earlier batches
  const uint64_t *bits = nullptr;  // fdnn_server_submit_lazy_bits: [n][ceil(O / 64)] (then masks is null)
  int most = 0;                    // ... and the largest number of active nodes in any of its rows (counted by the submitter)
  // raw submissions (then x is null): rows [raw_a, raw_a + n) of the raw_n-frame utterance at `raw`, spliced on the device by
  // the spec the request was submitted with
  const float *raw = nullptr;
  SpliceRef spec;
  int raw_n = 0, raw_a = 0;
  // set submissions (then out, masks and bits are null): ONE node set for all n rows; results probs [n][len], inactive [n]
  SetRef set;
  float *set_probs = nullptr, *set_inactive = nullptr;
  // top-k submissions (then out, masks, bits and set are null): the k first-ranked nodes of every row; results [n][topk] each
  int topk = 0;
  int32_t *topk_nodes = nullptr;
  float *topk_probs = nullptr;
  // pool submissions (then out, masks, bits, set and topk are null): every row's class sums under the map behind `pool`, which
  // has pool_classes classes; results pooled [n][pool_classes]
  const fdnn_pool *pool = nullptr;
  int pool_classes = 0;
  float *pooled = nullptr;
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

// what a host batch carries: kinds do not share a batch, except that dense callers may ride in a byte-mask batch (all active)
// -- and set requests (kSet: no output layer runs, fdnn_sets.hip scores each piece's set) share batches only with set requests
// -- and top-k requests (kTopk: a dense batch whose rows stay on the device, fdnn_topk.hip selects from them) only with top-k requests
// -- and pool requests (kPool: a dense batch whose rows stay on the device, fdnn_pool.hip sums them by class) only with pool
// requests of the SAME handle
enum BatchKind { kDense = 0, kBytes = 1, kBits = 2, kSet = 3, kTopk = 4, kPool = 5 };
inline int kind_of(const Request &r) { return r.pool ? kPool : r.topk ? kTopk : r.set ? kSet : r.bits ? kBits : r.masks ? kBytes : kDense; }

struct BatchPlan {
  std::vector<Request> taken;  // per piece: the request with .taken = first frame, .n = frames in THIS batch
  std::vector<Piece> pieces;
  std::vector<RawSrc> raw_src;  // raw batches: per piece
  std::vector<SpliceSeg> segs;  // raw batches: per piece (its own utterance's edges)
  SpliceRef spec;               // raw batches: one spec per batch
  int rows = 0, raw_frames = 0, most = 0, kind = kDense, stride = 0;  // stride: floats per compacted row (0: the rows leave whole)
  bool any_mask = false, raw = false;
  int nnz = 0, set_nodes = 0;  // set batches: the floats of the batch's probs (sum of rows x len) and the nodes of its pieces' sets
  int topk_k = 0;              // top-k batches: the largest k among its pieces (a smaller k's result is a prefix of it)
  const fdnn_pool *pool = nullptr;  // pool batches: the one handle of all its pieces ...
  int pool_classes = 0;             // ... and its class count
};

// Takes requests off the front of the queue, whole or in part, until the batch is full (max_frames rows) or the next one may
// not join it.  A batch carries bit-mask requests only, or none (dense rows in a byte-mask batch get all-active masks);
// raw-frame requests only, or none; and one spec object.  Request::taken advances in the queue; a finished request leaves it.
inline BatchPlan plan_batch(std::deque<Request> &queue, int max_frames, size_t O) {
  BatchPlan b;
  const size_t wpr = (O + 63) / 64;
  while (!queue.empty() && b.rows < max_frames) {
    Request &r = queue.front();
    const int rk = kind_of(r);
    if (b.rows == 0) {
      b.kind = rk;
      b.raw = r.raw != nullptr;
      b.spec = r.spec;
      b.pool = r.pool, b.pool_classes = r.pool_classes;
    } else if ((rk == kBits) != (b.kind == kBits) || (rk == kSet) != (b.kind == kSet) || (rk == kTopk) != (b.kind == kTopk) || (rk == kPool) != (b.kind == kPool) || r.pool != b.pool || (r.raw != nullptr) != b.raw || r.spec != b.spec)
      break;
    else if (rk == kBytes)
      b.kind = kBytes;
    b.most = std::max(b.most, r.most);
    const int take = std::min(r.n - r.taken, max_frames - b.rows);
    Request part = r;
    part.n = take;  // rows of this request in THIS batch
    b.taken.push_back(part);
    b.any_mask |= r.masks != nullptr;
    r.taken += take;
    const bool last = r.taken == r.n;
    b.pieces.push_back(Piece{r.ticket, r.out ? r.out + size_t(part.taken) * O : nullptr, b.rows, take, last, 0,
                             r.bits ? r.bits + size_t(part.taken) * wpr : nullptr});
    if (rk == kSet) {  // a later part of a split request continues at taken * len of the caller's probs
      Piece &pc = b.pieces.back();
      const size_t len = r.set->size();
      pc.set = r.set;
      pc.set_off = b.set_nodes, pc.block_off = b.nnz;
      pc.probs = r.set_probs ? r.set_probs + size_t(part.taken) * len : nullptr;
      pc.inactive = r.set_inactive + part.taken;
      b.set_nodes += int(len);
      b.nnz += take * int(len);
    }
    if (rk == kTopk) {  // a later part of a split request continues at taken * k of the caller's arrays
      Piece &pc = b.pieces.back();
      pc.topk = r.topk;
      pc.topk_nodes = r.topk_nodes + size_t(part.taken) * size_t(r.topk);
      pc.topk_probs = r.topk_probs + size_t(part.taken) * size_t(r.topk);
      b.topk_k = std::max(b.topk_k, r.topk);
    }
    if (rk == kPool)  // a later part of a split request continues at taken * C of the caller's array
      b.pieces.back().pooled = r.pooled + size_t(part.taken) * size_t(r.pool_classes);
    if (b.raw) {  // the raw frames this piece's rows reference, and where they are staged
      const int u0 = r.raw_a + part.taken;  // the piece's first row as a frame of its utterance
      int fa, fb;
      splice_halo(*r.spec, r.raw_n, u0, u0 + take, &fa, &fb);
      b.raw_src.push_back(RawSrc{fa, fb - fa, b.raw_frames});
      b.segs.push_back(SpliceSeg{b.rows, b.raw_frames + u0 - fa, b.raw_frames - fa, b.raw_frames + r.raw_n - 1 - fa});
      b.raw_frames += fb - fa;
    }
    b.rows += take;
    if (last) queue.pop_front();
  }
  // compacted return (bit-mask batches): worth it while a row is at most 3/4 active nodes
  const size_t stride = size_t(b.most) + 1;
  b.stride = b.kind == kBits && stride * 4 <= O * 3 ? int(stride) : 0;
  return b;
}

}  // namespace fdnn::plan
