// fdnn_server.cpp -- the multi-stream scoring loop: many utterances in flight
// on one MI355X behind one model handle.
//
// The reference's serving shape is caller-side threads over independent utterances, one
// CalculationContext per call (QuantizedDnn.java:72-107, MultiThreadedStressTest.java:48-69), and
// the README blames the per-call round trips for what the lazy path fails to gain (README.md:45).
// On the GPU the same shape wants two things the per-call API cannot give:
//
//   * batches in flight.  A full-size batch fills the chip kernel by kernel, so consecutive
//     batches are serialised on one compute stream, while their copies in and out run on the
//     slots' own streams.  That needs per-batch scratch (a context per slot) and a completion
//     handle per batch instead of "the stream is the handle": tickets.  (Round 2 ran the soft-max
//     scale pass of batch i on a tail stream under layer 0 of batch i+1; with the fused soft-max
//     and the int8 screening of layer 0 that lost and is gone: profiles/LABBOOK.md.)
//   * coalescing.  A 100-frame utterance is 1/100 of a launch that fills the chip.  Host-pointer
//     submissions from any number of threads are queued, packed into one batch per slot (up to
//     max_frames), scored once, and scattered back to the callers' buffers.  Frames are
//     independent and every kernel is batch-size invariant (tests: any split of a batch gives the
//     same bits), so a coalesced utterance is bit-identical to the same utterance scored alone.
//
// Small batches (too few tiles to fill the chip) run whole on the slot's own stream instead, so
// that several of them overlap.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "fdnn_internal.hpp"
#include "fdnn_lists.hpp"
#include "fdnn_server_plan.hpp"

using fdnn::Buf;  // a slot's staging buffers: pinned host memory, or device memory (fdnn_buf.hpp)
using fdnn::DeviceGuard;
using fdnn::fail;
using namespace fdnn::plan;  // Request, Piece, BatchPlan, plan_batch: what a batch contains

namespace {

// below this many frames a batch leaves most CUs idle: run it on its own stream next to others
constexpr int kSmallBatch = 2560;

struct TicketState {
  int status = 0;      // 0 running, != 0 failed with that fdnn_status
  int created = 0;     // pieces packed so far
  int done = 0;        // pieces copied out
  int failed = 0;      // pieces lost with their batch (never copied)
  bool closed = false; // the final piece has been packed, or the rest of the request was dropped after a failure
  // a piece is in flight while created > done + failed: wait() does not hand a failed ticket back to its caller before
  // that is over -- the packer still reads the caller's frames and the copy threads still write the caller's rows
};

struct Slot {
  fdnn_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;   // small batches: the whole batch; host batches: copies
  hipEvent_t gemm_done = nullptr, staged = nullptr, done = nullptr;  // gemm_done: the compute stream's results, for the slot's stream
  uint64_t ticket = 0;            // device submissions: the ticket this slot last carried
  bool used = false;              // `done` has been recorded at least once
  // host submissions: staging, sized in max_frames units (h_x, h_mask, d_out with the host side, the rest on first use)
  Buf<float> h_x;
  Buf<int8_t> h_mask;
  Buf<float, true> d_out;
  Buf<float> h_out;               // whole-row batches of several callers: where the rows land on the host, ONE transfer per batch
  Buf<uint64_t> h_bits;           // bit-mask batches: the batch's words (pageable where pinned memory is refused)
  Buf<float, true> d_comp;        // ... its compacted result rows [rows][stride]
  Buf<float> h_comp;              // ... and where they land on the host: ONE transfer per batch, behind the compaction
  Buf<float> h_raw;               // raw batches: the pieces' raw frames back to back; grows to the largest raw batch
  Buf<int32_t> h_nodes;           // set batches: the pieces' sets back to back (pageable where pinned memory is refused) ...
  Buf<int32_t, true> d_nodes;     // ... and on the device; both grow to the largest set batch
  Buf<int32_t, true> d_topk;      // top-k batches: [rows][k_b] nodes, then [rows][k_b] values (the dense rows stay in d_out) ...
  Buf<int32_t> h_topk;            // ... and where both land on the host: ONE transfer per batch (pageable where pinned memory is refused)
  Buf<float, true> d_pool;        // pool batches: [rows][C] class sums (the dense rows stay in d_out) ...
  Buf<float> h_pool;              // ... and where they land on the host: ONE transfer per batch (pageable where pinned memory is refused)
  Buf<float> h_set;               // ... where its probs [nnz] and inactive values [rows] land: ONE transfer per batch (d_out holds both)
  BatchPlan batch;                // the current host batch: its pieces, where their frames are staged, how its rows return
  bool rows_on_host = false;      // its rows have been brought to h_out
  int pieces_left = 0;            // pieces not copied out yet
  bool in_flight = false;         // host batch enqueued, not yet scattered
};

}  // namespace

struct fdnn_server {
  fdnn_model *m = nullptr;
  int max_frames = 0, depth = 0;
  hipStream_t s_main = nullptr;
  std::vector<Slot> slots;
  std::mutex mu;                  // submission order + slot table
  uint64_t next_ticket = 1;
  uint64_t next_slot = 0;       // device submissions (under mu)
  uint64_t host_next_slot = 0;  // host batches (under qmu)
  // host path
  std::mutex qmu;
  std::condition_variable qcv, done_cv, slot_cv;
  bool packer_done = false;       // set by fdnn_server_free once the packer thread has been joined (under qmu)
  std::deque<Request> queue;
  std::deque<int> flying;         // slots with a host batch enqueued, in launch order
  std::unordered_map<uint64_t, TicketState> pending;  // host tickets not yet complete (a failed one stays until waited for)
  std::thread packer, finisher;
  // Staging of the batch being packed (frames / masks into the slot's pinned buffers) is shared with the callers blocked in
  // fdnn_server_wait: sixteen 100-frame utterances are 4.4 MB of memcpy, half a millisecond on the packer thread alone and
  // the longest stage of the loop; pieces are handed out one by one under qmu (stage_one).
  struct StageJob {
    Slot *sl = nullptr;
    int next = 0, done = 0, total = 0;
  } stage;
  bool staging = false;
  std::condition_variable stage_cv;
  bool stop = false;
  bool host_ready = false;
  int linger_us = 0;
  // statistics
  std::atomic<uint64_t> n_batches{0}, n_frames{0}, n_requests{0}, n_coalesced{0};
};

namespace {

int alloc_host_side(fdnn_server *s) {
  const fdnn::BlobHeader &h = s->m->hm.hdr;
  for (Slot &sl : s->slots) {
    const size_t n = size_t(s->max_frames);
    hipError_t e = sl.h_x.reserve(n * h.in_dim);
    if (e == hipSuccess) e = sl.h_mask.reserve(n * h.out_dim);
    if (e == hipSuccess) e = sl.d_out.reserve(n * h.out_dim + n);  // (+ n: a set batch's inactive values behind its probs)
    // the slot's context was made lean: the device-side landing buffers of host batches live here
    if (e == hipSuccess && !sl.ctx->d_x) e = sl.ctx->d_x.reserve(n * h.in_dim);
    if (e == hipSuccess && !sl.ctx->d_mask) e = sl.ctx->d_mask.reserve(n * h.out_dim);
    if (e != hipSuccess)
      return fail(e == hipErrorOutOfMemory ? FDNN_E_NOMEM : FDNN_E_DEVICE, std::string("server staging: ") + hipGetErrorString(e));
  }
  return FDNN_OK;
}

// Enqueue one batch that is already on the device, as the chunks of a pass (fdnn::run_chunks) on the slot's context.  Large
// batches: chunk by chunk (fdnn::frame_chunks) on the shared main stream; small ones: one chunk on the slot's stream, so
// that several of them overlap.  `after` (may be null): an event the compute must wait for, the batch's H2D copy.  behind(cs):
// what the batch launches over all its rows behind the chunks.  Returns with *last_stream the stream the batch's last work went to.
template <class Behind>
int enqueue_pass(fdnn_server *s, Slot &sl, int n, hipEvent_t after, const fdnn::pass::Pass &p, hipStream_t *last_stream, Behind &&behind) {
  fdnn_ctx *c = sl.ctx;
  c->n = n;
  c->last = -1;
  const bool small = n <= kSmallBatch;
  hipStream_t cs = small ? sl.stream : s->s_main;
  if (after) HIP_TRY(hipStreamWaitEvent(cs, after, 0));
  fdnn::CtxUse use;  // every way out notes the stream the batch ends on and puts the batch's frame count back
  use.n_after = n;
  HIP_TRY(use.enter(c, cs));
  const int rc = fdnn::run_chunks(c, cs, small ? fdnn::pass::Chunks{{0, n}} : fdnn::frame_chunks(n, c->m), p);
  if (rc) return rc;
  behind(cs);
  *last_stream = cs;
  return FDNN_OK;
}

struct BatchCall {
  const float *d_x = nullptr;
  int n = 0;
  const int8_t *d_masks = nullptr;  // one mask or none
  const uint64_t *d_bits = nullptr;
  float *d_out = nullptr;
  hipEvent_t after = nullptr;  // (may be null) see enqueue_pass
  float *d_comp = nullptr;     // bit-mask host batches: the rows compacted, `stride` floats each
  int stride = 0;
  int32_t *d_topk = nullptr;   // top-k host batches: [n][topk_k] nodes, then [n][topk_k] values, selected from d_out
  int topk_k = 0;
  const fdnn_pool *pool = nullptr;  // pool host batches: the batch's handle and [n][C] class sums of d_out
  float *d_pool = nullptr;
};
int enqueue_batch(fdnn_server *s, Slot &sl, const BatchCall &b, hipStream_t *last_stream) {
  const int n = b.n, O = s->m->hm.hdr.out_dim;
  return enqueue_pass(s, sl, n, b.after, fdnn::pass::Pass::loop_rows(b.d_x, b.d_masks, b.d_bits, b.d_out), last_stream, [&](hipStream_t cs) {
    // bit-mask host batches: the rows compacted (active probabilities + one value per frame) for the trip over PCIe
    if (b.d_bits && b.d_comp && b.stride > 0) fdnn::launch_lazy_compact(b.d_out, b.d_bits, b.d_comp, n, O, b.stride, cs);
    // top-k host batches: one selection launch with the batch's k over the rows, which stay here
    if (b.d_topk && b.topk_k > 0)
      fdnn::launch_topk(b.d_out, n, O, b.topk_k, b.d_topk, reinterpret_cast<float *>(b.d_topk + size_t(n) * size_t(b.topk_k)), cs);
    // pool host batches: one pooling launch over the rows, which stay here
    if (b.pool && b.d_pool) fdnn::launch_pool(b.d_out, n, O, b.pool->d_class_ptr(), b.pool->d_member(), b.pool->n_classes, b.d_pool, cs);
  });
}

// Enqueue one SET batch that is already on the device (kSet): the hidden layers as enqueue_batch runs them, then the pieces'
// sets as the segments of ONE sets call per chunk (fdnn::run_sets) -- no output layer.  probs go to d_out [nnz], the
// inactive values behind them [rows].
int enqueue_set_batch(fdnn_server *s, Slot &sl, hipEvent_t after, hipStream_t *last_stream) {
  const BatchPlan &b = sl.batch;
  // the pieces as the tables of a sets call over the batch's rows
  std::vector<int32_t> seg_rows, set_ptr;
  for (const Piece &p : b.pieces) seg_rows.push_back(p.row0), set_ptr.push_back(p.set_off);
  seg_rows.push_back(b.rows), set_ptr.push_back(b.set_nodes);
  const fdnn::sets::Tables t{seg_rows.data(), set_ptr.data(), int(b.pieces.size())};
  return enqueue_pass(s, sl, b.rows, after, fdnn::pass::Pass::loop_sets(sl.ctx->d_x, t, sl.d_nodes.p, sl.d_out.p, sl.d_out.p + size_t(b.nnz)), last_stream,
                      [](hipStream_t) {});
}

// A batch carrying `ticket` failed: whatever of that request is still queued will never be packed (the packer would read
// caller memory that the caller, told of the failure, is free to release).  Call with qmu held.
void drop_queued_rest(fdnn_server *s, uint64_t ticket) {
  s->queue.erase(std::remove_if(s->queue.begin(), s->queue.end(), [&](const Request &r) { return r.ticket == ticket; }), s->queue.end());
  auto t = s->pending.find(ticket);
  if (t != s->pending.end()) t->second.closed = true;
}

// The slot's batch is lost (nothing usable was enqueued, or the device failed under it): its tickets fail with `status`,
// the slot is free again.  Call with qmu held.  Marking the pieces done is safe wherever the batch failed: fdnn_server_wait
// looks at a slot's pieces only while in_flight, and that is cleared in this same critical section.
void fail_batch(fdnn_server *s, Slot &sl, int status) {
  for (Piece &p : sl.batch.pieces) {
    p.state = 3;
    auto it = s->pending.find(p.ticket);
    if (it != s->pending.end()) {
      it->second.status = status;
      it->second.failed++;
      drop_queued_rest(s, p.ticket);
    }
  }
  sl.pieces_left = 0;
  sl.in_flight = false;
  s->slot_cv.notify_all();
  s->done_cv.notify_all();
}

// Hands rows back to their callers.  The rows of a finished batch sit in the slot's device buffer; whoever gets
// there first copies a piece out -- the caller blocked in fdnn_server_wait (so that many callers copy in
// parallel: 3.2 MB per 100-frame utterance, one thread's copies would be the slowest stage of the loop) or the
// finisher thread (so that a ticket nobody waits for cannot hold a slot).  Call with qmu held; the lock is
// dropped around each memcpy.  `only_ticket` = 0 takes any ready piece of the slot.
void copy_ready_pieces(fdnn_server *s, std::unique_lock<std::mutex> &lk, Slot &sl, uint64_t only_ticket) {
  const size_t O = size_t(s->m->hm.hdr.out_dim);
  for (size_t i = 0; i < sl.batch.pieces.size(); ++i) {
    Piece &p = sl.batch.pieces[i];
    if (p.state != 1 || (only_ticket && p.ticket != only_ticket)) continue;
    p.state = 2;
    const Piece job = p;  // the vector is stable while in_flight, but copy what the unlocked part needs anyway
    lk.unlock();
    // straight from the slot's device buffer into the caller's memory, on the copying thread's own stream: no pinned
    // bounce buffer and no second pass over the 32 KB per frame
    hipError_t ce = hipSuccess;
    const size_t stride = size_t(sl.batch.stride);  // (stable while the slot is in flight)
    if (job.pooled) {
      // a pool piece: the batch's class sums came to the slot's landing buffer with the batch, C columns a row
      const size_t C = size_t(sl.batch.pool_classes);
      std::memcpy(job.pooled, sl.h_pool.p + size_t(job.row0) * C, sizeof(float) * size_t(job.rows) * C);
    } else if (job.topk) {
      // a top-k piece: the batch's pairs came to the slot's landing buffer with the batch, k_b columns a row; this piece
      // keeps the first k of its rows (the top k is a prefix of the top k_b)
      const size_t kb = size_t(sl.batch.topk_k), k = size_t(job.topk), all = size_t(sl.batch.rows) * kb;
      for (size_t r = 0; r < size_t(job.rows); ++r) {
        const int32_t *src = sl.h_topk.p + (size_t(job.row0) + r) * kb;
        std::memcpy(job.topk_nodes + r * k, src, sizeof(int32_t) * k);
        std::memcpy(job.topk_probs + r * k, src + all, sizeof(float) * k);
      }
    } else if (job.set) {
      // a set piece: its block of probs and its inactive values came to the slot's landing buffer with the batch
      const size_t len = job.set->size();
      if (len) std::memcpy(job.probs, sl.h_set.p + size_t(job.block_off), sizeof(float) * size_t(job.rows) * len);
      std::memcpy(job.inactive, sl.h_set.p + size_t(sl.batch.nnz) + size_t(job.row0), sizeof(float) * size_t(job.rows));
    } else if (job.bits && stride > 0) {
      // lazy rows, compacted: the batch's rows arrived in the slot's pinned buffer with the batch (one transfer, enqueued
      // behind the compaction); THIS thread -- the caller's own, normally, so that sixteen callers work side by side --
      // expands its rows into the caller's block (fdnn::lazy_expand_rows_from)
      fdnn::lazy_expand_rows_from(job.out, sl.h_comp.p + size_t(job.row0) * stride, job.rows, O, stride, job.bits);
    } else if (sl.rows_on_host) {
      // whole rows of a coalesced batch: they came to the slot's pinned buffer with the batch; this thread moves its own
      std::memcpy(job.out, sl.h_out.p + size_t(job.row0) * O, sizeof(float) * size_t(job.rows) * O);
    } else {
      DeviceGuard dg(s->m->device);
      ce = hipMemcpyAsync(job.out, sl.d_out.p + size_t(job.row0) * O, sizeof(float) * size_t(job.rows) * O, hipMemcpyDeviceToHost,
                          hipStreamPerThread);
      if (ce == hipSuccess) ce = hipStreamSynchronize(hipStreamPerThread);
    }
    lk.lock();
    sl.batch.pieces[i].state = 3;
    auto it = s->pending.find(job.ticket);
    bool finished = false;
    if (it != s->pending.end()) {
      it->second.done++;
      if (ce != hipSuccess) {
        it->second.status = FDNN_E_DEVICE;
        drop_queued_rest(s, job.ticket);
      }
      if (it->second.closed && it->second.done == it->second.created && it->second.status == 0) {
        s->pending.erase(it);
        finished = true;
      }
    }
    if (--sl.pieces_left == 0) {
      sl.in_flight = false;
      s->slot_cv.notify_all();
    }
    if (finished || ce != hipSuccess) s->done_cv.notify_all();
  }
}

// One request's frames (and masks) into the slot's pinned buffers, by whoever asks: the packer, or a caller waiting for its
// ticket.  Call with qmu held (dropped around the copies); false = nothing left to hand out.
bool stage_one(fdnn_server *s, std::unique_lock<std::mutex> &lk) {
  if (!s->staging || s->stage.next >= s->stage.total) return false;
  const int i = s->stage.next++;
  Slot &sl = *s->stage.sl;
  const Request r = sl.batch.taken[size_t(i)];
  const int r0 = sl.batch.pieces[size_t(i)].row0, kind = sl.batch.kind;
  const bool any_mask = sl.batch.any_mask;
  lk.unlock();
  const fdnn::BlobHeader &h = s->m->hm.hdr;
  const size_t D = size_t(h.in_dim), O = size_t(h.out_dim), wpr = (O + 63) / 64;
  if (r.raw) {
    const size_t RD = size_t(sl.batch.spec->raw_dim);
    const RawSrc src = sl.batch.raw_src[size_t(i)];
    std::memcpy(sl.h_raw.p + size_t(src.at) * RD, r.raw + size_t(src.first) * RD, sizeof(float) * size_t(src.count) * RD);
  } else {
    std::memcpy(sl.h_x.p + size_t(r0) * D, r.x + size_t(r.taken) * D, sizeof(float) * size_t(r.n) * D);
  }
  if (kind == kSet) {
    const Piece &pc = sl.batch.pieces[size_t(i)];  // (stable while the slot is in flight)
    if (!pc.set->empty()) std::memcpy(sl.h_nodes.p + size_t(pc.set_off), pc.set->data(), sizeof(int32_t) * pc.set->size());
  } else if (kind == kBits && sl.h_bits.p) {  // (only bit-mask requests are in such a batch)
    std::memcpy(sl.h_bits.p + size_t(r0) * wpr, r.bits + size_t(r.taken) * wpr, sizeof(uint64_t) * size_t(r.n) * wpr);
  } else if (any_mask) {
    if (r.masks)
      std::memcpy(sl.h_mask.p + size_t(r0) * O, r.masks + size_t(r.taken) * O, size_t(r.n) * O);
    else
      std::memset(sl.h_mask.p + size_t(r0) * O, 1, size_t(r.n) * O);  // dense caller inside a lazy batch: all active
  }
  lk.lock();
  if (++s->stage.done == s->stage.total) s->stage_cv.notify_all();
  return true;
}

// The packer's steps, in packer_loop's order.  Work to pack (false: the loop ends with nothing queued).  Call with qmu held.
bool wait_for_work(fdnn_server *s, std::unique_lock<std::mutex> &lk) {
  s->qcv.wait(lk, [&] { return s->stop || !s->queue.empty(); });
  if (s->stop && s->queue.empty()) return false;
  // lingering only pays while an earlier batch keeps the device busy: an idle server launches at once
  const bool gpu_busy = std::any_of(s->slots.begin(), s->slots.end(), [](const Slot &sl) { return sl.in_flight; });
  if (s->linger_us > 0 && !s->stop && gpu_busy)  // give concurrent callers a moment to join the batch, unless it is full
    s->qcv.wait_for(lk, std::chrono::microseconds(s->linger_us), [&] {
      size_t have = 0;
      for (const Request &r : s->queue) have += size_t(r.n - r.taken);
      return s->stop || have >= size_t(s->max_frames);
    });
  return true;
}

// A free slot (its previous host batch scattered), the oldest first; -1: the loop ends.  Call with qmu held.
int claim_slot(fdnn_server *s, std::unique_lock<std::mutex> &lk) {
  int si = -1;
  s->slot_cv.wait(lk, [&] {
    for (int k = 0; k < s->depth && si < 0; ++k) {
      const int cand = int((s->host_next_slot + uint64_t(k)) % uint64_t(s->depth));
      if (!s->slots[size_t(cand)].in_flight) si = cand;
    }
    return si >= 0 || s->stop;
  });
  return si;
}

// The next batch becomes the slot's, and its pieces are entered with their tickets.  One hold of qmu for all of it:
// fdnn_server_wait reads an in-flight slot's pieces.
void plan_into_slot(fdnn_server *s, Slot &sl) {
  sl.batch = plan_batch(s->queue, s->max_frames, size_t(s->m->hm.hdr.out_dim));
  for (const Piece &p : sl.batch.pieces) {
    auto it = s->pending.find(p.ticket);
    if (it == s->pending.end()) continue;
    it->second.created++;
    if (p.last) it->second.closed = true;
  }
  sl.pieces_left = int(sl.batch.pieces.size());
  sl.in_flight = true;
}

// The staging buffers this batch needs beyond the slot's fixed ones, each by its own rule.
hipError_t reserve_buffers(fdnn_server *s, Slot &sl) {
  const size_t O = size_t(s->m->hm.hdr.out_dim), frames = size_t(s->max_frames);
  BatchPlan &b = sl.batch;
  // Whole rows of a batch that several callers share (1 GB of pinned memory per slot at most) go to the host in one transfer;
  // a single caller's batch, or one for which no pinned memory is to be had, leaves by per-caller copies from the device.
  sl.rows_on_host = b.kind != kSet && b.kind != kTopk && b.kind != kPool && b.stride == 0 && b.taken.size() > 1 && frames * O * sizeof(float) <= (size_t(1) << 30) &&
                    sl.h_out.reserve(frames * O) == hipSuccess;
  if (b.kind == kBits) {
    // (advisor, round 5) no pinned memory to be had: pageable staging, the batch is not lost
    if (sl.h_bits.reserve(frames * ((O + 63) / 64), /*pageable_ok=*/true) != hipSuccess) return hipErrorOutOfMemory;
    const size_t need = frames * (O * 3 / 4 + 1);
    if (b.stride > 0 && sl.d_comp.count < need) {
      // both halves or neither, the old pair kept until the new one stands; a failure is not the batch's: its rows go back whole
      Buf<float, true> d_new;
      Buf<float> h_new;
      if (d_new.reserve(need) == hipSuccess && h_new.reserve(need) == hipSuccess) {
        sl.d_comp.swap(d_new);
        sl.h_comp.swap(h_new);
      } else {
        (void)hipGetLastError();
        b.stride = 0;
      }
    }
  }
  if (b.kind == kSet) {  // the sets up, probs and inactive values back: grown to the largest batch, pageable if need be
    hipError_t e = sl.h_nodes.reserve(std::max<size_t>(size_t(b.set_nodes), 1), /*pageable_ok=*/true);
    if (e == hipSuccess) e = sl.d_nodes.reserve(std::max<size_t>(size_t(b.set_nodes), 1));
    if (e == hipSuccess) e = sl.h_set.reserve(size_t(b.nnz) + size_t(b.rows), /*pageable_ok=*/true);
    if (e != hipSuccess) return e;
  }
  if (b.kind == kTopk) {  // the pairs of the batch: grown to the largest batch, the landing buffer pageable if need be
    hipError_t e = sl.d_topk.reserve(2 * size_t(b.rows) * size_t(b.topk_k));
    if (e == hipSuccess) e = sl.h_topk.reserve(2 * size_t(b.rows) * size_t(b.topk_k), /*pageable_ok=*/true);
    if (e != hipSuccess) return e;
  }
  if (b.kind == kPool) {  // the class sums of the batch: grown to the largest batch, the landing buffer pageable if need be
    hipError_t e = sl.d_pool.reserve(size_t(b.rows) * size_t(b.pool_classes));
    if (e == hipSuccess) e = sl.h_pool.reserve(size_t(b.rows) * size_t(b.pool_classes), /*pageable_ok=*/true);
    if (e != hipSuccess) return e;
  }
  if (!b.raw) return hipSuccess;
  const hipError_t e = sl.h_raw.reserve(size_t(b.raw_frames) * size_t(b.spec->raw_dim));
  if (e == hipSuccess && fdnn::ctx_raw_reserve(sl.ctx, size_t(b.raw_frames), b.spec->raw_dim)) return hipErrorOutOfMemory;
  return e;
}

// The pieces' frames and masks into the slot's pinned buffers: this thread and whoever is blocked in fdnn_server_wait,
// piece by piece (stage_one).
void stage_batch(fdnn_server *s, Slot &sl) {
  std::unique_lock<std::mutex> lk(s->qmu);
  s->stage.sl = &sl;
  s->stage.next = s->stage.done = 0;
  s->stage.total = int(sl.batch.taken.size());
  s->staging = true;
  if (s->stage.total > 1) s->done_cv.notify_all();
  while (stage_one(s, lk)) continue;
  s->stage_cv.wait(lk, [&] { return s->stage.done == s->stage.total; });
  s->staging = false;
}

// Copy in, compute, copy back -- all asynchronous, in launch order against device submissions (s->mu).  *rc: what
// enqueue_batch said; the rows leave the slot later, piece by piece (copy_ready_pieces).
hipError_t launch_batch(fdnn_server *s, Slot &sl, int *rc) {
  const fdnn::BlobHeader &h = s->m->hm.hdr;
  const BatchPlan &b = sl.batch;
  const size_t D = size_t(h.in_dim), O = size_t(h.out_dim), wpr = (O + 63) / 64, rows = size_t(b.rows);
  std::lock_guard<std::mutex> order(s->mu);
  fdnn_ctx *c = sl.ctx;
  const bool bits = b.kind == kBits;
  hipError_t e;
  if (b.raw) {  // only the raw frames cross PCIe; the rows are spliced on the device, each piece within its utterance
    const size_t raw_floats = size_t(b.raw_frames) * size_t(b.spec->raw_dim);
    e = hipMemcpyAsync(c->d_raw, sl.h_raw.p, sizeof(float) * raw_floats, hipMemcpyHostToDevice, sl.stream);
    if (e == hipSuccess) fdnn::splice_rows(*b.spec, int(D), c->d_raw, b.raw_frames, b.segs, 0, b.rows, c->d_x, sl.stream);
  } else {
    e = hipMemcpyAsync(c->d_x, sl.h_x.p, sizeof(float) * rows * D, hipMemcpyHostToDevice, sl.stream);
  }
  if (b.kind == kSet) {  // no masks and no output layer: the pieces' sets go up, probs and inactive values come back
    if (e == hipSuccess && b.set_nodes > 0)
      e = hipMemcpyAsync(sl.d_nodes.p, sl.h_nodes.p, sizeof(int32_t) * size_t(b.set_nodes), hipMemcpyHostToDevice, sl.stream);
    if (e == hipSuccess) e = hipEventRecord(sl.staged, sl.stream);
    if (e != hipSuccess) return e;
    hipStream_t last = sl.stream;
    *rc = enqueue_set_batch(s, sl, sl.staged, &last);
    if (*rc) return hipSuccess;
    if (last != sl.stream) {
      e = hipEventRecord(sl.gemm_done, last);
      if (e == hipSuccess) e = hipStreamWaitEvent(sl.stream, sl.gemm_done, 0);
    }
    if (e == hipSuccess)
      e = hipMemcpyAsync(sl.h_set.p, sl.d_out.p, sizeof(float) * (size_t(b.nnz) + rows), hipMemcpyDeviceToHost, sl.stream);
    if (e == hipSuccess) e = hipEventRecord(sl.done, sl.stream);
    return e;
  }
  if (e == hipSuccess && bits)
    e = hipMemcpyAsync(c->d_mask_bits, sl.h_bits.p, sizeof(uint64_t) * rows * wpr, hipMemcpyHostToDevice, sl.stream);
  else if (e == hipSuccess && b.any_mask)
    e = hipMemcpyAsync(c->d_mask, sl.h_mask.p, rows * O, hipMemcpyHostToDevice, sl.stream);
  if (e == hipSuccess) e = hipEventRecord(sl.staged, sl.stream);
  if (e != hipSuccess) return e;
  hipStream_t last = sl.stream;
  *rc = enqueue_batch(s, sl, {.d_x = c->d_x, .n = b.rows, .d_masks = !bits && b.any_mask ? c->d_mask : nullptr,
                              .d_bits = bits ? c->d_mask_bits : nullptr, .d_out = sl.d_out.p, .after = sl.staged,
                              .d_comp = sl.d_comp.p, .stride = b.stride, .d_topk = b.kind == kTopk ? sl.d_topk.p : nullptr,
                              .topk_k = b.topk_k, .pool = b.kind == kPool ? b.pool : nullptr, .d_pool = b.kind == kPool ? sl.d_pool.p : nullptr}, &last);
  if (*rc) return hipSuccess;
  if (last != sl.stream) {  // results leave on the slot's stream, behind the main stream's compute
    e = hipEventRecord(sl.gemm_done, last);
    if (e == hipSuccess) e = hipStreamWaitEvent(sl.stream, sl.gemm_done, 0);
  }
  if (e == hipSuccess && bits && b.stride > 0)  // compacted rows: to the host with the batch
    e = hipMemcpyAsync(sl.h_comp.p, sl.d_comp.p, sizeof(float) * rows * size_t(b.stride), hipMemcpyDeviceToHost, sl.stream);
  else if (e == hipSuccess && b.kind == kTopk)  // the pairs: to the host with the batch, the rows never leave the device
    e = hipMemcpyAsync(sl.h_topk.p, sl.d_topk.p, sizeof(int32_t) * 2 * rows * size_t(b.topk_k), hipMemcpyDeviceToHost, sl.stream);
  else if (e == hipSuccess && b.kind == kPool)  // the class sums: to the host with the batch, the rows never leave the device
    e = hipMemcpyAsync(sl.h_pool.p, sl.d_pool.p, sizeof(float) * rows * size_t(b.pool_classes), hipMemcpyDeviceToHost, sl.stream);
  else if (e == hipSuccess && sl.rows_on_host)
    e = hipMemcpyAsync(sl.h_out.p, sl.d_out.p, sizeof(float) * rows * O, hipMemcpyDeviceToHost, sl.stream);
  if (e == hipSuccess) e = hipEventRecord(sl.done, sl.stream);
  return e;
}

// Packs queued requests into batches and enqueues them: wait, claim a slot, plan, reserve, stage, launch, account.
void packer_loop(fdnn_server *s) {
  DeviceGuard g(s->m->device);
  for (;;) {
    std::unique_lock<std::mutex> lk(s->qmu);
    if (!wait_for_work(s, lk)) return;
    const int si = claim_slot(s, lk);
    if (si < 0) return;
    Slot &sl = s->slots[size_t(si)];
    plan_into_slot(s, sl);
    s->host_next_slot = uint64_t(si) + 1;
    lk.unlock();
    int rc = FDNN_OK;
    hipError_t e = reserve_buffers(s, sl);
    if (e == hipSuccess) {
      stage_batch(s, sl);
      e = launch_batch(s, sl, &rc);
    }
    if (e != hipSuccess) rc = fail(FDNN_E_DEVICE, std::string("server batch: ") + hipGetErrorString(e));
    s->n_batches++;
    s->n_frames += uint64_t(sl.batch.rows);
    if (sl.batch.taken.size() > 1) s->n_coalesced += sl.batch.taken.size();
    lk.lock();
    if (rc) {
      fail_batch(s, sl, rc);
    } else {
      s->flying.push_back(si);
      s->qcv.notify_all();  // wakes the finisher
    }
  }
}

// Waits for enqueued host batches in launch order, marks their rows ready and helps copying them out.
void finisher_loop(fdnn_server *s) {
  DeviceGuard g(s->m->device);
  for (;;) {
    int si;
    {
      std::unique_lock<std::mutex> lk(s->qmu);
      // (the finisher outlives the packer: at shutdown the packer still drains the queue, and a batch it enqueues after the
      // finisher had gone would never be marked ready or scattered)
      s->qcv.wait(lk, [&] { return (s->stop && s->packer_done) || !s->flying.empty(); });
      if (s->flying.empty()) return;  // stopped, and the packer has gone
      si = s->flying.front();
      s->flying.pop_front();
    }
    Slot &sl = s->slots[size_t(si)];
    const hipError_t e = hipEventSynchronize(sl.done);
    std::unique_lock<std::mutex> lk(s->qmu);
    if (e != hipSuccess) {
      fail_batch(s, sl, FDNN_E_DEVICE);
      continue;
    }
    for (Piece &p : sl.batch.pieces) p.state = 1;
    s->done_cv.notify_all();             // callers blocked in wait() copy their own rows ...
    copy_ready_pieces(s, lk, sl, 0);     // ... and this thread takes whatever nobody has claimed
  }
}

int start_host_side(fdnn_server *s) {
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->host_ready) return FDNN_OK;
  int rc = alloc_host_side(s);
  if (rc) return rc;
  s->packer = std::thread(packer_loop, s);
  s->finisher = std::thread(finisher_loop, s);
  s->host_ready = true;
  return FDNN_OK;
}

// The common end of the host submit entry points: a ticket for the request, and the request into the packer's queue.
int submit_host(fdnn_server *s, Request r, uint64_t *ticket) {
  const int rc = start_host_side(s);
  if (rc) return rc;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    r.ticket = s->next_ticket++;
  }
  {
    std::lock_guard<std::mutex> lk(s->qmu);
    s->pending.emplace(r.ticket, TicketState{});
    s->queue.push_back(r);
  }
  s->n_requests++;
  s->qcv.notify_all();
  *ticket = r.ticket;
  return FDNN_OK;
}

}  // namespace

namespace fdnn {

int server_submit_raw_rows(fdnn_server *s, const SpliceRef &spec, const float *raw, int n, int a, int b, const uint64_t *bits,
                           float *out, uint64_t *ticket) {
  int rc = splice_check(spec, -1);
  if (rc) return rc;
  if (n <= 0 || a < 0 || b > n || b <= a) return fail(FDNN_E_ARG, "frame count must be positive");
  if (!raw || !out) return fail(FDNN_E_ARG, "null buffer");
  const int most = bits ? widest_row(bits, b - a, size_t(s->m->hm.hdr.out_dim)) : 0;
  return submit_host(s, Request{.out = out, .n = b - a, .bits = bits, .most = most, .raw = raw, .spec = spec, .raw_n = n, .raw_a = a},
                     ticket);
}

}  // namespace fdnn

namespace {

// The common end of the set submit entry points: the set validated and copied (the caller may release it at once).
int submit_set(fdnn_server *s, Request r, const int32_t *nodes, int len, float *probs, float *inactive, uint64_t *ticket) {
  const int O = s->m->hm.hdr.out_dim;
  if (len < 0 || (len > 0 && !nodes)) return fail(FDNN_E_ARG, "bad node set");
  const int32_t row_ptr[2] = {0, len};
  if (fdnn::lists::check(row_ptr, nodes, 1, O))
    return fail(FDNN_E_ARG, "node set: the nodes must ascend strictly inside [0, " + std::to_string(O) + ")");
  if (!inactive || (len > 0 && !probs)) return fail(FDNN_E_ARG, "null buffer");
  if (static_cast<long long>(r.n) * len > INT32_MAX) return fail(FDNN_E_ARG, "n x len must fit an int32");
  r.set = std::make_shared<const std::vector<int32_t>>(nodes, nodes + len);
  r.set_probs = probs;
  r.set_inactive = inactive;
  return submit_host(s, std::move(r), ticket);
}

}  // namespace

extern "C" {

int fdnn_server_create(fdnn_model *m, int max_frames, int depth, fdnn_server **out) {
  if (!m || !out) return fail(FDNN_E_ARG, "null argument");
  *out = nullptr;
  if (max_frames <= 0 || depth < 1 || depth > 16) return fail(FDNN_E_ARG, "server needs max_frames > 0 and 1 <= depth <= 16");
  DeviceGuard g(m->device);
  if (!g.ok) return fail(FDNN_E_DEVICE, "hipSetDevice failed");
  std::unique_ptr<fdnn_server> s(new fdnn_server());
  s->m = m;
  s->max_frames = max_frames;
  s->depth = depth;
  s->slots = std::vector<Slot>(size_t(depth));
  int prio_least = 0, prio_greatest = 0;  // (the compute stream keeps the priority it had over the retired tail stream)
  hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  hipError_t e = hipStreamCreateWithPriority(&s->s_main, hipStreamNonBlocking, prio_greatest);
  int rc = FDNN_OK;
  for (Slot &sl : s->slots) {
    if (e != hipSuccess || rc) break;
    rc = fdnn::make_ctx(m, max_frames, &sl.ctx, /*lean=*/true);
    if (rc) break;
    e = hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking);
    sl.ctx->durable[0] = s->s_main;  // the loop's streams outlive the slot's context: its ordering records can wait until
    sl.ctx->durable[1] = sl.stream;  // another stream asks for them (fdnn::ctx_leave)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.gemm_done, hipEventDisableTiming | hipEventDisableSystemFence);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.staged, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
  }
  if (e != hipSuccess && !rc) rc = fail(FDNN_E_DEVICE, std::string("server: ") + hipGetErrorString(e));
  if (rc) {
    fdnn_server_free(s.release());
    return rc;
  }
  *out = s.release();
  return FDNN_OK;
}

void fdnn_server_free(fdnn_server *s) {
  if (!s) return;
  DeviceGuard g(s->m->device);
  {
    std::lock_guard<std::mutex> lk(s->qmu);
    s->stop = true;
  }
  s->qcv.notify_all();
  s->slot_cv.notify_all();
  if (s->packer.joinable()) s->packer.join();
  {
    std::lock_guard<std::mutex> lk(s->qmu);
    s->packer_done = true;
  }
  s->qcv.notify_all();
  if (s->finisher.joinable()) s->finisher.join();
  for (Slot &sl : s->slots) {
    if (sl.used && sl.done) hipEventSynchronize(sl.done);
    if (sl.stream) hipStreamSynchronize(sl.stream);
  }
  for (Slot &sl : s->slots)
    if (sl.stream) fdnn::fuse_chain_retire_stream(s->m->device, sl.stream);
  if (s->s_main) fdnn::fuse_chain_retire_stream(s->m->device, s->s_main);  // (the device's chain of fused launches may still name them)
  if (s->s_main) hipStreamSynchronize(s->s_main);
  for (Slot &sl : s->slots) {
    if (sl.ctx) fdnn::destroy_ctx(sl.ctx);
    for (hipEvent_t ev : {sl.gemm_done, sl.staged, sl.done})
      if (ev) hipEventDestroy(ev);
    if (sl.stream) hipStreamDestroy(sl.stream);
  }
  if (s->s_main) hipStreamDestroy(s->s_main);
  delete s;  // (with the slots' staging buffers)
}

int fdnn_server_set_linger_us(fdnn_server *s, int microseconds) {
  if (!s || microseconds < 0) return fail(FDNN_E_ARG, "bad argument");
  std::lock_guard<std::mutex> lk(s->qmu);
  s->linger_us = microseconds;
  return FDNN_OK;
}

int fdnn_server_submit_device(fdnn_server *s, const float *d_x, int n, const int8_t *d_masks, float *d_out, uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  if (n <= 0 || n > s->max_frames) return fail(FDNN_E_ARG, "frame count must be in 1..max_frames of the server");
  if (!d_x || !d_out) return fail(FDNN_E_ARG, "null buffer");
  if (int rc = fdnn::check_frames_aligned(d_x)) return rc;
  DeviceGuard g(s->m->device);
  std::unique_lock<std::mutex> lk(s->mu);
  // next slot in submission order; its previous batch must have completed (that bounds the batches in flight)
  int si = -1;
  for (;;) {
    const int cand = int(s->next_slot % uint64_t(s->depth));
    Slot &c = s->slots[size_t(cand)];
    bool host_busy;
    {
      std::lock_guard<std::mutex> q(s->qmu);
      host_busy = c.in_flight;
    }
    if (!host_busy) {
      si = cand;
      break;
    }
    lk.unlock();  // a host batch owns it: wait for the finisher, then look again
    {
      std::unique_lock<std::mutex> q(s->qmu);
      s->slot_cv.wait(q, [&] { return !s->slots[size_t(cand)].in_flight; });
    }
    lk.lock();
  }
  Slot &sl = s->slots[size_t(si)];
  if (sl.used) HIP_TRY(hipEventSynchronize(sl.done));
  hipStream_t last = nullptr;
  int rc = enqueue_batch(s, sl, {.d_x = d_x, .n = n, .d_masks = d_masks, .d_out = d_out}, &last);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(sl.done, last));
  sl.used = true;
  sl.ticket = s->next_ticket++;
  s->next_slot = uint64_t(si) + 1;
  *ticket = sl.ticket;
  s->n_batches++;
  s->n_frames += uint64_t(n);
  s->n_requests++;
  return FDNN_OK;
}

int fdnn_server_submit(fdnn_server *s, const float *x, int n, const int8_t *masks, float *out, uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  if (n <= 0) return fail(FDNN_E_ARG, "frame count must be positive");
  if (!x || !out) return fail(FDNN_E_ARG, "null buffer");
  return submit_host(s, Request{.x = x, .masks = masks, .out = out, .n = n}, ticket);
}

int fdnn_server_submit_lazy_bits(fdnn_server *s, const float *x, int n, const uint64_t *bits, float *out, uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  if (n <= 0) return fail(FDNN_E_ARG, "frame count must be positive");
  if (!x || !out || !bits) return fail(FDNN_E_ARG, "null buffer");
  const int most = widest_row(bits, n, size_t(s->m->hm.hdr.out_dim));
  return submit_host(s, Request{.x = x, .out = out, .n = n, .bits = bits, .most = most}, ticket);
}

int fdnn_server_submit_raw(fdnn_server *s, const float *raw, int n, const uint64_t *bits, float *out, uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  return fdnn::server_submit_raw_rows(s, s->m->splice, raw, n, 0, n, bits, out, ticket);
}

int fdnn_server_submit_lazy_set(fdnn_server *s, const float *x, int n, const int32_t *nodes, int len, float *probs, float *inactive,
                                uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  if (n <= 0) return fail(FDNN_E_ARG, "frame count must be positive");
  if (!x) return fail(FDNN_E_ARG, "null buffer");
  return submit_set(s, Request{.x = x, .n = n}, nodes, len, probs, inactive, ticket);
}

int fdnn_server_submit_raw_set(fdnn_server *s, const float *raw, int n, const int32_t *nodes, int len, float *probs, float *inactive,
                               uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  const fdnn::SpliceRef spec = s->m->splice;
  if (int rc = fdnn::splice_check(spec, -1)) return rc;
  if (n <= 0) return fail(FDNN_E_ARG, "frame count must be positive");
  if (!raw) return fail(FDNN_E_ARG, "null buffer");
  return submit_set(s, Request{.n = n, .raw = raw, .spec = spec, .raw_n = n, .raw_a = 0}, nodes, len, probs, inactive, ticket);
}

int fdnn_server_submit_topk(fdnn_server *s, const float *x, int n, int k, int32_t *nodes, float *probs, uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  if (n <= 0) return fail(FDNN_E_ARG, "frame count must be positive");
  if (!fdnn::topk::args_ok(s->m->hm.hdr.out_dim, k)) return fail(FDNN_E_ARG, "k is 1 .. min(output_dim, 256)");
  if (!x || !nodes || !probs) return fail(FDNN_E_ARG, "null buffer");
  return submit_host(s, Request{.x = x, .n = n, .topk = k, .topk_nodes = nodes, .topk_probs = probs}, ticket);
}

int fdnn_server_submit_raw_topk(fdnn_server *s, const float *raw, int n, int k, int32_t *nodes, float *probs, uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  const fdnn::SpliceRef spec = s->m->splice;
  if (int rc = fdnn::splice_check(spec, -1)) return rc;
  if (n <= 0) return fail(FDNN_E_ARG, "frame count must be positive");
  if (!fdnn::topk::args_ok(s->m->hm.hdr.out_dim, k)) return fail(FDNN_E_ARG, "k is 1 .. min(output_dim, 256)");
  if (!raw || !nodes || !probs) return fail(FDNN_E_ARG, "null buffer");
  return submit_host(s, Request{.n = n, .raw = raw, .spec = spec, .raw_n = n, .raw_a = 0, .topk = k, .topk_nodes = nodes, .topk_probs = probs}, ticket);
}

int fdnn_server_submit_pool(fdnn_server *s, const float *x, int n, const fdnn_pool *pool, float *out, uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  if (n <= 0) return fail(FDNN_E_ARG, "frame count must be positive");
  if (int rc = fdnn::check_pool(s->m, pool)) return rc;
  if (!x || !out) return fail(FDNN_E_ARG, "null buffer");
  return submit_host(s, Request{.x = x, .n = n, .pool = pool, .pool_classes = pool->n_classes, .pooled = out}, ticket);
}

int fdnn_server_submit_raw_pool(fdnn_server *s, const float *raw, int n, const fdnn_pool *pool, float *out, uint64_t *ticket) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  const fdnn::SpliceRef spec = s->m->splice;
  if (int rc = fdnn::splice_check(spec, -1)) return rc;
  if (n <= 0) return fail(FDNN_E_ARG, "frame count must be positive");
  if (int rc = fdnn::check_pool(s->m, pool)) return rc;
  if (!raw || !out) return fail(FDNN_E_ARG, "null buffer");
  return submit_host(s, Request{.n = n, .raw = raw, .spec = spec, .raw_n = n, .raw_a = 0, .pool = pool, .pool_classes = pool->n_classes, .pooled = out}, ticket);
}

int fdnn_server_wait(fdnn_server *s, uint64_t ticket) {
  if (!s) return fail(FDNN_E_ARG, "null argument");
  {  // a host ticket?
    std::unique_lock<std::mutex> lk(s->qmu);
    if (s->pending.find(ticket) != s->pending.end()) {
      for (;;) {
        auto it = s->pending.find(ticket);
        if (it == s->pending.end()) return FDNN_OK;  // complete (the last piece was copied, here or by the finisher)
        if (it->second.status != 0 && it->second.closed && it->second.created == it->second.done + it->second.failed) {
          const int status = it->second.status;  // no piece of it is queued or in flight any more
          s->pending.erase(it);
          return fail(status, "a batch carrying this ticket failed on the device");
        }
        bool copied = false;
        for (Slot &sl : s->slots) {
          if (!sl.in_flight) continue;
          for (const Piece &p : sl.batch.pieces)
            if (p.ticket == ticket && p.state == 1) {
              copy_ready_pieces(s, lk, sl, ticket);
              copied = true;
              break;
            }
        }
        if (!copied && !stage_one(s, lk)) s->done_cv.wait(lk);  // (idle hands: help the packer stage the next batch)
      }
    }
  }
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(s->mu);
    if (ticket == 0 || ticket >= s->next_ticket) return fail(FDNN_E_ARG, "unknown ticket");
    for (Slot &sl : s->slots)
      if (sl.used && sl.ticket == ticket) ev = sl.done;
  }
  if (!ev) return FDNN_OK;  // its slot has been reused since: a slot is only reused after completion
  DeviceGuard g(s->m->device);
  HIP_TRY(hipEventSynchronize(ev));
  return FDNN_OK;
}

int fdnn_server_drain(fdnn_server *s) {
  if (!s) return fail(FDNN_E_ARG, "null argument");
  {
    std::unique_lock<std::mutex> lk(s->qmu);
    s->done_cv.wait(lk, [&] {
      for (auto it = s->pending.begin(); it != s->pending.end();) {
        const TicketState &t = it->second;
        if (t.status == 0 || !t.closed || t.created != t.done + t.failed) return false;  // running, or pieces still in flight
        it = s->pending.erase(it);  // failed and quiescent, nobody waited for it: forget it
      }
      return true;
    });
  }
  DeviceGuard g(s->m->device);
  std::lock_guard<std::mutex> lk(s->mu);
  for (Slot &sl : s->slots)
    if (sl.used) HIP_TRY(hipEventSynchronize(sl.done));
  return FDNN_OK;
}

int fdnn_server_stats(fdnn_server *s, uint64_t *batches, uint64_t *frames, uint64_t *requests, uint64_t *coalesced_requests) {
  if (!s) return fail(FDNN_E_ARG, "null argument");
  if (batches) *batches = s->n_batches.load();
  if (frames) *frames = s->n_frames.load();
  if (requests) *requests = s->n_requests.load();
  if (coalesced_requests) *coalesced_requests = s->n_coalesced.load();
  return FDNN_OK;
}

}  // extern "C"
