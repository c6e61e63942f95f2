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
#include <optional>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "fdnn_internal.hpp"
#include "fdnn_lists.hpp"
#include "fdnn_server_plan.hpp"
#include "fdnn_stream_plan.hpp"

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
  // A batch has one form, so one pair serves every form whose results are not rows: 32-bit words, both grow to the largest batch
  Buf<uint32_t, true> d_res;      // top-k batches: [rows][k_b] nodes, then [rows][k_b] values; pool batches: [rows][C] class sums (the dense rows stay in d_out)
  Buf<uint32_t> h_land;           // where they, or a set batch's probs [nnz] and inactive values [rows] (d_out holds both), land on the host:
                                  // ONE transfer per batch (pageable where pinned memory is refused)
  BatchPlan batch;                // the current host batch: its pieces, where their frames are staged, its form
  const void *landing = nullptr;  // where its one transfer lands (launch_batch): h_out, h_comp or h_land
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
  bool hold = false;              // fdnn_debug_server_hold: the packer plans nothing, submissions queue up (under qmu)
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
    hipError_t ce = hipSuccess;
    if (sl.batch.form.leave == Form::by_caller_copies) {  // (the batch's form is stable while the slot is in flight)
      // a single caller's whole rows: straight from the slot's device buffer into the caller's memory, on the copying
      // thread's own stream -- no pinned bounce buffer and no second pass over the 32 KB per frame
      DeviceGuard dg(s->m->device);
      ce = hipMemcpyAsync(job.want.out, sl.d_out.p + size_t(job.row0) * O, sizeof(float) * size_t(job.rows) * O, hipMemcpyDeviceToHost,
                          hipStreamPerThread);
      if (ce == hipSuccess) ce = hipStreamSynchronize(hipStreamPerThread);
    } else {
      // the piece's part of the batch's one transfer, which came to the slot's landing buffer with the batch; compacted lazy
      // rows are expanded by THIS thread -- the caller's own, normally, so that sixteen callers work side by side
      scatter(sl.batch, job, sl.landing, O, fdnn::lazy_expand_rows_from);
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
  const Piece &pc = sl.batch.pieces[size_t(i)];  // (the vector, the piece's rows and its Want are stable while the slot is in flight)
  const Form::Upload upload = sl.batch.form.upload;
  lk.unlock();
  const fdnn::BlobHeader &h = s->m->hm.hdr;
  const size_t D = size_t(h.in_dim), O = size_t(h.out_dim), wpr = (O + 63) / 64, r0 = size_t(pc.row0), rows = size_t(pc.rows);
  switch (r.frames.kind) {
    case Frames::raw_frames: {
      const size_t RD = size_t(sl.batch.spec->raw_dim);
      const RawSrc src = sl.batch.raw_src[size_t(i)];
      std::memcpy(sl.h_raw.p + size_t(src.at) * RD, r.frames.raw + size_t(src.first) * RD, sizeof(float) * size_t(src.count) * RD);
      break;
    }
    case Frames::host_rows: std::memcpy(sl.h_x.p + r0 * D, r.frames.x + size_t(r.taken) * D, sizeof(float) * rows * D); break;
  }
  switch (upload) {  // what goes up beside the frames: this piece's part of it
    case Form::no_upload: break;
    case Form::node_sets:
      if (!pc.want.nodes->empty()) std::memcpy(sl.h_nodes.p + size_t(pc.set_off), pc.want.nodes->data(), sizeof(int32_t) * pc.want.nodes->size());
      break;
    case Form::bit_words: std::memcpy(sl.h_bits.p + r0 * wpr, pc.want.bits, sizeof(uint64_t) * rows * wpr); break;
    case Form::byte_masks:
      if (pc.want.kind == Want::rows_behind_bytes)
        std::memcpy(sl.h_mask.p + r0 * O, pc.want.masks, rows * O);
      else
        std::memset(sl.h_mask.p + r0 * O, 1, rows * O);  // dense caller inside a byte-mask batch: all active
      break;
  }
  lk.lock();
  if (++s->stage.done == s->stage.total) s->stage_cv.notify_all();
  return true;
}

// The packer's steps, in packer_loop's order.  Work to pack (false: the loop ends with nothing queued).  Call with qmu held.
bool wait_for_work(fdnn_server *s, std::unique_lock<std::mutex> &lk) {
  s->qcv.wait(lk, [&] { return s->stop || (!s->hold && !s->queue.empty()); });
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

// The staging buffers this batch needs beyond the slot's fixed ones, each by its own rule; the sizes are the form's.  Where
// the room a form's transfer needs is refused, the batch is not lost: its rows leave by per-caller copies.
hipError_t reserve_buffers(fdnn_server *s, Slot &sl) {
  const size_t O = size_t(s->m->hm.hdr.out_dim), frames = size_t(s->max_frames);
  BatchPlan &b = sl.batch;
  const Form &f = b.form;
  hipError_t e = hipSuccess;
  switch (b.kind) {
    case Want::rows:
    case Want::rows_behind_bytes: break;  // (byte masks are staged in h_mask, one of the fixed buffers)
    case Want::rows_behind_bits: {
      // (advisor, round 5) no pinned memory to be had: pageable staging, the batch is not lost
      if (sl.h_bits.reserve(frames * ((O + 63) / 64), /*pageable_ok=*/true) != hipSuccess) return hipErrorOutOfMemory;
      const size_t need = frames * (O * 3 / 4 + 1);
      if (f.leave == Form::compacted_rows && sl.d_comp.count < need) {
        // both halves or neither, the old pair kept until the new one stands; a failure is not the batch's: its rows go back whole
        Buf<float, true> d_new;
        Buf<float> h_new;
        if (d_new.reserve(need) == hipSuccess && h_new.reserve(need) == hipSuccess) {
          sl.d_comp.swap(d_new);
          sl.h_comp.swap(h_new);
        } else {
          (void)hipGetLastError();
          leave_by_caller_copies(b);
        }
      }
      break;
    }
    case Want::set:  // the sets up, probs and inactive values back: grown to the largest batch, pageable if need be
      e = sl.h_nodes.reserve(std::max<size_t>(size_t(b.set_nodes), 1), /*pageable_ok=*/true);
      if (e == hipSuccess) e = sl.d_nodes.reserve(std::max<size_t>(size_t(b.set_nodes), 1));
      if (e == hipSuccess) e = sl.h_land.reserve(f.words, /*pageable_ok=*/true);
      break;
    case Want::topk:
    case Want::loglik:
    case Want::pool:  // the pairs, the class sums or the scores of the batch: grown to the largest batch, the landing buffer pageable if need be
      e = sl.d_res.reserve(f.words);
      if (e == hipSuccess) e = sl.h_land.reserve(f.words, /*pageable_ok=*/true);
      break;
  }
  if (e != hipSuccess) return e;
  // whole rows of a batch that several callers share land in pinned memory only
  if (f.leave == Form::whole_rows && sl.h_out.reserve(frames * O) != hipSuccess) leave_by_caller_copies(b);
  if (!b.raw) return hipSuccess;
  // a live batch's segment table rides behind the raw frames, in the same buffers and the same copy (live_table): the room
  // is asked for in whole raw frames
  const size_t RD = size_t(b.spec->raw_dim), words = b.live ? live_table(b).words : size_t(b.raw_frames) * RD;
  e = sl.h_raw.reserve(words);
  if (e == hipSuccess && fdnn::ctx_raw_reserve(sl.ctx, (words + RD - 1) / RD, b.spec->raw_dim)) return hipErrorOutOfMemory;
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

// Copy in, compute, copy back -- all asynchronous, in launch order against device submissions (s->mu), and one sequence for
// every form: frames up, the form's upload, `staged`, the form's pass and what it launches behind it, the streams joined,
// the form's one transfer, `done`.  *rc: what enqueue_pass said; the results leave the slot later, piece by piece
// (copy_ready_pieces).
hipError_t launch_batch(fdnn_server *s, Slot &sl, int *rc) {
  using fdnn::pass::Pass;
  const fdnn::BlobHeader &h = s->m->hm.hdr;
  const BatchPlan &b = sl.batch;
  const Form &f = b.form;
  const size_t D = size_t(h.in_dim), rows = size_t(b.rows);
  const int n = b.rows, O = h.out_dim;
  std::lock_guard<std::mutex> order(s->mu);
  fdnn_ctx *c = sl.ctx;
  hipError_t e;
  if (b.raw) {  // only the raw frames cross PCIe; the rows are spliced on the device, each piece within its utterance
    // A batch with a live piece has about one segment per push: its table goes up behind the frames, in the same copy, and
    // ONE launch reads it from device memory.  Every other batch: the table by value, as ever (fdnn::splice_rows).
    const LiveTable t = b.live ? live_table(b) : LiveTable{};
    if (b.live) write_live_table(b, t, reinterpret_cast<int32_t *>(sl.h_raw.p));
    const size_t raw_words = b.live ? t.words : size_t(b.raw_frames) * size_t(b.spec->raw_dim);
    e = hipMemcpyAsync(c->d_raw, sl.h_raw.p, sizeof(float) * raw_words, hipMemcpyHostToDevice, sl.stream);
    const int32_t *d_table = reinterpret_cast<const int32_t *>(c->d_raw.p);
    if (e == hipSuccess && b.live)
      fdnn::splice_rows_table(*b.spec, int(D), c->d_raw, b.raw_frames, d_table + t.segs_at, d_table + t.row_seg_at, int(b.segs.size()), b.rows,
                              c->d_x, sl.stream);
    else if (e == hipSuccess)
      fdnn::splice_rows(*b.spec, int(D), c->d_raw, b.raw_frames, b.segs, 0, b.rows, c->d_x, sl.stream);
  } else {
    e = hipMemcpyAsync(c->d_x, sl.h_x.p, sizeof(float) * rows * D, hipMemcpyHostToDevice, sl.stream);
  }
  const void *h_up = nullptr;  // what goes up beside the frames, and the mask it is to the pass (one or none)
  void *d_up = nullptr;
  const int8_t *d_masks = nullptr;
  const uint64_t *d_bits = nullptr;
  switch (f.upload) {
    case Form::no_upload: break;
    case Form::byte_masks: h_up = sl.h_mask.p, d_up = c->d_mask.p, d_masks = c->d_mask.p; break;
    case Form::bit_words: h_up = sl.h_bits.p, d_up = c->d_mask_bits.p, d_bits = c->d_mask_bits.p; break;
    case Form::node_sets: h_up = sl.h_nodes.p, d_up = sl.d_nodes.p; break;
  }
  if (e == hipSuccess && f.upload_bytes > 0) e = hipMemcpyAsync(d_up, h_up, f.upload_bytes, hipMemcpyHostToDevice, sl.stream);
  if (e == hipSuccess) e = hipEventRecord(sl.staged, sl.stream);
  if (e != hipSuccess) return e;
  // loop_sets: no output layer runs; the pieces are the segments of ONE sets call per chunk (fdnn::run_sets) over the batch's
  // rows, probs go to d_out [nnz], the inactive values behind them [rows]
  std::vector<int32_t> seg_rows, set_ptr;
  if (f.pass == Form::loop_sets) {
    for (const Piece &p : b.pieces) seg_rows.push_back(p.row0), set_ptr.push_back(p.set_off);
    seg_rows.push_back(b.rows), set_ptr.push_back(b.set_nodes);
  }
  const fdnn::sets::Tables t{seg_rows.data(), set_ptr.data(), int(b.pieces.size())};
  const Pass pass = f.pass == Form::loop_sets ? Pass::loop_sets(c->d_x, t, sl.d_nodes.p, sl.d_out.p, sl.d_out.p + size_t(b.nnz))
                                              : Pass::loop_rows(c->d_x, d_masks, d_bits, sl.d_out.p);
  hipStream_t last = sl.stream;
  *rc = enqueue_pass(s, sl, n, sl.staged, pass, &last, [&](hipStream_t cs) {
    switch (f.behind) {  // one launch over all the rows, which stay on the device
      case Form::nothing: break;
      case Form::compact:  // the rows compacted (active probabilities + one value per frame) for the trip over PCIe
        fdnn::launch_lazy_compact(sl.d_out.p, d_bits, sl.d_comp.p, n, O, b.stride, cs);
        break;
      case Form::select_topk: {  // one selection with the batch's k: [n][k_b] nodes, then [n][k_b] values
        int32_t *nodes = reinterpret_cast<int32_t *>(sl.d_res.p);
        fdnn::launch_topk(sl.d_out.p, n, O, b.topk_k, nodes, reinterpret_cast<float *>(nodes + rows * size_t(b.topk_k)), cs);
        break;
      }
      case Form::pool_sums:  // [n][C] class sums
        fdnn::launch_pool(sl.d_out.p, n, O, b.pool->d_class_ptr(), b.pool->d_member(), b.pool->n_classes, reinterpret_cast<float *>(sl.d_res.p), cs);
        break;
      case Form::loglik_scores:  // [n][O] decoder scores of the batch's handle
        fdnn::launch_loglik_rows(sl.d_out.p, n, O, b.score->d_log_prior, b.score->floor, b.score->type, sl.d_res.p, cs);
        break;
    }
  });
  if (*rc) return hipSuccess;
  if (last != sl.stream) {  // results leave on the slot's stream, behind the main stream's compute
    e = hipEventRecord(sl.gemm_done, last);
    if (e == hipSuccess) e = hipStreamWaitEvent(sl.stream, sl.gemm_done, 0);
  }
  const void *src = nullptr;  // the one transfer: f.words 32-bit words to the host with the batch
  void *dst = nullptr;
  switch (f.leave) {
    case Form::by_caller_copies: break;
    case Form::whole_rows: src = sl.d_out.p, dst = sl.h_out.p; break;
    case Form::compacted_rows: src = sl.d_comp.p, dst = sl.h_comp.p; break;
    case Form::set_blocks: src = sl.d_out.p, dst = sl.h_land.p; break;
    case Form::topk_pairs:
    case Form::scores:
    case Form::class_sums: src = sl.d_res.p, dst = sl.h_land.p; break;
  }
  sl.landing = dst;
  if (e == hipSuccess && dst) e = hipMemcpyAsync(dst, src, sizeof(uint32_t) * f.words, hipMemcpyDeviceToHost, sl.stream);
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

// The one path of every host submit entry point.  First where the frames come from: rows x [n][D] (spec null), or rows
// [a, b) of an n-frame raw utterance spliced by *spec.  Then what the entry's form needs: want(&w) fills w or fails.  Then
// submit_host.  Two bad arguments at once fail in this order.
using WantOut = std::optional<Want>;
template <class MakeWant>
int submit_frames(fdnn_server *s, const fdnn::SpliceRef *spec, const float *frames, int n, int a, int b, uint64_t *ticket, MakeWant &&want,
                  const WindowRef &window = nullptr) {
  if (spec)
    if (int rc = fdnn::splice_check(*spec, -1)) return rc;
  if (n <= 0 || a < 0 || b > n || b <= a) return fail(FDNN_E_ARG, "frame count must be positive");
  if (!frames) return fail(FDNN_E_ARG, "null buffer");
  WantOut w;
  if (int rc = want(&w)) return rc;
  // (window: a live push's own copy of its frames -- `frames` points into it, and the request keeps it alive)
  const Frames f = window ? Frames::live_rows(window, *spec, n, a) : spec ? Frames::raw_rows(frames, *spec, n, a) : Frames::rows(frames);
  return submit_host(s, Request(f, *w, b - a), ticket);
}

// ... for the extern "C" entries: n rows x, or (kRaw) a whole n-frame utterance under the model's splice spec as it is now
constexpr bool kRows = false, kRaw = true;
template <class MakeWant>
int submit_entry(fdnn_server *s, bool raw, const float *frames, int n, uint64_t *ticket, MakeWant &&want) {
  if (!s || !ticket) return fail(FDNN_E_ARG, "null argument");
  if (!raw) return submit_frames(s, nullptr, frames, n, 0, n, ticket, want);
  const fdnn::SpliceRef spec = s->m->splice;
  return submit_frames(s, &spec, frames, n, 0, n, ticket, want);
}

// A set submission's Want: the set validated and copied (the caller may release it at once).
int want_set(fdnn_server *s, int n, const int32_t *nodes, int len, float *probs, float *inactive, WantOut *w) {
  const int O = s->m->hm.hdr.out_dim;
  if (len < 0 || (len > 0 && !nodes)) return fail(FDNN_E_ARG, "bad node set");
  const int32_t row_ptr[2] = {0, len};
  if (fdnn::lists::check(row_ptr, nodes, 1, O))
    return fail(FDNN_E_ARG, "node set: the nodes must ascend strictly inside [0, " + std::to_string(O) + ")");
  if (!inactive || (len > 0 && !probs)) return fail(FDNN_E_ARG, "null buffer");
  if (static_cast<long long>(n) * len > INT32_MAX) return fail(FDNN_E_ARG, "n x len must fit an int32");
  *w = Want::set_to(std::make_shared<const std::vector<int32_t>>(nodes, nodes + len), probs, inactive);
  return FDNN_OK;
}

int want_topk(fdnn_server *s, int k, int32_t *nodes, float *probs, WantOut *w) {
  if (!fdnn::topk::args_ok(s->m->hm.hdr.out_dim, k)) return fail(FDNN_E_ARG, "k is 1 .. min(output_dim, 256)");
  if (!nodes || !probs) return fail(FDNN_E_ARG, "null buffer");
  *w = Want::topk_to(k, nodes, probs);
  return FDNN_OK;
}

int want_pool(fdnn_server *s, const fdnn_pool *pool, float *out, WantOut *w) {
  if (int rc = fdnn::check_pool(s->m, pool)) return rc;
  if (!out) return fail(FDNN_E_ARG, "null buffer");
  *w = Want::pool_to(pool, pool->n_classes, out);
  return FDNN_OK;
}

int want_loglik(fdnn_server *s, const fdnn_loglik *ll, void *out, WantOut *w) {
  if (int rc = fdnn::check_loglik(s->m, ll)) return rc;
  if (!out) return fail(FDNN_E_ARG, "null buffer");
  *w = Want::loglik_to(ll, fdnn::loglik::elem_bytes(ll->type), out);
  return FDNN_OK;
}

// rows, behind byte masks or bit words where the caller gives some (the widest row is counted here, on the submitting thread)
int want_rows(fdnn_server *s, int n, const int8_t *masks, const uint64_t *bits, float *out, WantOut *w) {
  if (!out) return fail(FDNN_E_ARG, "null buffer");
  *w = bits    ? Want::rows_behind_bits_to(bits, widest_row(bits, n, size_t(s->m->hm.hdr.out_dim)), out)
       : masks ? Want::rows_behind_bytes_to(masks, out)
               : Want::rows_to(out);
  return FDNN_OK;
}

}  // namespace

// A live utterance of the loop (fdnn_server_live_*): where it stands, and its window -- the last L + R frames plus the last
// push's new ones -- on the host.  Every push makes a new window (at most L + R + max_chunk frames, 156 B each) and hands it to
// its request, so a queued push never reads the caller's memory or this handle: reset and close need not wait for anything.
struct fdnn_live {
  fdnn_server *s = nullptr;
  fdnn::SpliceRef spec;  // the model's spec when the handle was opened: every push is spliced by it
  int max_chunk = 0;
  fdnn::stream::Window w;
  WindowRef window;
};

namespace {

// The one path of every live push.  The position arithmetic is fdnn_stream_push's (fdnn_stream_plan.hpp); the rows the push
// completes are rows [a, a + rows) of the window, submitted as any raw rows are (submit_frames).  want(rows, &w): the entry's
// Want for that many rows -- built for a push that completes none as well, so that a bad argument fails at the first push
// and not at whichever push first has rows.  The handle moves on only when the push has been accepted.
template <class MakeWant>
int live_push(fdnn_live *l, const float *raw, int n_raw, int end, int *n_out, uint64_t *ticket, MakeWant &&want) {
  if (!l || !n_out || !ticket) return fail(FDNN_E_ARG, "null argument");
  *n_out = 0;
  *ticket = 0;
  if (l->w.ended) return fail(FDNN_E_STATE, "the utterance has ended: fdnn_server_live_reset starts the next one");
  if (n_raw < 0 || n_raw > l->max_chunk) return fail(FDNN_E_ARG, "a push holds 0 .. max_chunk raw frames");
  if (n_raw > 0 && !raw) return fail(FDNN_E_ARG, "null raw frames");
  // the push's window: the kept frames and the new ones, copied (the caller may overwrite its frames at once)
  fdnn::stream::HostPush p = fdnn::stream::host_push(l->w, l->window, *l->spec, raw, n_raw, end != 0);
  const fdnn::stream::Rows &done = p.done;
  if (done.rows > 0) {
    const int rc = submit_frames(l->s, &l->spec, p.window->data(), done.raw_n, done.a, done.a + done.rows, ticket,
                                 [&](WantOut *o) { return want(done.rows, o); }, p.window);
    if (rc) return rc;
  } else {  // nothing to score and nothing to wait for; the arguments are held to the same checks
    WantOut o;
    if (int rc = want(0, &o)) return rc;
  }
  l->w = p.after;
  l->window = std::move(p.window);
  *n_out = done.rows;
  return FDNN_OK;
}

}  // namespace

namespace fdnn {

int server_submit_raw_rows(fdnn_server *s, const SpliceRef &spec, const float *raw, int n, int a, int b, const uint64_t *bits,
                           float *out, uint64_t *ticket) {
  return submit_frames(s, &spec, raw, n, a, b, ticket, [&](WantOut *w) { return want_rows(s, b - a, nullptr, bits, out, w); });
}

}  // namespace fdnn

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
  int rc = enqueue_pass(s, sl, n, nullptr, fdnn::pass::Pass::loop_rows(d_x, d_masks, nullptr, d_out), &last, [](hipStream_t) {});
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
  return submit_entry(s, kRows, x, n, ticket, [&](WantOut *w) { return want_rows(s, n, masks, nullptr, out, w); });
}

int fdnn_server_submit_lazy_bits(fdnn_server *s, const float *x, int n, const uint64_t *bits, float *out, uint64_t *ticket) {
  return submit_entry(s, kRows, x, n, ticket, [&](WantOut *w) { return bits ? want_rows(s, n, nullptr, bits, out, w) : fail(FDNN_E_ARG, "null buffer"); });
}

int fdnn_server_submit_raw(fdnn_server *s, const float *raw, int n, const uint64_t *bits, float *out, uint64_t *ticket) {
  return submit_entry(s, kRaw, raw, n, ticket, [&](WantOut *w) { return want_rows(s, n, nullptr, bits, out, w); });
}

int fdnn_server_submit_lazy_set(fdnn_server *s, const float *x, int n, const int32_t *nodes, int len, float *probs, float *inactive,
                                uint64_t *ticket) {
  return submit_entry(s, kRows, x, n, ticket, [&](WantOut *w) { return want_set(s, n, nodes, len, probs, inactive, w); });
}

int fdnn_server_submit_raw_set(fdnn_server *s, const float *raw, int n, const int32_t *nodes, int len, float *probs, float *inactive,
                               uint64_t *ticket) {
  return submit_entry(s, kRaw, raw, n, ticket, [&](WantOut *w) { return want_set(s, n, nodes, len, probs, inactive, w); });
}

int fdnn_server_submit_topk(fdnn_server *s, const float *x, int n, int k, int32_t *nodes, float *probs, uint64_t *ticket) {
  return submit_entry(s, kRows, x, n, ticket, [&](WantOut *w) { return want_topk(s, k, nodes, probs, w); });
}

int fdnn_server_submit_raw_topk(fdnn_server *s, const float *raw, int n, int k, int32_t *nodes, float *probs, uint64_t *ticket) {
  return submit_entry(s, kRaw, raw, n, ticket, [&](WantOut *w) { return want_topk(s, k, nodes, probs, w); });
}

int fdnn_server_submit_pool(fdnn_server *s, const float *x, int n, const fdnn_pool *pool, float *out, uint64_t *ticket) {
  return submit_entry(s, kRows, x, n, ticket, [&](WantOut *w) { return want_pool(s, pool, out, w); });
}

int fdnn_server_submit_raw_pool(fdnn_server *s, const float *raw, int n, const fdnn_pool *pool, float *out, uint64_t *ticket) {
  return submit_entry(s, kRaw, raw, n, ticket, [&](WantOut *w) { return want_pool(s, pool, out, w); });
}

int fdnn_server_submit_loglik(fdnn_server *s, const float *x, int n, const fdnn_loglik *ll, void *out, uint64_t *ticket) {
  return submit_entry(s, kRows, x, n, ticket, [&](WantOut *w) { return want_loglik(s, ll, out, w); });
}

int fdnn_server_submit_raw_loglik(fdnn_server *s, const float *raw, int n, const fdnn_loglik *ll, void *out, uint64_t *ticket) {
  return submit_entry(s, kRaw, raw, n, ticket, [&](WantOut *w) { return want_loglik(s, ll, out, w); });
}

int fdnn_server_live_open(fdnn_server *s, int max_chunk, fdnn_live **out) {
  if (!s || !out) return fail(FDNN_E_ARG, "null argument");
  *out = nullptr;
  const fdnn::SpliceRef spec = s->m->splice;
  if (int rc = fdnn::splice_check(spec, -1)) return rc;
  if (max_chunk < 1) return fail(FDNN_E_ARG, "max_chunk must be positive");
  fdnn_live *l = new fdnn_live();
  l->s = s;
  l->spec = spec;
  l->max_chunk = max_chunk;
  *out = l;
  return FDNN_OK;
}

void fdnn_server_live_close(fdnn_live *l) { delete l; }  // (queued pushes own their frames)

int fdnn_server_live_reset(fdnn_live *l) {
  if (!l) return fail(FDNN_E_ARG, "null live handle");
  l->w = fdnn::stream::Window{};
  l->window.reset();
  return FDNN_OK;
}

int fdnn_server_live_position(const fdnn_live *l, int64_t *pushed, int64_t *emitted) {
  if (!l) return fail(FDNN_E_ARG, "null live handle");
  if (pushed) *pushed = l->w.pushed;
  if (emitted) *emitted = l->w.emitted;
  return FDNN_OK;
}

int fdnn_server_live_push(fdnn_live *l, const float *raw, int n_raw, int end, float *out, int *n_out, uint64_t *ticket) {
  return live_push(l, raw, n_raw, end, n_out, ticket, [&](int rows, WantOut *w) { return want_rows(l->s, rows, nullptr, nullptr, out, w); });
}

int fdnn_server_live_push_topk(fdnn_live *l, const float *raw, int n_raw, int end, int k, int32_t *nodes, float *probs, int *n_out,
                               uint64_t *ticket) {
  return live_push(l, raw, n_raw, end, n_out, ticket, [&](int, WantOut *w) { return want_topk(l->s, k, nodes, probs, w); });
}

int fdnn_server_live_push_pool(fdnn_live *l, const float *raw, int n_raw, int end, const fdnn_pool *pool, float *out, int *n_out,
                               uint64_t *ticket) {
  return live_push(l, raw, n_raw, end, n_out, ticket, [&](int, WantOut *w) { return want_pool(l->s, pool, out, w); });
}

int fdnn_server_live_push_loglik(fdnn_live *l, const float *raw, int n_raw, int end, const fdnn_loglik *ll, void *out, int *n_out,
                                 uint64_t *ticket) {
  return live_push(l, raw, n_raw, end, n_out, ticket, [&](int, WantOut *w) { return want_loglik(l->s, ll, out, w); });
}

int fdnn_server_live_push_set(fdnn_live *l, const float *raw, int n_raw, int end, const int32_t *nodes, int len, float *probs,
                              float *inactive, int *n_out, uint64_t *ticket) {
  return live_push(l, raw, n_raw, end, n_out, ticket,
                   [&](int rows, WantOut *w) { return want_set(l->s, rows, nodes, len, probs, inactive, w); });
}

int fdnn_debug_server_hold(fdnn_server *s, int on) {
  if (!s) return fail(FDNN_E_ARG, "null argument");
  {
    std::lock_guard<std::mutex> lk(s->qmu);
    s->hold = on != 0;
  }
  s->qcv.notify_all();  // (switched off: the packer looks at the queue again)
  return FDNN_OK;
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
