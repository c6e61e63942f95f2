// fdnn_stream_plan.hpp -- where an utterance that arrives chunk by chunk stands: which raw frames are still needed, which rows
// a push completes, and how those rows index the frames that are kept.  One arithmetic for both kinds of stream: fdnn_stream_*
// (fdnn_api.cpp) keeps its window on the device and splices it with the window's SpliceSeg; a live handle of the scoring loop
// (fdnn_server_live_*, fdnn_server.cpp) keeps it on the host and hands the loop rows [a, a + rows) of the window as if the
// window were a short utterance of its own.  Free of HIP: tests/host/stream_plan_check.cpp runs it under the sanitizers.
//
// The window holds the utterance's frames [base, base + len), base + len == pushed.  Row t reads frames t - L .. t + R (L / R:
// SpliceSpec::left / right), is complete once frame t + R has arrived, and at the end of the utterance every remaining row is
// complete, right-clamped to the last frame.  Between pushes the window keeps frames from emitted - L on: at most L + R.
#pragma once
#include <algorithm>
#include <memory>
#include <vector>

#include "fdnn_splice_spec.hpp"

namespace fdnn::stream {

struct Window {
  long long base = 0, len = 0, pushed = 0, emitted = 0;
  bool ended = false;
};

// Before a push: the frames that rows not emitted yet still read are [drop, drop + kept) of the window as it stands.  moved:
// they are not the whole window, the caller moves them to the front.  The window then starts at them.
struct Keep {
  long long drop = 0, kept = 0;
  bool moved = false;
};
inline Keep keep_frames(Window &w, int left) {
  Keep k;
  const long long keep = std::max(w.base, w.emitted - left);
  k.kept = w.len;
  if (keep > w.base) {
    k.moved = true;
    k.drop = keep - w.base;
    k.kept = w.base + w.len - keep;
    w.base = keep;
    w.len = k.kept;
  }
  return k;
}

// The push's n_raw new frames go behind the kept ones: the window index of the first of them.
inline long long append_frames(Window &w, int n_raw) {
  const long long at = w.len;
  w.len += n_raw;
  w.pushed += n_raw;
  return at;
}

// The rows the push completes: utterance rows [w.emitted, upto), `rows` of them.
//   seg      the window's splice segment: row 0 of the push reads window frame seg.center + o, clamped to [seg.lo, seg.hi] --
//            seg.lo is frame 0 of the utterance as a window index (negative once the window has moved on: no row that is still
//            to come reads that far back), seg.hi the last frame pushed
//   a, raw_n the same rows as rows [a, a + rows) of a raw_n-frame utterance that is the window itself: its left edge is the
//            utterance's while base == 0, and is never reached afterwards (base <= emitted - L then); its right edge is the
//            last frame pushed, which only the rows of an `end` reach
struct Rows {
  long long upto = 0;
  int rows = 0, a = 0, raw_n = 0;
  SpliceSeg seg{0, 0, 0, 0};
};
inline Rows complete_rows(const Window &w, int right, bool end) {
  Rows r;
  r.upto = end ? w.pushed : std::max(w.emitted, w.pushed - right);
  r.rows = int(r.upto - w.emitted);
  r.a = int(w.emitted - w.base);
  r.raw_n = int(w.len);
  const int lo = int(std::max(-w.base, -(1LL << 30)));  // global frame 0 -- the left clamp -- as a window index
  r.seg = SpliceSeg{0, r.a, lo, int(w.pushed - 1 - w.base)};
  return r;
}

// The push has succeeded: its rows are emitted, and `end` closes the utterance.
inline void commit(Window &w, const Rows &r, bool end) {
  w.emitted = r.upto;
  w.ended = end;
}

// A window kept on the HOST (the scoring loop's live handles): one push as a value.  The push's window is a new array -- the
// kept frames of `before`'s window, then the n_raw new ones, [frames][spec.raw_dim] -- that whoever scores the rows can own:
// nothing of it is the caller's memory or the handle's.  `after`: where the utterance stands once the push is accepted; the
// handle takes it, and the window, only then.  At most L + R + n_raw frames.
using Frames = std::shared_ptr<const std::vector<float>>;
struct HostPush {
  Window after;
  Frames window;
  Rows done;
};
inline HostPush host_push(const Window &before, const Frames &kept, const SpliceSpec &spec, const float *raw, int n_raw, bool end) {
  HostPush p;
  p.after = before;
  const size_t D = size_t(spec.raw_dim);
  const Keep k = keep_frames(p.after, spec.left);
  auto win = std::make_shared<std::vector<float>>();
  win->reserve(size_t(k.kept + n_raw) * D);
  if (k.kept > 0) win->insert(win->end(), kept->begin() + size_t(k.drop) * D, kept->begin() + size_t(k.drop + k.kept) * D);
  append_frames(p.after, n_raw);
  if (n_raw > 0) win->insert(win->end(), raw, raw + size_t(n_raw) * D);
  p.done = complete_rows(p.after, spec.right, end);
  commit(p.after, p.done, end);
  p.window = std::move(win);
  return p;
}

}  // namespace fdnn::stream
