// stream_plan_check.cpp -- where a chunked utterance stands (fdnn_stream_plan.hpp) and how the scoring loop batches live pushes
// (fdnn_server_plan.hpp), checked without a GPU.  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_live_host.py; exit status 0 = all cases hold.
//
// Every raw frame carries its identity in its first float: 1000 * utterance + frame.  A row is right when every frame it
// reads -- followed through the window, its segment, and for batches the staged copy and the device table's words -- is frame
// clamp(t + o, 0, last) of its own utterance.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>

#include "fdnn_server_plan.hpp"
#include "fdnn_stream_plan.hpp"

using namespace fdnn::plan;
using fdnn::SpliceRef;
using fdnn::SpliceSeg;
using fdnn::SpliceSpec;
namespace st = fdnn::stream;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }

SpliceRef make_spec(std::vector<int> offsets, int raw_dim) {
  auto sp = std::make_shared<SpliceSpec>();
  sp->offsets = std::move(offsets);
  sp->raw_dim = raw_dim;
  for (int o : sp->offsets) sp->left = std::max(sp->left, -o), sp->right = std::max(sp->right, o);
  return sp;
}

// the five specs of tests/test_gpu_splice.py: Kaldi +-5 x 39, three offsets x 144, identity x 432, left-only, duplicates out of order
std::vector<SpliceRef> specs() {
  std::vector<int> kaldi, left;
  for (int o = -5; o <= 5; ++o) kaldi.push_back(o);
  for (int o = -10; o <= 0; ++o) left.push_back(o);
  return {make_spec(kaldi, 39), make_spec({-2, 0, 3}, 144), make_spec({0}, 432), make_spec(left, 39), make_spec({2, -1, 2, 0, -1, 5}, 64)};
}

float frame_id(int utt, int f) { return float(1000 * utt + f); }

std::vector<float> utterance(int utt, int n, int D) {
  std::vector<float> raw(size_t(n) * size_t(D));
  for (int f = 0; f < n; ++f) {
    for (int j = 0; j < D; ++j) raw[size_t(f) * D + j] = float(j) + 0.5f;
    raw[size_t(f) * D] = frame_id(utt, f);
  }
  return raw;
}

// A feed: the utterance in chunks, each chunk copied into a buffer of the caller's that is overwritten right after the push.
struct Feed {
  int utt, n, max_chunk;
  SpliceRef spec;
  std::vector<float> raw;
  std::vector<int> chunks;  // frames per push, in order; the last push carries `end`
  size_t next = 0;
  int fed = 0, rows = 0;    // frames pushed, rows emitted
  st::Window w;
  st::Frames window;
  bool done() const { return next == chunks.size(); }
  // one push: the HostPush, with every property of a single push checked
  st::HostPush push() {
    const int D = spec->raw_dim, L = spec->left, R = spec->right;
    const int c = chunks[next];
    const bool end = ++next == chunks.size();
    std::vector<float> callers(size_t(std::max(c, 1)) * size_t(D));
    if (c > 0) std::memcpy(callers.data(), raw.data() + size_t(fed) * D, sizeof(float) * size_t(c) * D);
    st::HostPush p = st::host_push(w, window, *spec, c > 0 ? callers.data() : nullptr, c, end);
    std::fill(callers.begin(), callers.end(), -7.0f);  // the ring buffer moves on
    fed += c;
    const st::Window &a = p.after;
    const size_t frames = p.window->size() / size_t(D);
    CHECK(p.window->size() == frames * size_t(D) && (long long)frames == a.len && a.base + a.len == a.pushed && a.pushed == fed);
    CHECK(int(frames) <= L + R + max_chunk);  // the window never exceeds L + R + max_chunk
    for (size_t i = 0; i < frames; ++i) CHECK((*p.window)[i * size_t(D)] == frame_id(utt, int(a.base) + int(i)));
    // the rows: the next ones in order; complete exactly when t + R has arrived, all of them at the end
    const st::Rows &d = p.done;
    CHECK(d.rows >= 0 && d.upto - d.rows == rows && a.emitted == d.upto && a.ended == end);
    CHECK(d.upto == (end ? fed : std::max<long long>(rows, fed - R)));
    CHECK(d.rows <= c + R && d.raw_n == int(frames));
    for (int r = 0; r < d.rows; ++r) {
      const int t = rows + r;
      for (int o : spec->offsets) {
        const float want = frame_id(utt, clampi(t + o, 0, n - 1));
        const int f = clampi(d.seg.center + (r - d.seg.row) + o, d.seg.lo, d.seg.hi);  // the window's segment (fdnn_stream_push)
        CHECK(f >= 0 && f < int(frames) && (*p.window)[size_t(f) * D] == want);
        const int g = clampi(d.a + r + o, 0, d.raw_n - 1);  // rows [a, a + rows) of the window as an utterance (the live handle)
        CHECK((*p.window)[size_t(g) * D] == want);
      }
    }
    rows += d.rows;
    w = p.after;
    window = p.window;
    return p;
  }
};

enum Chunking { ALL_ONE, ALL_MAX, RANDOM };

Feed make_feed(int utt, const SpliceRef &spec, int n, int max_chunk, Chunking how, bool flush_only, std::mt19937 &rng) {
  Feed f{utt, n, max_chunk, spec, utterance(utt, n, spec->raw_dim), {}};
  for (int left = n; left > 0;) {
    int c = how == ALL_ONE ? 1 : how == ALL_MAX ? max_chunk : int(rng() % unsigned(max_chunk + 1));  // (RANDOM: empty pushes too)
    c = std::min(c, left);
    f.chunks.push_back(c);
    left -= c;
  }
  if (flush_only) f.chunks.push_back(0);  // n_raw == 0 with end
  return f;
}

void positions() {
  std::mt19937 rng(1);
  int utt = 0;
  for (const SpliceRef &spec : specs()) {
    const int L = spec->left, R = spec->right;
    for (int n : {1, 2, std::max(L, 1), L + R + 1, 300})
      for (Chunking how : {ALL_ONE, ALL_MAX, RANDOM})
        for (bool flush_only : {false, true})
          for (int max_chunk : {3, 16}) {
            Feed f = make_feed(++utt % 1000, spec, n, how == ALL_ONE ? 1 : max_chunk, how, flush_only, rng);
            while (!f.done()) f.push();
            CHECK(f.rows == n && f.fed == n && f.w.ended);  // rows 0 .. n - 1, once each and in order (push() checks the order)
          }
  }
}

// A queue that mixes live pushes of several handles (two and more of one handle among them) with whole raw utterances, drained
// by plan_batch: every row of every batch, followed through raw_src, the staged copy and the segment -- and through the words of
// the device table -- reads the frame the definition names.  The handles are reset and gone before anything is planned.
void batches(const SpliceRef &spec, int max_frames, unsigned seed) {
  std::mt19937 rng(seed);
  const int D = spec->raw_dim;
  struct Asked { int utt, n, t0, rows; bool live; };  // rows [t0, t0 + rows) of utterance utt (n frames)
  std::map<uint64_t, Asked> asked;
  std::deque<Request> q;
  std::vector<std::vector<float>> whole;  // whole raw utterances: the caller keeps these
  uint64_t ticket = 0;
  float sink = 0;
  {
    std::vector<Feed> feeds;
    for (int h = 0; h < 6; ++h) feeds.push_back(make_feed(h + 1, spec, 3 + int(rng() % 40), 4, RANDOM, rng() % 2, rng));
    for (bool any = true; any;) {
      any = false;
      for (Feed &f : feeds) {
        if (f.done()) continue;
        any = true;
        const int t0 = f.rows;
        const st::HostPush p = f.push();
        if (p.done.rows > 0) {
          Request r(Frames::live_rows(p.window, spec, p.done.raw_n, p.done.a), Want::rows_to(&sink), p.done.rows);
          r.ticket = ++ticket;
          q.push_back(r);
          asked[ticket] = Asked{f.utt, f.n, t0, p.done.rows, true};
        }
        if (rng() % 5 == 0) {  // a whole raw utterance between the pushes
          const int utt = 100 + int(whole.size()), n = 1 + int(rng() % 30);
          whole.push_back(utterance(utt, n, D));
          Request r(Frames::raw_rows(whole.back().data(), spec, n, 0), Want::rows_to(&sink), n);
          r.ticket = ++ticket;
          q.push_back(r);
          asked[ticket] = Asked{utt, n, 0, n, false};
        }
      }
    }
    for (Feed &f : feeds) f.w = st::Window{}, f.window.reset();  // reset ...
  }  // ... and closed: the queued requests own their frames
  std::map<uint64_t, int> covered;
  while (!q.empty()) {
    const BatchPlan b = plan_batch(q, max_frames, 70);
    CHECK(b.raw && b.spec == spec && b.segs.size() == b.pieces.size() && b.raw_src.size() == b.pieces.size());
    bool live = false;
    for (const Request &r : b.taken) live |= r.frames.window != nullptr;
    CHECK(b.live == live);
    // stage as the loop does: the pieces' frames back to back, the table behind them
    const LiveTable t = live_table(b);
    CHECK(t.segs_at % 4 == 0 && t.segs_at >= size_t(b.raw_frames) * size_t(D) && t.row_seg_at == t.segs_at + 4 * b.segs.size());
    CHECK(t.words == t.row_seg_at + size_t(b.rows));
    std::vector<float> staged(t.words, -1.0f);
    for (size_t i = 0; i < b.pieces.size(); ++i) {
      const RawSrc &src = b.raw_src[i];
      std::memcpy(staged.data() + size_t(src.at) * D, b.taken[i].frames.raw + size_t(src.first) * D, sizeof(float) * size_t(src.count) * D);
    }
    write_live_table(b, t, reinterpret_cast<int32_t *>(staged.data()));
    const int32_t *words = reinterpret_cast<const int32_t *>(staged.data());
    for (size_t i = 0; i < b.pieces.size(); ++i) {
      const Piece &p = b.pieces[i];
      const Asked &a = asked.at(p.ticket);
      CHECK(b.taken[i].taken == covered[p.ticket]);
      for (int r = p.row0; r < p.row0 + p.rows; ++r) {
        const int u = a.t0 + covered[p.ticket] + (r - p.row0);  // the row, as a row of its utterance
        const int g = words[t.row_seg_at + size_t(r)];
        CHECK(g == int(i));
        const int32_t *sg = words + t.segs_at + 4 * size_t(g);
        CHECK(sg[0] == b.segs[i].row && sg[1] == b.segs[i].center && sg[2] == b.segs[i].lo && sg[3] == b.segs[i].hi && sg[0] == p.row0);
        for (int o : spec->offsets) {
          const int f = clampi(sg[1] + (r - sg[0]) + o, std::max(sg[2], 0), std::min(sg[3], b.raw_frames - 1));  // what the kernel reads
          CHECK(f >= b.raw_src[i].at && f < b.raw_src[i].at + b.raw_src[i].count);                               // this piece's own
          CHECK(staged[size_t(f) * D] == frame_id(a.utt, clampi(u + o, 0, a.n - 1)));
        }
      }
      covered[p.ticket] += p.rows;
      CHECK(p.last == (covered[p.ticket] == a.rows));
    }
  }
  for (const auto &kv : asked) CHECK(covered[kv.first] == kv.second.rows);
}

}  // namespace

int main() {
  positions();
  unsigned seed = 0;
  for (const SpliceRef &spec : specs())
    for (int max_frames : {5, 64, 4096}) batches(spec, max_frames, ++seed);
  std::puts("stream plan ok");
  return 0;
}
