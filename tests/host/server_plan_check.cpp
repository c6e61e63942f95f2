// server_plan_check.cpp -- what a batch of the scoring loop must contain (fdnn_server_plan.hpp), checked without a GPU.
// Built with -fsanitize=address,undefined and run as a child process by tests/test_server_plan_host.py; exit status 0 = all
// cases hold.  O = 70: two mask words per row, the second partial.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>

#include "fdnn_server_plan.hpp"

using namespace fdnn::plan;
using fdnn::SpliceRef;
using fdnn::SpliceSeg;
using fdnn::SpliceSpec;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

constexpr size_t O = 70, WPR = 2;
enum Kind { DENSE, BYTES, BITS, RAW, RAW_BITS };

// the callers' memory: real blocks, so that every pointer the plan derives is in bounds under the sanitizers
struct Caller {
  std::vector<float> out;
  std::vector<uint64_t> bits;
  float x = 0, raw = 0;  // (the plan never offsets these two)
  int8_t masks = 1;
};

SpliceRef make_spec(int lo, int hi) {
  auto sp = std::make_shared<SpliceSpec>();
  for (int o = lo; o <= hi; ++o) sp->offsets.push_back(o);
  sp->raw_dim = 39;
  sp->left = std::max(-lo, 0);
  sp->right = std::max(hi, 0);
  return sp;
}

struct Queue {
  std::deque<Request> q;
  std::vector<std::unique_ptr<Caller>> callers;
  std::map<uint64_t, Request> asked;  // by ticket, as submitted
  // rows [a, a + n) of a raw_n-frame utterance for the raw kinds; `most` as the submitter would have counted it
  uint64_t add(Kind k, int n, int most = 0, const SpliceRef &spec = nullptr, int raw_n = 0, int a = 0) {
    callers.emplace_back(new Caller());
    Caller &c = *callers.back();
    c.out.resize(size_t(n) * O);
    Request r;
    r.ticket = callers.size();
    r.out = c.out.data();
    r.n = n;
    if (k == BYTES) r.masks = &c.masks;
    if (k == BITS || k == RAW_BITS) {
      c.bits.resize(size_t(n) * WPR);
      r.bits = c.bits.data();
      r.most = most;
    }
    if (k == RAW || k == RAW_BITS) {
      r.raw = &c.raw;
      r.spec = spec;
      r.raw_n = raw_n ? raw_n : n;
      r.raw_a = a;
    } else {
      r.x = &c.x;
    }
    q.push_back(r);
    asked[r.ticket] = r;
    return r.ticket;
  }
};

int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }

// Every rule a single batch must keep, and for raw batches: every row of every piece reads, through its segment and the
// staged frames, exactly the frames of ITS utterance that the splice asks for.
void check_batch(const BatchPlan &b, int max_frames, const std::map<uint64_t, Request> &asked) {
  CHECK(b.rows > 0 && b.rows <= max_frames);
  CHECK(b.taken.size() == b.pieces.size());
  CHECK(b.raw_src.size() == (b.raw ? b.pieces.size() : 0) && b.segs.size() == b.raw_src.size());
  int row = 0, at = 0, most = 0;
  bool any_mask = false, bytes = false;
  for (size_t i = 0; i < b.pieces.size(); ++i) {
    const Piece &p = b.pieces[i];
    const Request &part = b.taken[i], &whole = asked.at(p.ticket);
    CHECK(part.ticket == p.ticket && part.n == p.rows && p.rows > 0);
    CHECK(p.row0 == row);  // the pieces tile [0, rows) without gap or overlap
    row += p.rows;
    CHECK(part.taken >= 0 && part.taken + p.rows <= whole.n);
    CHECK(p.out == whole.out + size_t(part.taken) * O);
    CHECK(p.bits == (whole.bits ? whole.bits + size_t(part.taken) * WPR : nullptr));
    CHECK(p.last == (part.taken + p.rows == whole.n) && p.state == 0);
    CHECK((kind_of(whole) == kBits) == (b.kind == kBits));  // bit masks never share a batch with another kind
    CHECK((whole.raw != nullptr) == b.raw && whole.spec == b.spec);  // nor raw with spliced rows, nor two spec objects
    any_mask |= whole.masks != nullptr;
    bytes |= kind_of(whole) == kBytes;
    most = std::max(most, whole.most);
    if (!b.raw) continue;
    const RawSrc &src = b.raw_src[i];
    const SpliceSeg &sg = b.segs[i];
    CHECK(src.at == at && src.count > 0 && src.first >= 0 && src.first + src.count <= whole.raw_n);
    at += src.count;
    CHECK(sg.row == p.row0);
    for (int t = p.row0; t < p.row0 + p.rows; ++t) {
      const int u = whole.raw_a + part.taken + (t - p.row0);  // the row's own frame of its utterance
      for (int o : b.spec->offsets) {
        const int f = clampi(sg.center + (t - sg.row) + o, sg.lo, sg.hi);  // what the splice kernel reads (SpliceSeg)
        CHECK(f >= src.at && f < src.at + src.count);                      // staged, and this piece's own
        CHECK(src.first + (f - src.at) == clampi(u + o, 0, whole.raw_n - 1));
      }
    }
  }
  CHECK(row == b.rows && at == b.raw_frames && most == b.most && any_mask == b.any_mask);
  if (b.kind != kBits) CHECK(b.kind == (bytes ? kBytes : kDense));
  CHECK(b.stride == (b.kind == kBits && 4 * (size_t(b.most) + 1) <= 3 * O ? b.most + 1 : 0));
}

// Drains the queue; every batch is checked, and over all batches every request's pieces cover [0, n) once, in order.
std::vector<BatchPlan> drain(Queue &Q, int max_frames) {
  std::vector<BatchPlan> out;
  std::map<uint64_t, int> covered;
  std::map<uint64_t, bool> closed;
  while (!Q.q.empty()) {
    const size_t before = Q.q.size();
    const int front_taken = Q.q.front().taken;
    out.push_back(plan_batch(Q.q, max_frames, O));
    const BatchPlan &b = out.back();
    check_batch(b, max_frames, Q.asked);
    CHECK(Q.q.size() < before || Q.q.front().taken > front_taken);  // (progress)
    for (size_t i = 0; i < b.pieces.size(); ++i) {
      const uint64_t t = b.pieces[i].ticket;
      CHECK(!closed[t] && b.taken[i].taken == covered[t]);
      covered[t] += b.pieces[i].rows;
      closed[t] = b.pieces[i].last;
    }
  }
  for (const auto &kv : Q.asked) CHECK(covered[kv.first] == kv.second.n && closed[kv.first]);
  return out;
}

void expect_pieces(const BatchPlan &b, std::vector<std::array<int, 3>> want) {  // (row0, rows, last)
  CHECK(b.pieces.size() == want.size());
  for (size_t i = 0; i < want.size(); ++i)
    CHECK(b.pieces[i].row0 == want[i][0] && b.pieces[i].rows == want[i][1] && b.pieces[i].last == (want[i][2] != 0));
}

void kinds_and_strides() {
  {  // dense 40 + 40 + 40 at max_frames = 100
    Queue Q;
    for (int i = 0; i < 3; ++i) Q.add(DENSE, 40);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 2 && bs[0].kind == kDense && !bs[0].any_mask && !bs[0].raw && bs[0].stride == 0);
    expect_pieces(bs[0], {{0, 40, 1}, {40, 40, 1}, {80, 20, 0}});
    expect_pieces(bs[1], {{0, 20, 1}});
    CHECK(bs[0].pieces[2].out == Q.asked[3].out && bs[1].pieces[0].out == Q.asked[3].out + 20 * O);  // taken * O
    CHECK(bs[1].taken[0].taken == 20 && bs[1].rows == 20);
  }
  {  // dense, bytes, dense: one byte-mask batch
    Queue Q;
    Q.add(DENSE, 10), Q.add(BYTES, 10), Q.add(DENSE, 10);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 1 && bs[0].kind == kBytes && bs[0].any_mask && bs[0].pieces.size() == 3);
  }
  {  // bits behind dense: a new batch starts (and dense behind bits)
    Queue Q;
    Q.add(DENSE, 10), Q.add(BITS, 10, 5), Q.add(DENSE, 10);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 3 && bs[0].kind == kDense && bs[1].kind == kBits && bs[2].kind == kDense);
    CHECK(bs[1].stride == 6 && bs[0].stride == 0);
  }
  {  // two bits requests: one batch, the larger `most`, bits offsets in words
    Queue Q;
    Q.add(BITS, 50, 10), Q.add(BITS, 80, 30);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 2 && bs[0].kind == kBits && bs[0].most == 30 && bs[0].stride == 31 && !bs[0].any_mask);
    expect_pieces(bs[0], {{0, 50, 1}, {50, 50, 0}});
    CHECK(bs[0].pieces[1].bits == Q.asked[2].bits && bs[1].pieces[0].bits == Q.asked[2].bits + 50 * 2);
  }
  for (int most : {51, 52}) {  // the stride boundary at O = 70: 4 * 52 = 208 <= 210 < 4 * 53
    Queue Q;
    Q.add(BITS, 3, most);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 1 && bs[0].stride == (most == 51 ? 52 : 0));
  }
  {  // widest_row counts the first O bits of a row only: the second word's upper 58 bits are not nodes
    std::vector<uint64_t> bits(3 * WPR, 0);
    bits[0] = ~uint64_t(0) >> 17, bits[1] = ~uint64_t(0) << 2;  // 47 + 4 = 51 nodes, and 58 stray bits
    bits[2] = 1, bits[3] = ~uint64_t(63);                       // 1 node
    bits[4] = ~uint64_t(0), bits[5] = 63;                       // all 70
    CHECK(widest_row(bits.data(), 1, O) == 51 && widest_row(bits.data(), 2, O) == 51 && widest_row(bits.data(), 3, O) == 70);
    CHECK(widest_row(bits.data() + 2, 1, O) == 1 && widest_row(bits.data(), 0, O) == 0);
  }
}

void raw_batches() {
  const SpliceRef kaldi = make_spec(-5, 5);
  {  // a 30-frame utterance at max_frames = 16: two pieces in two batches (check_batch walks every row and offset)
    Queue Q;
    Q.add(RAW, 30, 0, kaldi);
    const auto bs = drain(Q, 16);
    CHECK(bs.size() == 2 && bs[0].raw && bs[0].spec == kaldi);
    expect_pieces(bs[0], {{0, 16, 0}});
    expect_pieces(bs[1], {{0, 14, 1}});
    CHECK(bs[0].raw_src[0].first == 0 && bs[0].raw_src[0].count == 21 && bs[0].raw_frames == 21);  // frames 0 .. 20
    CHECK(bs[1].raw_src[0].first == 11 && bs[1].raw_src[0].count == 19);                           // frames 11 .. 29
  }
  {  // two utterances share a batch (neither reads the other's frames), one of them rows [8, 20) of 30 frames, with bits
    Queue Q;
    Q.add(RAW_BITS, 10, 7, kaldi), Q.add(RAW_BITS, 12, 9, kaldi, 30, 8);
    const auto bs = drain(Q, 64);
    CHECK(bs.size() == 1 && bs[0].kind == kBits && bs[0].pieces.size() == 2 && bs[0].stride == 10);
    CHECK(bs[0].raw_src[1].first == 3 && bs[0].raw_src[1].count == 22 && bs[0].raw_src[1].at == 10);
  }
  for (const SpliceRef &sp : {make_spec(-10, 0), make_spec(0, 0), make_spec(2, 5)}) {  // one-sided halos, split three ways
    Queue Q;
    Q.add(RAW, 20, 0, sp), Q.add(RAW, 1, 0, sp), Q.add(RAW, 5, 0, sp, 40, 35);
    drain(Q, 7);
  }
  {  // distinct spec objects (of equal content) do not share a batch; nor do raw and spliced rows, either way round
    Queue Q;
    Q.add(RAW, 5, 0, kaldi), Q.add(RAW, 5, 0, make_spec(-5, 5)), Q.add(DENSE, 5), Q.add(RAW, 5, 0, kaldi);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 4 && bs[0].raw && bs[1].raw && !bs[2].raw && bs[3].raw && bs[0].spec != bs[1].spec);
  }
}

void random_queues() {
  const SpliceRef specs[2] = {make_spec(-5, 5), make_spec(-1, 3)};
  const int sizes[3] = {1, 7, 64};
  for (unsigned seed = 0; seed < 300; ++seed) {
    std::mt19937 rng(seed);
    const int max_frames = sizes[rng() % 3];
    Queue Q;
    const int count = 1 + int(rng() % 10);
    for (int i = 0; i < count; ++i) {
      const Kind k = Kind(rng() % 5);
      const int n = 1 + int(rng() % unsigned(3 * max_frames));
      const int before = int(rng() % 4) * int(rng() % 7), after = int(rng() % 4) * int(rng() % 7);  // often 0: whole utterances
      Q.add(k, n, int(rng() % (O + 1)), specs[rng() % 2], before + n + after, before);
    }
    drain(Q, max_frames);
    CHECK(Q.q.empty());
  }
}

}  // namespace

int main() {
  kinds_and_strides();
  raw_batches();
  random_queues();
  std::puts("server plan ok");
  return 0;
}
