// server_plan_check.cpp -- what a batch of the scoring loop must contain (fdnn_server_plan.hpp), checked without a GPU.
// Built with -fsanitize=address,undefined and run as a child process by tests/test_server_plan_host.py; exit status 0 = all
// cases hold.  O = 70: two mask words per row, the second partial.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
// what a caller wants back, in the order of Want::Kind (a batch's kind is one of them too); raw or not is a second axis
enum Kind { DENSE, BYTES, BITS, SET, TOPK, POOL };
constexpr int kKinds = 6;

// the two pool handles of the cases, C = 3 and C = 5 (never dereferenced by the plan)
const fdnn_pool *handle(int i) { return reinterpret_cast<const fdnn_pool *>(static_cast<uintptr_t>(0x1000 + 0x100 * i)); }
constexpr int kClasses[2] = {3, 5};

// A caller's block with one guard word on either side: every pointer the plan derives is in bounds under the sanitizers,
// and a scatter that writes beside the block is seen.
template <class T>
struct Block {
  std::vector<T> mem;
  static T guard() { T g; std::memset(&g, 0xA5, sizeof g); return g; }
  void resize(size_t n) { mem.assign(n + 2, guard()); }
  T *data() { return mem.data() + 1; }
  const T *data() const { return mem.data() + 1; }
  size_t size() const { return mem.size() - 2; }
  bool guards_whole() const { const T g = guard(); return !std::memcmp(&mem.front(), &g, sizeof g) && !std::memcmp(&mem.back(), &g, sizeof g); }
};

// the callers' memory of one request, whatever its kind
struct Caller {
  Block<float> out, probs, inactive, topk_probs, pooled;
  Block<int32_t> topk_nodes;
  std::vector<uint64_t> bits;
  std::vector<int8_t> masks;
  float x = 0, raw = 0;  // (the plan never offsets these two)
};

// A request as the case asked for it: what the plan's pieces are compared with.  to_request, view(Request) and view(Piece)
// below are the only code of this file that names the fields of a Request, a Want or a Piece.
struct Ask {
  uint64_t ticket = 0;
  Kind kind = DENSE;
  int n = 0;
  float *out = nullptr;
  const int8_t *masks = nullptr;
  const uint64_t *bits = nullptr;
  int most = 0;
  SetRef set;
  float *probs = nullptr, *inactive = nullptr;
  int k = 0;
  int32_t *topk_nodes = nullptr;
  float *topk_probs = nullptr;
  const fdnn_pool *pool = nullptr;
  int classes = 0;
  float *pooled = nullptr;
  bool is_raw = false;
  const float *x = nullptr, *raw = nullptr;
  SpliceRef spec;
  int raw_n = 0, raw_a = 0;
};

Request to_request(const Ask &a) {
  const Frames f = a.is_raw ? Frames::raw_rows(a.raw, a.spec, a.raw_n, a.raw_a) : Frames::rows(a.x);
  const Want w = a.kind == DENSE  ? Want::rows_to(a.out)
                 : a.kind == BYTES ? Want::rows_behind_bytes_to(a.masks, a.out)
                 : a.kind == BITS  ? Want::rows_behind_bits_to(a.bits, a.most, a.out)
                 : a.kind == SET   ? Want::set_to(a.set, a.probs, a.inactive)
                 : a.kind == TOPK  ? Want::topk_to(a.k, a.topk_nodes, a.topk_probs)
                                   : Want::pool_to(a.pool, a.classes, a.pooled);
  Request r(f, w, a.n);
  r.ticket = a.ticket;
  return r;
}

Ask view(const Want &w) {
  Ask a;
  a.kind = Kind(int(w.kind));
  a.out = w.out, a.masks = w.masks, a.bits = w.bits, a.most = w.most;
  a.set = w.nodes, a.probs = w.probs, a.inactive = w.inactive;
  a.k = w.k, a.topk_nodes = w.topk_nodes, a.topk_probs = w.topk_probs;
  a.pool = w.map, a.classes = w.classes, a.pooled = w.pooled;
  return a;
}
Ask view(const Request &r) {
  Ask a = view(r.want);
  a.ticket = r.ticket, a.n = r.n;
  a.is_raw = r.frames.kind == Frames::raw_frames, a.x = r.frames.x, a.raw = r.frames.raw, a.spec = r.frames.spec;
  a.raw_n = r.frames.raw_n, a.raw_a = r.frames.raw_a;
  return a;
}
Ask view(const Piece &p) {
  Ask a = view(p.want);
  a.ticket = p.ticket;
  return a;
}

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
  std::map<uint64_t, Ask> asked;  // by ticket, as submitted
  // `param`: BITS -- `most` as the submitter would have counted it; SET -- the set's length; TOPK -- k; POOL -- which of the
  // two handles.  A spec makes the request a raw one: rows [a, a + n) of a raw_n-frame utterance.
  uint64_t add(Kind k, int n, int param = 0, const SpliceRef &spec = nullptr, int raw_n = 0, int a = 0) {
    callers.emplace_back(new Caller());
    Caller &c = *callers.back();
    Ask r;
    r.ticket = callers.size();
    r.kind = k;
    r.n = n;
    if (k == DENSE || k == BYTES || k == BITS) {
      c.out.resize(size_t(n) * O);
      r.out = c.out.data();
    }
    if (k == BYTES) {
      c.masks.assign(size_t(n) * O, 1);
      r.masks = c.masks.data();
    }
    if (k == BITS) {
      c.bits.resize(size_t(n) * WPR);
      r.bits = c.bits.data();
      r.most = param;
    }
    if (k == SET) {  // nodes 2, 5, 8, ...: what they are does not matter to the plan
      std::vector<int32_t> nodes;
      for (int j = 0; j < param; ++j) nodes.push_back(2 + 3 * j);
      r.set = std::make_shared<const std::vector<int32_t>>(nodes);
      c.probs.resize(size_t(n) * size_t(param));
      c.inactive.resize(size_t(n));
      r.probs = param ? c.probs.data() : nullptr;
      r.inactive = c.inactive.data();
    }
    if (k == TOPK) {
      c.topk_nodes.resize(size_t(n) * size_t(param));
      c.topk_probs.resize(size_t(n) * size_t(param));
      r.k = param, r.topk_nodes = c.topk_nodes.data(), r.topk_probs = c.topk_probs.data();
    }
    if (k == POOL) {
      c.pooled.resize(size_t(n) * size_t(kClasses[param]));
      r.pool = handle(param), r.classes = kClasses[param], r.pooled = c.pooled.data();
    }
    if (spec) {
      r.is_raw = true;
      r.raw = &c.raw;
      r.spec = spec;
      r.raw_n = raw_n ? raw_n : n;
      r.raw_a = a;
    } else {
      r.x = &c.x;
    }
    q.push_back(to_request(r));
    asked[r.ticket] = r;
    return r.ticket;
  }
};

int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }

// Every rule a single batch must keep, and for raw batches: every row of every piece reads, through its segment and the
// staged frames, exactly the frames of ITS utterance that the splice asks for.
void check_batch(const BatchPlan &b, int max_frames, const std::map<uint64_t, Ask> &asked) {
  CHECK(b.rows > 0 && b.rows <= max_frames);
  CHECK(b.taken.size() == b.pieces.size());
  CHECK(b.raw_src.size() == (b.raw ? b.pieces.size() : 0) && b.segs.size() == b.raw_src.size());
  int row = 0, at = 0, most = 0, set_nodes = 0, nnz = 0, topk_k = 0;
  bool any_mask = false, bytes = false;
  for (size_t i = 0; i < b.pieces.size(); ++i) {
    const Piece &p = b.pieces[i];
    const Ask pv = view(p);
    const Request &part = b.taken[i];
    const Ask &whole = asked.at(p.ticket);
    const size_t taken = size_t(part.taken);
    CHECK(part.ticket == p.ticket && part.n == p.rows && p.rows > 0);
    CHECK(view(part).kind == whole.kind && view(part).is_raw == whole.is_raw);
    CHECK(p.row0 == row);  // the pieces tile [0, rows) without gap or overlap
    row += p.rows;
    CHECK(part.taken >= 0 && part.taken + p.rows <= whole.n);
    CHECK(pv.out == (whole.out ? whole.out + taken * O : nullptr));
    CHECK(pv.bits == (whole.bits ? whole.bits + taken * WPR : nullptr));
    CHECK(p.last == (part.taken + p.rows == whole.n) && p.state == 0);
    CHECK((whole.kind == BITS) == (int(b.kind) == BITS));  // bit masks never share a batch with another kind
    CHECK((whole.kind == SET) == (int(b.kind) == SET) && (whole.kind == TOPK) == (int(b.kind) == TOPK));  // nor sets, nor top-k
    CHECK((whole.kind == POOL) == (int(b.kind) == POOL) && whole.pool == b.pool);  // nor pool, nor two handles
    CHECK(whole.is_raw == b.raw && whole.spec == b.spec);  // nor raw with spliced rows, nor two spec objects
    // the caller's destinations of these rows: advanced by the rows that earlier batches took, in the form's own unit
    const size_t len = whole.set ? whole.set->size() : 0;
    CHECK(pv.set == whole.set && pv.inactive == (whole.inactive ? whole.inactive + taken : nullptr));
    CHECK(pv.probs == (whole.probs ? whole.probs + taken * len : nullptr));
    CHECK(pv.k == whole.k && pv.topk_nodes == (whole.k ? whole.topk_nodes + taken * size_t(whole.k) : nullptr));
    CHECK(pv.topk_probs == (whole.k ? whole.topk_probs + taken * size_t(whole.k) : nullptr));
    CHECK(pv.pooled == (whole.pool ? whole.pooled + taken * size_t(whole.classes) : nullptr));
    if (whole.kind == SET) {  // set_off tiles [0, set_nodes) and block_off tiles [0, nnz), in piece order
      CHECK(p.set_off == set_nodes && p.block_off == nnz);
      set_nodes += int(len);
      nnz += p.rows * int(len);
    }
    if (whole.kind == POOL) CHECK(b.pool_classes == whole.classes);
    topk_k = std::max(topk_k, whole.k);
    any_mask |= whole.masks != nullptr;
    bytes |= whole.kind == BYTES;
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
  CHECK(set_nodes == b.set_nodes && nnz == b.nnz && topk_k == b.topk_k);  // the batch selects with its largest k
  if (int(b.kind) == DENSE || int(b.kind) == BYTES) CHECK(int(b.kind) == (bytes ? BYTES : DENSE));
  CHECK(b.stride == (int(b.kind) == BITS && 4 * (size_t(b.most) + 1) <= 3 * O ? b.most + 1 : 0));
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
    CHECK(bs.size() == 2 && int(bs[0].kind) == DENSE && !bs[0].any_mask && !bs[0].raw && bs[0].stride == 0);
    expect_pieces(bs[0], {{0, 40, 1}, {40, 40, 1}, {80, 20, 0}});
    expect_pieces(bs[1], {{0, 20, 1}});
    CHECK(view(bs[0].pieces[2]).out == Q.asked[3].out && view(bs[1].pieces[0]).out == Q.asked[3].out + 20 * O);  // taken * O
    CHECK(bs[1].taken[0].taken == 20 && bs[1].rows == 20);
  }
  {  // dense, bytes, dense: one byte-mask batch
    Queue Q;
    Q.add(DENSE, 10), Q.add(BYTES, 10), Q.add(DENSE, 10);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 1 && int(bs[0].kind) == BYTES && bs[0].any_mask && bs[0].pieces.size() == 3);
  }
  {  // bits behind dense: a new batch starts (and dense behind bits)
    Queue Q;
    Q.add(DENSE, 10), Q.add(BITS, 10, 5), Q.add(DENSE, 10);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 3 && int(bs[0].kind) == DENSE && int(bs[1].kind) == BITS && int(bs[2].kind) == DENSE);
    CHECK(bs[1].stride == 6 && bs[0].stride == 0);
  }
  {  // two bits requests: one batch, the larger `most`, bits offsets in words
    Queue Q;
    Q.add(BITS, 50, 10), Q.add(BITS, 80, 30);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 2 && int(bs[0].kind) == BITS && bs[0].most == 30 && bs[0].stride == 31 && !bs[0].any_mask);
    expect_pieces(bs[0], {{0, 50, 1}, {50, 50, 0}});
    CHECK(view(bs[0].pieces[1]).bits == Q.asked[2].bits && view(bs[1].pieces[0]).bits == Q.asked[2].bits + 50 * 2);
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
    Q.add(DENSE, 30, 0, kaldi);
    const auto bs = drain(Q, 16);
    CHECK(bs.size() == 2 && bs[0].raw && bs[0].spec == kaldi);
    expect_pieces(bs[0], {{0, 16, 0}});
    expect_pieces(bs[1], {{0, 14, 1}});
    CHECK(bs[0].raw_src[0].first == 0 && bs[0].raw_src[0].count == 21 && bs[0].raw_frames == 21);  // frames 0 .. 20
    CHECK(bs[1].raw_src[0].first == 11 && bs[1].raw_src[0].count == 19);                           // frames 11 .. 29
  }
  {  // two utterances share a batch (neither reads the other's frames), one of them rows [8, 20) of 30 frames, with bits
    Queue Q;
    Q.add(BITS, 10, 7, kaldi), Q.add(BITS, 12, 9, kaldi, 30, 8);
    const auto bs = drain(Q, 64);
    CHECK(bs.size() == 1 && int(bs[0].kind) == BITS && bs[0].pieces.size() == 2 && bs[0].stride == 10);
    CHECK(bs[0].raw_src[1].first == 3 && bs[0].raw_src[1].count == 22 && bs[0].raw_src[1].at == 10);
  }
  for (const SpliceRef &sp : {make_spec(-10, 0), make_spec(0, 0), make_spec(2, 5)}) {  // one-sided halos, split three ways
    Queue Q;
    Q.add(DENSE, 20, 0, sp), Q.add(DENSE, 1, 0, sp), Q.add(DENSE, 5, 0, sp, 40, 35);
    drain(Q, 7);
  }
  {  // distinct spec objects (of equal content) do not share a batch; nor do raw and spliced rows, either way round
    Queue Q;
    Q.add(DENSE, 5, 0, kaldi), Q.add(DENSE, 5, 0, make_spec(-5, 5)), Q.add(DENSE, 5), Q.add(DENSE, 5, 0, kaldi);
    const auto bs = drain(Q, 100);
    CHECK(bs.size() == 4 && bs[0].raw && bs[1].raw && !bs[2].raw && bs[3].raw && bs[0].spec != bs[1].spec);
  }
}

// The set, top-k and pool forms: a split request continues at taken * len / k / C of the caller's arrays, a batch's set
// pieces tile its nodes and its probs, its k is the largest of its pieces', and its pool handle is the one of all of them
// (check_batch states each of these for every piece; here the numbers of one small queue per form).
void set_topk_pool_batches() {
  {  // sets of 5, 0 and 1 nodes at max_frames = 16: 10 + 6 | 4 + 7 + 3
    Queue Q;
    Q.add(SET, 10, 5), Q.add(SET, 10, 0), Q.add(SET, 7, 1), Q.add(SET, 3, 5);
    const auto bs = drain(Q, 16);
    CHECK(bs.size() == 2 && int(bs[0].kind) == SET && bs[0].stride == 0 && !bs[0].any_mask);
    expect_pieces(bs[0], {{0, 10, 1}, {10, 6, 0}});
    expect_pieces(bs[1], {{0, 4, 1}, {4, 7, 1}, {11, 3, 1}});
    CHECK(bs[0].set_nodes == 5 && bs[0].nnz == 50 && bs[1].set_nodes == 6 && bs[1].nnz == 7 + 15);
    CHECK(bs[0].pieces[1].set_off == 5 && bs[0].pieces[1].block_off == 50);
    CHECK(bs[1].pieces[1].set_off == 0 && bs[1].pieces[1].block_off == 0 && bs[1].pieces[2].set_off == 1 && bs[1].pieces[2].block_off == 7);
    CHECK(view(bs[1].pieces[0]).inactive == Q.asked[2].inactive + 6 && view(bs[1].pieces[0]).probs == nullptr);  // (len 0: no probs at all)
  }
  {  // a 25-row set request at max_frames = 10: probs at taken * len
    Queue Q;
    Q.add(SET, 25, 5);
    const auto bs = drain(Q, 10);
    CHECK(bs.size() == 3 && view(bs[2].pieces[0]).probs == Q.asked[1].probs + 20 * 5 && view(bs[2].pieces[0]).inactive == Q.asked[1].inactive + 20);
    CHECK(bs[2].nnz == 25 && bs[2].set_nodes == 5);
  }
  {  // top-k with k = 3, 7, 1 at max_frames = 10: the batch's k is the largest of ITS pieces
    Queue Q;
    Q.add(TOPK, 12, 3), Q.add(TOPK, 4, 7), Q.add(TOPK, 6, 1);
    const auto bs = drain(Q, 10);
    CHECK(bs.size() == 3 && int(bs[0].kind) == TOPK && bs[0].topk_k == 3 && bs[1].topk_k == 7 && bs[2].topk_k == 1);
    expect_pieces(bs[1], {{0, 2, 1}, {2, 4, 1}, {6, 4, 0}});
    CHECK(view(bs[1].pieces[0]).topk_nodes == Q.asked[1].topk_nodes + 10 * 3 && view(bs[1].pieces[0]).topk_probs == Q.asked[1].topk_probs + 10 * 3);
    CHECK(view(bs[2].pieces[0]).topk_nodes == Q.asked[3].topk_nodes + 4 && view(bs[2].pieces[0]).k == 1);
  }
  {  // pool: one handle per batch, a split request at taken * C
    Queue Q;
    Q.add(POOL, 12, 0), Q.add(POOL, 4, 0), Q.add(POOL, 4, 1);
    const auto bs = drain(Q, 10);
    CHECK(bs.size() == 3 && int(bs[0].kind) == POOL && bs[0].pool == handle(0) && bs[1].pool == handle(0) && bs[2].pool == handle(1));
    CHECK(bs[1].pool_classes == 3 && bs[2].pool_classes == 5 && bs[1].pieces.size() == 2);
    CHECK(view(bs[1].pieces[0]).pooled == Q.asked[1].pooled + 10 * 3 && view(bs[1].pieces[1]).pooled == Q.asked[2].pooled);
  }
}

// For every ordered pair of kinds, A queued before B with the same raw-ness: they make one batch exactly where the join rule
// says they share -- dense and byte masks with one another, every other kind with its own only -- and two otherwise.
void join_table() {
  const SpliceRef kaldi = make_spec(-5, 5);
  const int param[kKinds] = {0, 0, 9, 5, 3, 0};  // most, len, k, handle
  for (int raw = 0; raw < 2; ++raw)
    for (int a = 0; a < kKinds; ++a)
      for (int b = 0; b < kKinds; ++b) {
        Queue Q;
        Q.add(Kind(a), 4, param[a], raw ? kaldi : nullptr), Q.add(Kind(b), 4, param[b], raw ? kaldi : nullptr);
        const bool share = a == b || (a <= BYTES && b <= BYTES);
        const auto bs = drain(Q, 100);
        CHECK(bs.size() == (share ? 1u : 2u));
        if (share) CHECK(int(bs[0].kind) == std::max(a, b));  // dense + bytes: a byte-mask batch, whichever came first
      }
  for (int k = 0; k < kKinds; ++k) {
    {  // a raw request and a spliced one of the same kind, either way round
      Queue Q;
      Q.add(Kind(k), 4, param[k], kaldi), Q.add(Kind(k), 4, param[k]), Q.add(Kind(k), 4, param[k], kaldi);
      CHECK(drain(Q, 100).size() == 3);
    }
    {  // equal content, distinct spec objects
      Queue Q;
      Q.add(Kind(k), 4, param[k], kaldi), Q.add(Kind(k), 4, param[k], make_spec(-5, 5));
      CHECK(drain(Q, 100).size() == 2);
    }
  }
  {  // two pool requests with distinct handles, and the first handle again behind them
    Queue Q;
    Q.add(POOL, 4, 0), Q.add(POOL, 4, 1), Q.add(POOL, 4, 0);
    CHECK(drain(Q, 100).size() == 3);
  }
}

void random_queues() {
  const SpliceRef specs[2] = {make_spec(-5, 5), make_spec(-1, 3)};
  const int sizes[3] = {1, 7, 64}, lens[3] = {0, 1, 5}, ks[3] = {1, 3, 7};
  for (unsigned seed = 0; seed < 300; ++seed) {
    std::mt19937 rng(seed);
    const int max_frames = sizes[rng() % 3];
    Queue Q;
    const int count = 1 + int(rng() % 10);
    for (int i = 0; i < count; ++i) {
      const Kind k = Kind(rng() % kKinds);
      const bool raw = rng() % 2;
      const int n = 1 + int(rng() % unsigned(3 * max_frames));
      const int before = int(rng() % 4) * int(rng() % 7), after = int(rng() % 4) * int(rng() % 7);  // often 0: whole utterances
      const int pick = int(rng() % 3);
      const int param = k == BITS ? int(rng() % (O + 1)) : k == SET ? lens[pick] : k == TOPK ? ks[pick] : k == POOL ? pick % 2 : 0;
      Q.add(k, n, param, raw ? specs[rng() % 2] : nullptr, before + n + after, before);
    }
    drain(Q, max_frames);
    CHECK(Q.q.empty());
  }
}

// ---- the form of a batch and its scatter (the cases above state plan outcomes; these state what every later step of the
// loop reads off the plan, and where a piece's data sits in the slot's landing buffer)

// word (row, col) of a landing buffer, as the device would have written it: any value that names its place
uint32_t word(size_t row, size_t col) { return uint32_t(row) * 1000u + uint32_t(col) + 1u; }
template <class T>
uint32_t as_word(T v) {
  uint32_t w;
  static_assert(sizeof v == sizeof w, "");
  std::memcpy(&w, &v, sizeof w);
  return w;
}
void never_expands(float *, const float *, int, size_t, size_t, const uint64_t *) { CHECK(!"a batch that is not compacted was expanded"); }

template <class T>
void check_guards(const std::vector<std::unique_ptr<Caller>> &cs, Block<T> Caller::*blk) {
  for (const auto &c : cs) CHECK(((*c).*blk).guards_whole());
}

// A batch of a split request's first part is followed by one that holds its rest and a whole request: the landing buffer of
// the second holds (row, column) words, every piece is scattered, and every caller block must hold exactly its rows' words.
void scatter_forms() {
  {  // whole rows of a coalesced batch: rows * O words of d_out
    Queue Q;
    Q.add(DENSE, 14), Q.add(BYTES, 5);
    auto bs = drain(Q, 10);  // 10 | 4 + 5
    const BatchPlan &b = bs[1];
    CHECK(bs[0].form.leave == Form::by_caller_copies && bs[0].form.words == 0 && bs[0].form.behind == Form::nothing);  // one caller
    CHECK(bs[0].form.upload == Form::no_upload && bs[0].form.upload_bytes == 0);
    CHECK(b.form.leave == Form::whole_rows && b.form.words == 9 * O && b.form.behind == Form::nothing && b.form.pass == Form::loop_rows);
    CHECK(b.form.upload == Form::byte_masks && b.form.upload_bytes == 9 * O);
    CHECK(b.pieces[0].want.kind == Want::rows && b.pieces[1].want.kind == Want::rows_behind_bytes);  // (a piece keeps its own kind)
    std::vector<uint32_t> land(b.form.words);
    for (size_t r = 0; r < 9; ++r)
      for (size_t j = 0; j < O; ++j) land[r * O + j] = word(r, j);
    for (const Piece &p : b.pieces) scatter(b, p, land.data(), O, never_expands);
    for (size_t r = 0; r < 4; ++r)
      for (size_t j = 0; j < O; ++j) CHECK(as_word(Q.callers[0]->out.data()[(10 + r) * O + j]) == word(r, j));
    for (size_t r = 0; r < 5; ++r)
      for (size_t j = 0; j < O; ++j) CHECK(as_word(Q.callers[1]->out.data()[r * O + j]) == word(4 + r, j));
    CHECK(as_word(Q.callers[0]->out.data()[10 * O - 1]) == as_word(Block<float>::guard()));  // rows of the earlier batch: not this one's
    check_guards(Q.callers, &Caller::out);
  }
  {  // a batch too large for one pinned landing buffer (1 GB) leaves by per-caller copies, as a single caller's does
    Queue Q;
    Q.add(DENSE, 2), Q.add(DENSE, 2);
    const BatchPlan b = plan_batch(Q.q, (1 << 30) / int(4 * O) + 1, O);
    CHECK(b.pieces.size() == 2 && b.form.leave == Form::by_caller_copies && b.form.words == 0);
  }
  {  // sets of 5 and 0 nodes: nnz + rows words of d_out, the blocks first, then one inactive value per row
    Queue Q;
    Q.add(SET, 14, 5), Q.add(SET, 5, 0), Q.add(SET, 1, 5);
    auto bs = drain(Q, 10);  // 10 | 4 + 5 + 1
    const BatchPlan &b = bs[1];
    CHECK(b.form.leave == Form::set_blocks && b.form.words == size_t(b.nnz + b.rows) && b.nnz == 25 && b.form.behind == Form::nothing);
    CHECK(b.form.pass == Form::loop_sets && b.form.upload == Form::node_sets && b.form.upload_bytes == 4 * 10);
    std::vector<uint32_t> land(b.form.words);
    for (size_t i = 0; i < land.size(); ++i) land[i] = word(0, i);
    for (const Piece &p : b.pieces) scatter(b, p, land.data(), O, never_expands);
    for (size_t i = 0; i < 20; ++i) CHECK(as_word(Q.callers[0]->probs.data()[50 + i]) == word(0, i));  // block 0: rows 10 .. 13
    for (size_t i = 0; i < 5; ++i) CHECK(as_word(Q.callers[2]->probs.data()[i]) == word(0, 20 + i));
    for (size_t r = 0; r < 4; ++r) CHECK(as_word(Q.callers[0]->inactive.data()[10 + r]) == word(0, 25 + r));
    for (size_t r = 0; r < 5; ++r) CHECK(as_word(Q.callers[1]->inactive.data()[r]) == word(0, 29 + r));
    CHECK(as_word(Q.callers[2]->inactive.data()[0]) == word(0, 34));
    CHECK(as_word(Q.callers[0]->probs.data()[49]) == as_word(Block<float>::guard()) && Q.callers[1]->probs.size() == 0);
    check_guards(Q.callers, &Caller::probs), check_guards(Q.callers, &Caller::inactive);
  }
  {  // top-k with k = 3 and 7: 2 * rows * 7 words, nodes [rows][7] then values [rows][7]; a piece keeps its first k columns
    Queue Q;
    Q.add(TOPK, 14, 3), Q.add(TOPK, 5, 7);
    auto bs = drain(Q, 10);  // 10 | 4 + 5
    const BatchPlan &b = bs[1];
    CHECK(b.topk_k == 7 && b.form.leave == Form::topk_pairs && b.form.words == 2 * 9 * 7 && b.form.behind == Form::select_topk);
    CHECK(b.form.pass == Form::loop_rows && b.form.upload == Form::no_upload && bs[0].form.words == 2 * 10 * 3);
    std::vector<uint32_t> land(b.form.words);
    for (size_t r = 0; r < 9; ++r)
      for (size_t j = 0; j < 7; ++j) land[r * 7 + j] = word(r, j), land[9 * 7 + r * 7 + j] = word(r, 100 + j);
    for (const Piece &p : b.pieces) scatter(b, p, land.data(), O, never_expands);
    for (size_t r = 0; r < 4; ++r)
      for (size_t j = 0; j < 3; ++j) {
        CHECK(as_word(Q.callers[0]->topk_nodes.data()[(10 + r) * 3 + j]) == word(r, j));
        CHECK(as_word(Q.callers[0]->topk_probs.data()[(10 + r) * 3 + j]) == word(r, 100 + j));
      }
    for (size_t r = 0; r < 5; ++r)
      for (size_t j = 0; j < 7; ++j) {
        CHECK(as_word(Q.callers[1]->topk_nodes.data()[r * 7 + j]) == word(4 + r, j));
        CHECK(as_word(Q.callers[1]->topk_probs.data()[r * 7 + j]) == word(4 + r, 100 + j));
      }
    CHECK(as_word(Q.callers[0]->topk_nodes.data()[29]) == as_word(Block<int32_t>::guard()));
    check_guards(Q.callers, &Caller::topk_nodes), check_guards(Q.callers, &Caller::topk_probs);
  }
  {  // pool, C = 5: rows * C words
    Queue Q;
    Q.add(POOL, 14, 1), Q.add(POOL, 5, 1);
    auto bs = drain(Q, 10);  // 10 | 4 + 5
    const BatchPlan &b = bs[1];
    CHECK(b.form.leave == Form::class_sums && b.form.words == 9 * 5 && b.form.behind == Form::pool_sums && b.form.upload == Form::no_upload);
    std::vector<uint32_t> land(b.form.words);
    for (size_t r = 0; r < 9; ++r)
      for (size_t j = 0; j < 5; ++j) land[r * 5 + j] = word(r, j);
    for (const Piece &p : b.pieces) scatter(b, p, land.data(), O, never_expands);
    for (size_t r = 0; r < 4; ++r)
      for (size_t j = 0; j < 5; ++j) CHECK(as_word(Q.callers[0]->pooled.data()[(10 + r) * 5 + j]) == word(r, j));
    for (size_t r = 0; r < 5; ++r)
      for (size_t j = 0; j < 5; ++j) CHECK(as_word(Q.callers[1]->pooled.data()[r * 5 + j]) == word(4 + r, j));
    CHECK(as_word(Q.callers[0]->pooled.data()[49]) == as_word(Block<float>::guard()));
    check_guards(Q.callers, &Caller::pooled);
  }
  {  // compacted rows: rows * stride words of d_comp; the expander is handed each piece's first row, the stride and its bits
    Queue Q;
    Q.add(BITS, 14, 9), Q.add(BITS, 5, 20);
    auto bs = drain(Q, 10);  // 10 | 4 + 5
    const BatchPlan &b = bs[1];
    CHECK(b.stride == 21 && b.form.leave == Form::compacted_rows && b.form.words == 9 * 21 && b.form.behind == Form::compact);
    CHECK(b.form.upload == Form::bit_words && b.form.upload_bytes == 9 * WPR * 8 && bs[0].stride == 10 && bs[0].form.words == 10 * 10);
    std::vector<float> land(b.form.words);
    int calls = 0;
    for (const Piece &p : b.pieces)
      scatter(b, p, land.data(), O, [&](float *out, const float *comp, int count, size_t width, size_t stride, const uint64_t *bits) {
        const Ask &whole = Q.asked.at(p.ticket);
        const size_t taken = calls == 0 ? 10 : 0;
        CHECK(out == whole.out + taken * O && bits == whole.bits + taken * WPR && count == p.rows && width == O && stride == 21);
        CHECK(comp == land.data() + size_t(p.row0) * 21);
        ++calls;
      });
    CHECK(calls == 2);
    // no room for the compacted pair, or no pinned landing buffer for whole rows: the rows leave by per-caller copies
    BatchPlan whole = b;
    leave_by_caller_copies(whole);
    CHECK(whole.stride == 0 && whole.form.leave == Form::by_caller_copies && whole.form.words == 0 && whole.form.behind == Form::nothing);
    CHECK(whole.form.upload == Form::bit_words && whole.form.upload_bytes == b.form.upload_bytes);
  }
  {  // a bit-mask batch not worth compacting leaves as whole rows do
    Queue Q;
    Q.add(BITS, 4, 60), Q.add(BITS, 5, 20);
    const auto bs = drain(Q, 10);
    CHECK(bs.size() == 1 && bs[0].stride == 0 && bs[0].form.leave == Form::whole_rows && bs[0].form.words == 9 * O);
  }
}

}  // namespace

int main() {
  kinds_and_strides();
  raw_batches();
  set_topk_pool_batches();
  join_table();
  random_queues();
  scatter_forms();
  std::puts("server plan ok");
  return 0;
}
