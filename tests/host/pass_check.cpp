// pass_check.cpp -- what a scoring pass hands each of its chunks (fdnn_pass.hpp), checked without a GPU: every named
// constructor over SYNTHETIC base addresses (only row_ptr, the set tables and the splice segments are read), chunk lists of
// one, two and three chunks, and the chunk arithmetic against the values fdnn_debug_frame_chunks_for gave before the
// arithmetic moved here.  Built with -fsanitize=address,undefined and run as a child process by tests/test_pass_host.py;
// exit status 0 = all cases hold.  D = 7, O = 70: two mask words per row, the second partial.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "fdnn_pass.hpp"

using namespace fdnn::pass;
namespace sets = fdnn::sets;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: [%s] CHECK(%s) failed\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace {

std::string g_case;
constexpr Dims kDims{7, 70, 2};
constexpr int N = 60, K = 5, LEN = 9;

// a base address per caller array, far apart: a pointer advanced by the wrong array's stride never meets another's range
template <class T>
T *base(int which) { return reinterpret_cast<T *>(uintptr_t(0x100000000ull) * uintptr_t(which)); }
const float *const X = base<const float>(1);
const int8_t *const BYTES = base<const int8_t>(2);
const uint64_t *const BITS = base<const uint64_t>(3);
float *const ROWS = base<float>(4);
int32_t *const TK_NODES = base<int32_t>(5);
float *const TK_PROBS = base<float>(6);
const int32_t *const NODES = base<const int32_t>(7);
float *const PROBS = base<float>(8);
float *const INACTIVE = base<float>(9);

// the tables that ARE read.  Lists: rows of 0..4 entries; the cuts at 20 and 37 fall where row_ptr is well inside the arrays.
std::vector<int32_t> make_row_ptr() {
  std::vector<int32_t> rp{0};
  for (int r = 0; r < N; ++r) rp.push_back(rp.back() + (r * 7 + 3) % 5);
  return rp;
}
const std::vector<int32_t> ROW_PTR = make_row_ptr();
// Sets: segments [0,10) len 3, [10,10) len 4 (no rows), [10,45) len 5 (both cuts fall inside it), [45,60) len 1
const std::vector<int32_t> SEG_ROWS{0, 10, 10, 45, 60}, SET_PTR{0, 3, 7, 12, 13};
const sets::Tables TABLES{SEG_ROWS.data(), SET_PTR.data(), 4};
const std::vector<fdnn::SpliceSeg> SEGS{fdnn::SpliceSeg{0, 0, 0, N - 1}};
const fdnn::SpliceSpec SPEC{};
constexpr int ROW0 = 11;
const Raw RAW{&SPEC, &SEGS, X, N + 4, ROW0};

const std::vector<Chunks> CUTS{{{0, N}}, {{0, 37}, {37, 23}}, {{0, 20}, {20, 17}, {37, 23}}};

int seg_of(int row) {
  for (int s = 0; s < TABLES.n_segs; ++s)
    if (row >= SEG_ROWS[size_t(s)] && row < SEG_ROWS[size_t(s) + 1]) return s;
  return -1;
}
size_t sets_probs_off(int row) {  // where row's block row starts in the caller's ragged probs
  size_t block = 0;
  const int s = seg_of(row);
  for (int t = 0; t < s; ++t) block += size_t(SEG_ROWS[size_t(t) + 1] - SEG_ROWS[size_t(t)]) * size_t(SET_PTR[size_t(t) + 1] - SET_PTR[size_t(t)]);
  return block + size_t(row - SEG_ROWS[size_t(s)]) * size_t(SET_PTR[size_t(s) + 1] - SET_PTR[size_t(s)]);
}
size_t sets_total() { return sets_probs_off(N - 1) + size_t(SET_PTR[4] - SET_PTR[3]); }

// One pass over every chunk list: each pointer chunk_view returns is its base plus the expected element offset, and the
// chunks' result ranges tile the caller's arrays -- each begins where the one before ended, the last ends at the array's end.
void check(const char *name, const Pass &p, Rows::Kind rows, Mask::Kind mask, Sink::Kind sink, bool callers) {
  CHECK(p.rows.kind == rows && p.mask.kind == mask && p.sink.kind == sink && on_callers_stream(p.sink.kind) == callers);
  const bool raw = rows == Rows::raw_device || rows == Rows::raw_host;
  const bool has_rows = sink == Sink::device_rows || sink == Sink::host_dense || sink == Sink::host_behind_bits;
  const bool topk = sink == Sink::host_topk || sink == Sink::device_topk;
  const bool sets_k = sink == Sink::host_sets || sink == Sink::device_sets;
  const bool entries = sink == Sink::host_lists || sink == Sink::host_set || sets_k;
  for (const Chunks &chunks : CUTS) {
    g_case = std::string(name) + ", " + std::to_string(chunks.size()) + " chunk(s)";
    size_t rows_at = 0, topk_at = 0, probs_at = 0, inactive_at = 0;  // elements of each result array handed out so far
    for (const auto &ch : chunks) {
      const int off = ch.first, cnt = ch.second;
      const size_t o = size_t(off);
      const ChunkView v = chunk_view(p, kDims, off, cnt);
      CHECK(v.cnt == cnt);
      // rows
      if (raw) CHECK(v.x == nullptr && v.splice_row == ROW0 + off && p.rows.raw.frames == X && p.rows.raw.n_frames == N + 4);
      else CHECK(v.x == X + o * 7 && v.splice_row == 0);
      // mask
      CHECK(v.bytes == (mask == Mask::device_bytes ? BYTES + o * 70 : nullptr));
      CHECK(v.bits == (mask == Mask::device_bits || mask == Mask::host_bits ? BITS + o * 2 : nullptr));
      // sink
      CHECK(v.rows == (has_rows ? ROWS + rows_at : nullptr) && (!has_rows || rows_at == o * 70));
      if (has_rows) rows_at += size_t(cnt) * 70;
      CHECK(v.topk_nodes == (topk ? TK_NODES + topk_at : nullptr) && v.topk_probs == (topk ? TK_PROBS + topk_at : nullptr) && (!topk || topk_at == o * K));
      if (topk) topk_at += size_t(cnt) * K;
      CHECK(v.inactive == (entries ? INACTIVE + inactive_at : nullptr) && (!entries || inactive_at == o));
      if (entries) inactive_at += size_t(cnt);
      if (!entries) CHECK(!v.probs && !v.nodes && v.n_nodes == 0 && v.row_ptr.empty() && v.segs.empty());
      if (entries) CHECK(v.probs == PROBS + probs_at);
      if (sink == Sink::host_lists) {
        const int32_t e0 = ROW_PTR[o];
        CHECK(probs_at == size_t(e0) && v.nodes == NODES + e0 && v.row_ptr.size() == size_t(cnt) + 1 && v.segs.empty());
        for (int i = 0; i <= cnt; ++i) CHECK(v.row_ptr[size_t(i)] == ROW_PTR[o + size_t(i)] - e0);
        CHECK(v.n_nodes == ROW_PTR[o + size_t(cnt)] - e0);
        probs_at += size_t(v.n_nodes);
      } else if (sink == Sink::host_set) {
        CHECK(probs_at == o * LEN && v.nodes == NODES && v.n_nodes == LEN && v.row_ptr.empty() && v.segs.empty());
        probs_at += size_t(cnt) * LEN;
      } else if (sets_k) {
        CHECK(probs_at == sets_probs_off(off) && v.nodes == NODES && v.n_nodes == SET_PTR[4] && v.row_ptr.empty());
        // every row of the chunk lies in exactly one segment of the slice, with its own segment's set, and its block row
        // -- reached through the slice's out_off from v.probs -- is the caller's
        size_t covered = 0, block = 0;
        for (const sets::Seg &sg : v.segs) {
          CHECK(sg.rows > 0 && size_t(sg.row0) == covered && size_t(sg.out_off) == block);
          for (int r = 0; r < sg.rows; ++r) {
            const int row = off + sg.row0 + r, s = seg_of(row);
            CHECK(s >= 0 && sg.set_off == SET_PTR[size_t(s)] && sg.len == SET_PTR[size_t(s) + 1] - SET_PTR[size_t(s)]);
            CHECK(v.probs + size_t(sg.out_off) + size_t(r) * size_t(sg.len) == PROBS + sets_probs_off(row));
          }
          covered += size_t(sg.rows), block += size_t(sg.rows) * size_t(sg.len);
        }
        CHECK(covered == size_t(cnt));
        probs_at += block;
      }
    }
    CHECK(rows_at == (has_rows ? size_t(N) * 70 : 0) && topk_at == (topk ? size_t(N) * K : 0) && inactive_at == (entries ? size_t(N) : 0));
    CHECK(probs_at == (sink == Sink::host_lists ? size_t(ROW_PTR[N]) : sink == Sink::host_set ? size_t(N) * LEN : sets_k ? sets_total() : 0));
  }
}

void every_constructor() {
  check("host_dense", Pass::host_dense("t", X, ROWS), Rows::host, Mask::none, Sink::host_dense, false);
  check("host_bits", Pass::host_bits("t", X, BITS, ROWS), Rows::host, Mask::host_bits, Sink::host_behind_bits, false);
  check("host_topk", Pass::host_topk("t", X, K, TK_NODES, TK_PROBS), Rows::host, Mask::none, Sink::host_topk, false);
  check("host_lists", Pass::host_lists("t", X, ROW_PTR.data(), NODES, PROBS, INACTIVE), Rows::host, Mask::none, Sink::host_lists, false);
  check("host_set", Pass::host_set("t", X, NODES, LEN, PROBS, INACTIVE), Rows::host, Mask::none, Sink::host_set, false);
  check("host_sets", Pass::host_sets("t", X, TABLES, NODES, PROBS, INACTIVE), Rows::host, Mask::none, Sink::host_sets, false);
  check("raw_dense", Pass::raw_dense("t", RAW, ROWS), Rows::raw_host, Mask::none, Sink::host_dense, false);
  check("raw_bits", Pass::raw_bits("t", RAW, BITS, ROWS), Rows::raw_host, Mask::host_bits, Sink::host_behind_bits, false);
  check("raw_topk", Pass::raw_topk("t", RAW, K, TK_NODES, TK_PROBS), Rows::raw_host, Mask::none, Sink::host_topk, false);
  check("device_dense", Pass::device_dense("t", X, ROWS), Rows::device, Mask::none, Sink::device_rows, true);
  check("device_bits", Pass::device_bits("t", X, BITS, ROWS), Rows::device, Mask::device_bits, Sink::device_rows, true);
  check("device_topk", Pass::device_topk("t", X, K, TK_NODES, TK_PROBS), Rows::device, Mask::none, Sink::device_topk, true);
  check("raw_device_dense", Pass::raw_device_dense("t", RAW, ROWS), Rows::raw_device, Mask::none, Sink::device_rows, true);
  check("loop_rows, dense", Pass::loop_rows(X, nullptr, nullptr, ROWS), Rows::device, Mask::none, Sink::device_rows, true);
  check("loop_rows, bytes", Pass::loop_rows(X, BYTES, nullptr, ROWS), Rows::device, Mask::device_bytes, Sink::device_rows, true);
  check("loop_rows, bits", Pass::loop_rows(X, nullptr, BITS, ROWS), Rows::device, Mask::device_bits, Sink::device_rows, true);
  check("loop_sets", Pass::loop_sets(X, TABLES, NODES, PROBS, INACTIVE), Rows::device, Mask::none, Sink::device_sets, true);
  // results that may be null because nothing lands there: empty lists, an empty set
  g_case = "null probs";
  const std::vector<int32_t> none(size_t(N) + 1, 0);
  CHECK(chunk_view(Pass::host_lists("t", X, none.data(), nullptr, nullptr, INACTIVE), kDims, 37, 23).probs == nullptr);
  CHECK(chunk_view(Pass::host_set("t", X, nullptr, 0, nullptr, INACTIVE), kDims, 37, 23).probs == nullptr);
}

// fdnn_debug_frame_chunks_for(n, chained) at the parent of the change that moved the arithmetic here, by the case each n
// exercises.  (Only a remainder ABOVE one round is ever split, so the n the change was asked to pin cut the same chained or
// not; the last four are the ones where the hidden layers' chaining decides.)
struct Recorded {
  int n;
  const char *exercises;
  Chunks chained, unchained;
};
const std::vector<Recorded> RECORDED{
    {1, "a single chunk", {{0, 1}}, {{0, 1}}},
    {2560, "a single chunk (the scoring loop's small-batch limit)", {{0, 2560}}, {{0, 2560}}},
    {10240, "10 240: one whole round", {{0, 10240}}, {{0, 10240}}},
    {20480, "20 480: one whole chunk", {{0, 20480}}, {{0, 20480}}},
    {20481, "20 481: the first n cut in two", {{0, 20480}, {20480, 1}}, {{0, 20480}, {20480, 1}}},
    {21000, "21 000: a short tail chunk", {{0, 20480}, {20480, 520}}, {{0, 20480}, {20480, 520}}},
    {22528, "a cut inside the tail split (20 480 + 2 048)", {{0, 20480}, {20480, 2048}}, {{0, 20480}, {20480, 2048}}},
    {22529, "a tail past the split", {{0, 20480}, {20480, 2049}}, {{0, 20480}, {20480, 2049}}},
    {33000, "a remainder above one round, its tail past the split", {{0, 20480}, {20480, 12520}}, {{0, 20480}, {20480, 12520}}},
    {125000, "several whole chunks",
     {{0, 20480}, {20480, 20480}, {40960, 20480}, {61440, 20480}, {81920, 20480}, {102400, 20480}, {122880, 2120}},
     {{0, 20480}, {20480, 20480}, {40960, 20480}, {61440, 20480}, {81920, 20480}, {102400, 20480}, {122880, 2120}}},
    {11000, "one batch whose tail is split off when unchained", {{0, 11000}}, {{0, 10240}, {10240, 760}}},
    {12288, "the largest tail that is split off", {{0, 12288}}, {{0, 10240}, {10240, 2048}}},
    {12289, "the first tail past the split", {{0, 12289}}, {{0, 12289}}},
    {32768, "a whole chunk, then a remainder with a split tail", {{0, 20480}, {20480, 12288}}, {{0, 20480}, {20480, 10240}, {30720, 2048}}},
};

void chunk_arithmetic() {
  CHECK(chunk_size(false, 0) == kChunkFrames && chunk_size(true, 0) == 0 && chunk_size(true, -1) == 0);
  CHECK(chunk_size(true, 4096) == kRoundFrames && chunk_size(true, 25000) == 2 * kRoundFrames && chunk_size(true, 30720) == 3 * kRoundFrames);
  for (const Recorded &r : RECORDED) {
    g_case = std::string("frame_chunks ") + std::to_string(r.n) + ": " + r.exercises;
    CHECK(frame_chunks(r.n, kChunkFrames, [](int) { return true; }) == r.chained);
    CHECK(frame_chunks(r.n, kChunkFrames, [](int) { return false; }) == r.unchained);
    int asked = -1;  // the predicate is asked about the remainder, the batch that would be split
    frame_chunks(r.n, kChunkFrames, [&](int cnt) { asked = cnt; return true; });
    CHECK(asked < 0 || asked == r.chained.back().second);
  }
  g_case = "never chunk";
  CHECK((frame_chunks(125000, 0, [](int) { return true; }) == Chunks{{0, 125000}}));
  CHECK((frame_chunks(43008, 0, [](int) { return false; }) == Chunks{{0, 40960}, {40960, 2048}}));
  g_case = "stride_chunks";
  CHECK((stride_chunks(1) == Chunks{{0, 1}}) && (stride_chunks(20480) == Chunks{{0, 20480}}) && (stride_chunks(20481) == Chunks{{0, 20480}, {20480, 1}}));
  CHECK((stride_chunks(22528) == Chunks{{0, 20480}, {20480, 2048}}) && (stride_chunks(45000) == Chunks{{0, 20480}, {20480, 20480}, {40960, 4040}}));
  // a production-sized cut through the view: the second chunk of 20 481 rows of the usual net's widths
  g_case = "20 481 rows";
  const Dims big{432, 8000, 125};
  const ChunkView v = chunk_view(Pass::device_bits("t", X, BITS, ROWS), big, 20480, 1);
  CHECK(v.x == X + size_t(20480) * 432 && v.bits == BITS + size_t(20480) * 125 && v.rows == ROWS + size_t(20480) * 8000);
}

}  // namespace

int main() {
  every_constructor();
  chunk_arithmetic();
  std::puts("pass ok");
  return 0;
}
