// fdnn_sets.hip -- lazy output for PER-SEGMENT NODE SETS: several row ranges of one context, each with its own active list,
// scored on the int8 MFMA in ONE launch.
//
//   LazyOutputActivations (dnn.cc:355-392): the listed nodes' logits, every other node's logit 0
//   SoftMax::apply (dnn.cc:534-544): e = exp(z), total, p = e / total; every unlisted node reads 1 / total
//
// fdnn_set.hip scores one set over a row range in two launches of 11 - 13 us: more than the work of a 100-frame utterance
// with 80 nodes.  Callers that serve many utterances, each with its own set (forced alignment, keyword spotting, n-best
// rescoring), would pay that per utterance.  Here a workgroup runs fdnn_set_tile.hpp's tile -- the very code of
// set_score_kernel, launched by the same launch_set_tile -- on the segment that sets::block_tile names for it:
//
//   * the segment table (sets::Launch, up to 64 segments) is a kernel argument; the segment of a workgroup is found by a
//     binary search over block_off on the scalar unit, and what the segment contributes to addresses (its first row, where
//     its set and its block begin) is scalar too;
//   * the tile's view begins at the segment's first row and has the segment's row count: the activation descriptor of a
//     frame tile ends at the SEGMENT's last row, so the rows of the next segment that fall into a tile's 32 read zeros and
//     nothing is stored for them -- a neighbour's rows are never scored with this segment's set;
//   * the node gather reads the segment's own set under set::row_offset's guard; e of (row r, entry j) of the segment goes to
//     probs[out_off + r * len + j].
//
// The total and the scale are the list path's finish kernel over the row pointer the call synthesizes (sets::row_ptr): the
// bytes of a row are those of fdnn_ctx_lazy_output_set on its segment alone and of fdnn_ctx_lazy_output_lists with the sets
// repeated per row.  Where the tile's shape does not apply, sets_expand_kernel writes those lists and the list kernels score.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_set_tile.hpp"

namespace fdnn {
namespace {

LaunchCounts<3> g_sets_launches;  // MFMA kernel without / with the pair walk, calls served by the list kernels

// p: the layer, and a / nodes / probs / acc of the call's first row, whole node array and first block (count, len and plan
// are not read); l: this launch's segments
template <bool FIX, bool FAST>
__global__ __launch_bounds__(kStThreads, 2) void sets_score_kernel(SetParams p, sets::Launch l) {
  const sets::Tile tile = sets::block_tile(l, blockIdx.x);
  const int s = __builtin_amdgcn_readfirstlane(tile.seg);
  const int row0 = l.row0[s], len = l.len[s], out_off = l.out_off[s];
  set_tile<FIX, FAST>(p, SetView{p.a + static_cast<size_t>(row0) * p.lda, l.rows[s], p.lda, p.nodes + l.set_off[s], len, p.probs + out_off,
                                 p.acc != nullptr ? p.acc + out_off : nullptr, __builtin_amdgcn_readfirstlane(tile.m0),
                                 __builtin_amdgcn_readfirstlane(tile.t_begin), __builtin_amdgcn_readfirstlane(tile.t_end)});
}

// The list contract's row pointer of the ragged blocks (sets::row_ptr is its host statement), for the finish pass, and for
// the fallback where each row's set begins (sets::row_set): workgroup s writes segment s's rows, the last launch's
// workgroup 0 the end.  Written on the device from the launch table, so that an enqueued call reads no host memory after
// it has returned.
__global__ __launch_bounds__(256) void sets_rows_kernel(sets::Launch l, int32_t *row_ptr, int32_t *row_set, int end_row, int end) {
  const int s = blockIdx.x;
  const int row0 = l.row0[s], rows = l.rows[s], len = l.len[s], out_off = l.out_off[s], set_off = l.set_off[s];
  for (int r = threadIdx.x; r < rows; r += 256) {
    row_ptr[row0 + r] = out_off + r * len;
    if (row_set != nullptr) row_set[row0 + r] = set_off;
  }
  if (s == 0 && threadIdx.x == 0 && end_row >= 0) row_ptr[end_row] = end;
}

// The fallback's lists: row r's list is its segment's set, entries [row_ptr[r], row_ptr[r + 1]) copied from nodes + row_set[r].
__global__ __launch_bounds__(256) void sets_expand_kernel(const int32_t *nodes, const int32_t *row_ptr, const int32_t *row_set, int32_t *rep) {
  const int r = blockIdx.x;
  const int b = row_ptr[r], len = row_ptr[r + 1] - b;
  const int32_t *set = nodes + row_set[r];
  for (int j = threadIdx.x; j < len; j += 256) rep[b + j] = set[j];
}

}  // namespace

void launch_sets_score(const SetParams &p, const sets::Launch &l, hipStream_t s) {
  if (sets::blocks(l) <= 0) return;
  const bool fix = p.fix_off != nullptr && p.fix_pairs != nullptr;
  g_sets_launches.bump(fix ? 1 : 0);
  with_fix_fast(fix, p.fastdiv, [&](auto FIX, auto FAST) { launch_set_tile<sets_score_kernel<FIX(), FAST()>>(sets::blocks(l), s, p, l); });
}

void launch_sets_rows(const sets::Launch &l, int32_t *row_ptr, int32_t *row_set, int end_row, int end, hipStream_t s) {
  if (l.n_segs <= 0) return;
  hipLaunchKernelGGL(sets_rows_kernel, dim3(l.n_segs), dim3(256), 0, s, l, row_ptr, row_set, end_row, end);
}

void launch_sets_expand(const int32_t *nodes, const int32_t *row_ptr, const int32_t *row_set, int count, int32_t *rep, hipStream_t s) {
  g_sets_launches.bump(2);
  if (count <= 0) return;
  hipLaunchKernelGGL(sets_expand_kernel, dim3(count), dim3(256), 0, s, nodes, row_ptr, row_set, rep);
}

void sets_launch_counts(unsigned long long out[3]) { g_sets_launches.read(out); }

}  // namespace fdnn
