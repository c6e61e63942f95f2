// fdnn_set.hip -- lazy output for a SHARED NODE SET: one active list for a whole row range, scored on the int8 MFMA.
//
//   LazyOutputActivations (dnn.cc:355-392): the listed nodes' logits, every other node's logit 0
//   SoftMax::apply (dnn.cc:534-544): e = exp(z), total, p = e / total; every unlisted node reads 1 / total
//
// The list path (fdnn_lists.hip) treats count rows x len nodes as count x len independent dot products: every entry reads
// its 2 KB weight row again.  With ONE set for all rows the same work is an n x K x len GEMM whose len weight rows are read
// once per frame group.  This kernel is fdnn_small.hip's output instance with four differences:
//
//   * the 64 weight rows of a node tile are GATHERED: a lane's row offset is nodes[m0 + row] * ldw inside one descriptor
//     over the whole layer; a slot past len and a node outside [0, O) get the offset that reads zeros (fdnn_set.hpp: the
//     node is never used as an address before that guard);
//   * the activation descriptor of a frame tile ends at the call's last row: rows past it read zeros, nothing is stored
//     for them.  Every row-dependent part of an offset is in the per-lane offset, the scalar offset is the wave's K slice;
//   * saturating pairs come from the per-node index (fdnn_lists.hpp) and are applied where the partial tiles meet, from
//     the row's activation bytes in memory: sat16(p) - p is additive on an order-free integer sum;
//   * the epilogue stores e = exp(z) of (row r, entry j) at probs[r * len + j] -- NaN for a node outside the layer -- and
//     no partial sums: the total and the scale are the list path's finish kernel with a uniform row stride, so the order of
//     the row sum is the normative one and the bytes are those of fdnn_ctx_lazy_output_lists on the same (row, set).
//
// Each of the 8 waves owns a 256-byte slice of K, requests its slice of W and of the first activation tile by LDS-DMA up
// front, keeps W in registers (64 VGPRs of MFMA fragments) and streams activation tiles through a double buffer; the eight
// partial 64 x 32 int32 tiles meet in LDS.  The tile itself is fdnn_set_tile.hpp's set_tile, shared with fdnn_sets.hip (one set per
// segment of the row range): this kernel runs it on the whole call.  So is its launch: that header's launch_set_tile (the
// dynamic LDS limit, once per device) on the <FIX, FAST> instance fdnn_launch.hpp's with_fix_fast picks.
#include <algorithm>
#include <atomic>

#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_set_tile.hpp"

namespace fdnn {
namespace {

LaunchCounts<3> g_set_launches;                     // MFMA kernel without / with the pair walk, calls served by the list kernels
std::atomic<int> g_set_mode{0};                     // fdnn_debug_set_kernel

// FIX: the layer has saturating pairs (the walk over a node's own list); FAST: validated 3-operation division
template <bool FIX, bool FAST>
__global__ __launch_bounds__(kStThreads, 2) void set_score_kernel(SetParams p) {
  const set::Tile tile = set::block_tile(p.plan, blockIdx.x);
  set_tile<FIX, FAST>(p, SetView{p.a, p.count, p.lda, p.nodes, p.len, p.probs, p.acc, tile.m0, tile.t_begin, tile.t_end});
}

// The fallback's lists: row r of the call is entries [r * len, (r + 1) * len), each row the set itself.
__global__ __launch_bounds__(256) void set_expand_kernel(const int32_t *nodes, int len, int count, int32_t *row_ptr, int32_t *rep) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < static_cast<long long>(count) * len) rep[i] = nodes[i % len];
  if (i <= count) row_ptr[i] = static_cast<int32_t>(i * len);
}

}  // namespace

void launch_set_score(const SetParams &p, hipStream_t s) {
  if (p.plan.blocks <= 0) return;
  const bool fix = p.fix_off != nullptr && p.fix_pairs != nullptr;
  g_set_launches.bump(fix ? 1 : 0);
  with_fix_fast(fix, p.fastdiv, [&](auto FIX, auto FAST) { launch_set_tile<set_score_kernel<FIX(), FAST()>>(p.plan.blocks, s, p); });
}

void launch_set_expand(const int32_t *nodes, int len, int count, int32_t *row_ptr, int32_t *rep, hipStream_t s) {
  const long long items = std::max<long long>(static_cast<long long>(count) * len, static_cast<long long>(count) + 1);
  g_set_launches.bump(2);
  hipLaunchKernelGGL(set_expand_kernel, dim3(static_cast<unsigned>((items + 255) / 256)), dim3(256), 0, s, nodes, len, count, row_ptr, rep);
}

void set_launch_counts(unsigned long long out[3]) { g_set_launches.read(out); }

int set_kernel_mode() { return g_set_mode.load(std::memory_order_relaxed); }
void set_kernel_mode(int mode) { g_set_mode.store(mode, std::memory_order_relaxed); }

}  // namespace fdnn
