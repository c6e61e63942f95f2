// fdnn_lists_union.hip -- lazy output by active-node LISTS scored over PER-FRAME-GROUP NODE UNIONS on the int8 MFMA.
//
//   LazyOutputActivations (dnn.cc:355-392): the listed nodes' logits, every other node's logit 0
//   SoftMax::apply (dnn.cc:534-544): e = exp(z), total, p = e / total; every unlisted node reads 1 / total
//
// The list kernels (fdnn_lists.hip) read a 2 KB weight row per entry: right for tens of nodes per frame, slower than the
// whole masked layer from a few per cent of the layer up.  The set kernels (fdnn_set.hip, fdnn_sets.hip) read a weight row
// once per frame group, but only where every row of a range has the same nodes.  A decoder's beam is neither: 1 - 20 % of the
// states, another set every frame, changing slowly.  So the UNION of 32 * g consecutive rows' lists is little longer than
// one row's list; here it is scored as a set for those rows, and only the entries the caller listed are handed back:
//
//   build   one workgroup per group of 32 * g rows (fdnn_lists_union.hpp: group_range).  The group's valid nodes are OR-ed
//           into an output_dim-bit set in LDS, a popcount prefix over the words ranks them, the union goes ascending to
//           u_nodes + (the group's first entry), its length to u_len, every entry's rank to pos -- an entry whose node is
//           outside [0, O) gets pos -1 and its NaN here, and is never used as an address or a bit index --, and the
//           group's (group, 64-node chunk) work items are appended to a work list through one atomic counter.
//   score   fdnn_set_tile.hpp's tile, the set kernels' own code, one workgroup per work item: the view is the group (its
//           rows, its union), the weights stay in registers over the group's g frame tiles.  The store is a GATHER: e of the
//           32 x 64 tile is parked in the LDS buffer the tile has just consumed, and after a barrier the workgroup walks
//           the frame tile's rows' entries and copies probs[i] = e[row][pos[i] - m0] for those whose rank falls into its
//           chunk.  Every entry is written exactly once, by the workgroup of its chunk, whatever order a device list has.
//           The work list holds at most nnz / 64 + groups items (fdnn_lists_union.hpp); the grid is that bound or four
//           workgroups per CU, whichever is less, and a workgroup walks the list with the grid's stride.  The launch is the
//           set kernels' launch_set_tile.
//   finish  the list path's own kernel over the caller's row_ptr (fdnn_lists.hip): the normative sum order.
//
// The accumulators are exact integers and the logit, the exp2 and the finish pass are the list path's instructions, so the
// bytes are those of the dot-product kernels on the same lists.
#include <algorithm>

#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_set_tile.hpp"

namespace fdnn {
namespace {

constexpr int kLuThreads = 512;
constexpr int kLuWaves = kLuThreads / 64;
constexpr int kLuOrderedBit = 16;  // of a work item's chunk word: every row of the group ascends (chunks < kMaxNodes / 64 = 2^10)
static_assert(lunion::kMaxNodes / set::kNodeTile <= 1 << kLuOrderedBit, "a chunk index stays below the flag");

LaunchCounts<4> g_union_launches;  // build, score without / with the pair walk, calls served by the list kernels

__global__ __launch_bounds__(kLuThreads) void lists_union_build_kernel(UnionParams u) {
  __shared__ uint32_t bits[lunion::kMaxWords];
  __shared__ int32_t rank[lunion::kMaxWords];
  __shared__ int32_t wtot[kLuWaves];
  __shared__ int32_t slot_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const lunion::Range r = lunion::group_range(u.row_ptr, u.count, u.nnz, u.group_tiles, q);
  const int words = (u.rows + lunion::kBitWord - 1) / lunion::kBitWord;  // <= kMaxWords: lunion::shape_applies
  for (int w = tid; w < words; w += kLuThreads) bits[w] = 0;
  __syncthreads();
  for (int i = r.b + tid; i < r.e; i += kLuThreads) {
    const int32_t node = u.nodes[i];
    if (set::node_ok(node, u.rows)) atomicOr(&bits[node >> 5], 1u << (node & 31));
  }
  __syncthreads();
  // ranks: thread t owns words [t * wpt, (t + 1) * wpt); an exclusive scan of the threads' popcounts
  const int wpt = (words + kLuThreads - 1) / kLuThreads;
  const int w0 = tid * wpt;
  int local = 0;
  for (int k = 0; k < wpt; ++k)
    if (w0 + k < words) local += __popc(bits[w0 + k]);
  int x = local;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) wtot[wave] = x;
  __syncthreads();
  int base = 0, total = 0;
  for (int w = 0; w < kLuWaves; ++w) {
    if (w < wave) base += wtot[w];
    total += wtot[w];
  }
  // the union, ascending: total <= r.e - r.b (distinct nodes among that many entries), so it ends inside the group's range
  int at = base + x - local;
  for (int k = 0; k < wpt; ++k) {
    if (w0 + k >= words) break;
    rank[w0 + k] = at;
    for (uint32_t b = bits[w0 + k]; b != 0; b &= b - 1) u.u_nodes[r.b + at++] = (w0 + k) * lunion::kBitWord + (__ffs(b) - 1);
  }
  __syncthreads();
  int unordered = 0;  // some row of the group does not ascend, or holds a node outside the layer: its ranks do not ascend either
  for (int i = r.b + tid; i < r.e; i += kLuThreads) {
    const int32_t node = u.nodes[i];
    if (set::node_ok(node, u.rows)) {
      u.pos[i] = rank[node >> 5] + __popc(bits[node >> 5] & ((1u << (node & 31)) - 1u));
    } else {  // a node outside the layer: NaN, and so is its row's total (as fdnn_lists.hip)
      u.pos[i] = -1;
      u.probs[i] = __builtin_nanf("");
      if (u.acc != nullptr) u.acc[i] = 0;
      unordered = 1;
    }
  }
  // 16 lanes per row, the row's range clamped as the gather and the finish kernel clamp it
  const int g_rows = min(u.count - q * lunion::group_rows(u.group_tiles), lunion::group_rows(u.group_tiles));
  for (int rr = tid >> 4; rr < g_rows; rr += kLuThreads / 16) {
    const int32_t *rp = u.row_ptr + q * lunion::group_rows(u.group_tiles) + rr;
    const int b = lunion::clamp_ptr(rp[0], u.nnz), e = max(b, lunion::clamp_ptr(rp[1], u.nnz));
    for (int i = b + 1 + (tid & 15); i < e; i += 16) unordered |= u.nodes[i] < u.nodes[i - 1];
  }
  const int ordered = __syncthreads_or(unordered) ? 0 : 1;
  const int chunks = (total + set::kNodeTile - 1) / set::kNodeTile;
  if (tid == 0) {
    u.u_len[q] = total;
    slot_s = chunks > 0 ? atomicAdd(u.counter, chunks) : 0;
  }
  __syncthreads();
  const int slot = slot_s;
  for (int c = tid; c < chunks; c += kLuThreads)
    if (slot + c < u.bound) {  // (always, for row pointers that do not decrease: lunion::grid_bound)
      u.work[2 * (slot + c)] = q;
      u.work[2 * (slot + c) + 1] = c | ordered << kLuOrderedBit;
    }
}

// The gather store of set_tile (fdnn_set_tile.hpp: DenseStore is the other one).  entry() parks e -- and the accumulator,
// for the parity tap -- in the 16 bytes its thread owns in wave regions 0 and 1 of the consumed buffer (the thread has read
// them, nobody else does); tile_done() waits for every thread's, then 16 lanes per row of the frame tile walk the row's
// entries.  row_ptr is the caller's at the view's first row, its values clamped as the finish kernel clamps them.  Where
// the build kernel found every row of the group ascending (`ordered`), a row's entries of one chunk are one run of it: the
// lanes search its start and stop behind its end; otherwise they look at every entry of the row.
struct GatherStore {
  const int32_t *row_ptr;
  const int32_t *pos;
  float *probs;
  int32_t *acc;
  int nnz, m0, ordered;
  __device__ __forceinline__ void entry(const SetView &, size_t, int f, int jl, int cur, float e, int a32) const {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *at = smem + cur * kStABuf + st_park(f, jl);
    *reinterpret_cast<float *>(at) = e;
    if (acc != nullptr) *reinterpret_cast<int32_t *>(at + kStFT * kStSlice) = a32;
  }
  __device__ __forceinline__ void tile_done(const SetView &v, int f0, int cur) const {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int f = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const int ff = f0 + f;
    if (ff >= v.count) return;
    const int b = lunion::clamp_ptr(row_ptr[ff], nnz);
    const int e = max(b, lunion::clamp_ptr(row_ptr[ff + 1], nnz));
    int lo = b;
    if (ordered) {
      // the ranks of an ascending row ascend: the row's first entry with pos >= m0 lies in [lo, hi]; its 16 lanes probe
      // lo, lo + step, .. and keep the interval between the last probe below m0 and the first one at or above it
      int hi = e;
      while (hi - lo > 16) {
        const int step = (hi - lo + 15) >> 4;
        const int at = lo + l16 * step;
        const bool ge = at >= hi || pos[at] >= m0;
        const unsigned mask = static_cast<unsigned>(__ballot(ge) >> (threadIdx.x & 48)) & 0xffffu;
        const int k = mask != 0 ? __ffs(mask) - 1 : 16;  // the first probe that is not below
        if (k < 16) hi = min(hi, lo + k * step);
        if (k > 0) lo += (k - 1) * step + 1;
      }
    }
    for (int i = lo + l16; i < e; i += 16) {
      const int jl = pos[i] - m0;
      if (ordered && jl >= set::kNodeTile) break;  // (this lane's later entries rank higher still)
      if (static_cast<unsigned>(jl) >= static_cast<unsigned>(set::kNodeTile)) continue;
      const char *at = smem + cur * kStABuf + st_park(f, jl);
      probs[i] = *reinterpret_cast<const float *>(at);
      if (acc != nullptr) acc[i] = *reinterpret_cast<const int32_t *>(at + kStFT * kStSlice);  // (fdnn_debug_ctx_lists_acc)
    }
  }
};
static_assert(kStThreads == 16 * kStFT, "16 lanes per row of a frame tile");

// FIX: the layer has saturating pairs (the walk over a node's own list); FAST: validated 3-operation division
template <bool FIX, bool FAST>
__global__ __launch_bounds__(kStThreads, 2) void lists_union_score_kernel(SetParams p, UnionParams u) {
  const int items = min(*u.counter, u.bound);
  // (a workgroup walks the work list with the grid's stride: the bound is many times the list's length where rows share nodes)
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int q = __builtin_amdgcn_readfirstlane(u.work[2 * item]);
    const int word = __builtin_amdgcn_readfirstlane(u.work[2 * item + 1]);
    const int m0 = (word & ((1 << kLuOrderedBit) - 1)) * set::kNodeTile;
    const int r0 = q * lunion::group_rows(u.group_tiles);
    const int rows = min(u.count - r0, lunion::group_rows(u.group_tiles));
    const int b = __builtin_amdgcn_readfirstlane(lunion::clamp_ptr(u.row_ptr[r0], u.nnz));
    const int len = __builtin_amdgcn_readfirstlane(u.u_len[q]);
    const GatherStore st{u.row_ptr + r0, u.pos, u.probs, u.acc, u.nnz, m0, word >> kLuOrderedBit & 1};
    set_tile<FIX, FAST, GatherStore>(p, SetView{p.a + static_cast<size_t>(r0) * p.lda, rows, p.lda, u.u_nodes + b, len, nullptr, nullptr, m0, 0,
                                                (rows + kStFT - 1) / kStFT},
                                     st);
  }
}

}  // namespace

hipError_t launch_lists_union_build(const UnionParams &u, int n_groups, hipStream_t s) {
  if (n_groups <= 0 || u.nnz <= 0) return hipSuccess;
  const hipError_t e = hipMemsetAsync(u.counter, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  g_union_launches.bump(0);
  hipLaunchKernelGGL(lists_union_build_kernel, dim3(n_groups), dim3(kLuThreads), 0, s, u);
  return hipSuccess;
}

void launch_lists_union_score(const SetParams &p, const UnionParams &u, int n_cu, hipStream_t s) {
  if (u.bound <= 0 || u.nnz <= 0) return;
  // one workgroup fills a CU (128 KiB of LDS); a few rounds of them even out the groups' last, shorter items
  const int blocks = std::min(u.bound, 4 * (n_cu > 0 ? n_cu : 256));
  const bool fix = p.fix_off != nullptr && p.fix_pairs != nullptr;
  g_union_launches.bump(fix ? 2 : 1);
  with_fix_fast(fix, p.fastdiv, [&](auto FIX, auto FAST) { launch_set_tile<lists_union_score_kernel<FIX(), FAST()>>(blocks, s, p, u); });
}

void lists_union_note_fallback() { g_union_launches.bump(3); }

void lists_union_launch_counts(unsigned long long out[4]) { g_union_launches.read(out); }

}  // namespace fdnn
