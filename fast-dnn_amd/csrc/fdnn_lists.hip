// fdnn_lists.hip -- lazy output by active-node LISTS: only the listed nodes of the output layer are scored.
//
//   LazyOutputActivations (dnn.cc:355-392): the listed nodes' logits, every other node's logit 0
//   SoftMax::apply (dnn.cc:534-544): e = exp(z), total, p = e / total; every unlisted node reads 1 / total
//
// The masked output kernels (fdnn_gemm.hip, fdnn_small.hip) compute the whole layer and mask in the epilogue: right for
// the reference's 40 % masks over a batch, where the matrix pipe does 8000 nodes in the time the weights stream once.
// A narrow active set (forced alignment, rescoring, keyword spotting: 1 .. tens of nodes per frame) needs count x len dot
// products of K bytes, and one frame of the per-frame protocol needs len weight rows, not all of them.  Here the work is
// the flat entry array (row, node):
//
//   score   a 16-lane group per entry: v_dot4c_i32_i8 over K of (s8 activation, s8 weight row), + 128 * sum(w), the
//           node's saturating pairs (its own list: fdnn_lists.hpp), the logit as every output path forms it, e = exp(z)
//           by fdnn_small.hip's instruction sequence.  A group takes `epg` consecutive entries and keeps its row's
//           activation bytes in registers while the row does not change; a workgroup is 16 groups = 16 * epg consecutive
//           entries, and the rows it spans are found by binary search in row_ptr.  The integer sum is order-free.
//   finish  one wave per row, the order is NORMATIVE (results do not depend on batch size, position or scheduling): lane
//           l adds e[l], e[l + 64], .. of its row in index order, an xor butterfly over 32, 16, 8, 4, 2, 1, then
//           + float(O - len) for the unlisted nodes' exp(0) (exact: O < 2^24); inactive = RN(1 / total), p = RN(e * inactive).
//
// A node outside [0, O) (device lists are not validated) is never used as an address: its e is NaN, and so is its row.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_pair.hpp"

namespace fdnn {
namespace {

constexpr int kLsThreads = 256;
constexpr int kLsLanes = 16;                       // lanes per entry
constexpr int kLsGroups = kLsThreads / kLsLanes;   // entries a workgroup scores side by side
constexpr int kLsChunk = kLsLanes * 16 * 8;        // bytes of K a group holds in registers: 8 x 16 bytes per lane = 2048

LaunchCounts<3> g_lists_launches;  // score without / with the pair walk, finish (fdnn_debug_lists_launches)

// FIX: the layer has saturating pairs (the walk over the node's own list); FAST: validated 3-operation division
template <bool FIX, bool FAST>
__global__ __launch_bounds__(kLsThreads) void lists_score_kernel(ListsParams p) {
  const int l16 = threadIdx.x & (kLsLanes - 1);
  const int group = threadIdx.x >> 4;
  const long long i0 = (static_cast<long long>(blockIdx.x) * kLsGroups + group) * p.epg;
  // the row of this group's first entry: the last r with row_ptr[r] <= i0, inside [0, count - 1] whatever row_ptr holds
  int r = 0;
  {
    int lo = 0, hi = p.count;  // row_ptr[lo] <= i0 (row_ptr[0] = 0), row_ptr[hi] > i0 or hi = count
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (p.row_ptr[mid] <= i0)
        lo = mid;
      else
        hi = mid;
    }
    r = lo;
  }
  v4i a[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) a[s] = v4i{0, 0, 0, 0};
  int held = -1;  // the row whose first kLsChunk bytes a[] holds
  const bool one_chunk = p.K <= kLsChunk;
  for (int j = 0; j < p.epg; ++j) {
    const long long i = i0 + j;
    const bool live = i < p.nnz;
    const int node = live ? p.nodes[i] : -1;
    const bool ok = live && static_cast<unsigned>(node) < static_cast<unsigned>(p.rows);
    if (live)
      while (r + 1 < p.count && p.row_ptr[r + 1] <= i) ++r;  // (empty rows are stepped over)
    int part = 0;
    if (ok) {
      const int8_t *arow = p.a + static_cast<size_t>(r) * p.lda;
      const int8_t *wrow = p.w + static_cast<size_t>(node) * p.ldw;
      for (int kc = 0; kc < p.K; kc += kLsChunk) {
        if (held != r || !one_chunk) {
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            const int k = kc + s * 256 + l16 * 16;
            a[s] = k < p.K ? *reinterpret_cast<const v4i *>(arow + k) : v4i{0, 0, 0, 0};
          }
          held = r;
        }
        v4i w[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int k = kc + s * 256 + l16 * 16;
          w[s] = k < p.K ? *reinterpret_cast<const v4i *>(wrow + k) : v4i{0, 0, 0, 0};
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          part = __builtin_amdgcn_sdot4(a[s].x, w[s].x, part, false);
          part = __builtin_amdgcn_sdot4(a[s].y, w[s].y, part, false);
          part = __builtin_amdgcn_sdot4(a[s].z, w[s].z, part, false);
          part = __builtin_amdgcn_sdot4(a[s].w, w[s].w, part, false);
        }
      }
      if (FIX) {
        // saturating pairs (rare): the reference clamps a[2j]*w[2j] + a[2j+1]*w[2j+1] to int16 (dnn.cc:337-340); the
        // activation pair comes from memory again (a line this group has just read)
        const int fe = p.fix_off[node + 1];
        for (int f = p.fix_off[node] + l16; f < fe; f += kLsLanes) {
          const PairEntry en = decode_pair(p.fix_pairs[f]);
          const uint32_t pair = *reinterpret_cast<const uint16_t *>(arow + en.k);  // k is even
          part += pair_excess(pair, en.w0, en.w1);
        }
      }
    }
    part += __shfl_xor(part, 8);
    part += __shfl_xor(part, 4);
    part += __shfl_xor(part, 2);
    part += __shfl_xor(part, 1);
    if (l16 == 0 && live) {
      float e = __builtin_nanf("");
      int acc = 0;
      if (ok) {
        acc = part + p.wsum[node];  // 128 * sum_k w[node][k]: the s8 = u8 - 128 activation offset
        const float z = dequant<FAST>(acc, p.coef, p.rcp_coef) + p.bias[node];
        e = logit_exp(z);
      }
      p.probs[i] = e;
      if (p.acc != nullptr) p.acc[i] = acc;  // parity tests only (fdnn_debug_ctx_lists_acc): the same for every lane
    }
  }
}

// UNIFORM: every row has p.row_len entries and there is no row_ptr (a shared node set, fdnn_set.hip): row r is
// [r * row_len, (r + 1) * row_len).  The order below is the same instruction for instruction.
template <bool UNIFORM>
__global__ __launch_bounds__(kLsThreads) void lists_finish_kernel(ListsParams p) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (kLsThreads / 64) + (threadIdx.x >> 6);
  if (r >= p.count) return;  // (whole waves)
  const int b = UNIFORM ? r * p.row_len : max(0, min(p.nnz, p.row_ptr[r]));
  const int e = UNIFORM ? b + p.row_len : max(b, min(p.nnz, p.row_ptr[r + 1]));
  float s = 0.0f;
  for (int i = b + lane; i < e; i += 64) s += p.probs[i];
  s += __shfl_xor(s, 32);
  s += __shfl_xor(s, 16);
  s += __shfl_xor(s, 8);
  s += __shfl_xor(s, 4);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 1);
  const float total = s + static_cast<float>(p.rows - (e - b));  // every unlisted node: exp(0) = 1 (dnn.cc:366-369)
  const float inv = 1.0f / total;
  for (int i = b + lane; i < e; i += 64) p.probs[i] = p.probs[i] * inv;
  if (lane == 0) p.inactive[r] = inv;
}

}  // namespace

void launch_lists_score(const ListsParams &p, hipStream_t s) {
  if (p.nnz <= 0) return;
  const long long per_block = static_cast<long long>(kLsGroups) * p.epg;
  const unsigned blocks = static_cast<unsigned>((p.nnz + per_block - 1) / per_block);
  const bool fix = p.fix_off != nullptr && p.fix_pairs != nullptr;
  g_lists_launches.bump(fix ? 1 : 0);
  with_fix_fast(fix, p.fastdiv, [&](auto FIX, auto FAST) {
    hipLaunchKernelGGL((lists_score_kernel<FIX(), FAST()>), dim3(blocks), dim3(kLsThreads), 0, s, p);
  });
}

void launch_lists_finish(const ListsParams &p, hipStream_t s) {
  if (p.count <= 0) return;
  g_lists_launches.bump(2);
  const int rows_per_block = kLsThreads / 64;
  const dim3 grid((p.count + rows_per_block - 1) / rows_per_block);
  if (p.row_ptr != nullptr)
    hipLaunchKernelGGL(lists_finish_kernel<false>, grid, dim3(kLsThreads), 0, s, p);
  else
    hipLaunchKernelGGL(lists_finish_kernel<true>, grid, dim3(kLsThreads), 0, s, p);
}

// Entries per 16-lane group: as many as leave the launch about four workgroups per CU -- one frame's 3 200 entries spread
// over 200 workgroups, 10 000 rows of 8 share their rows' activation bytes among 4 .. 8 entries.
int lists_entries_per_group(long long nnz, int n_cu) {
  const long long want = nnz / (static_cast<long long>(kLsGroups) * 4 * (n_cu > 0 ? n_cu : 256));
  return static_cast<int>(want < 1 ? 1 : want > 8 ? 8 : want);
}

void lists_launch_counts(unsigned long long out[3]) { g_lists_launches.read(out); }

}  // namespace fdnn
