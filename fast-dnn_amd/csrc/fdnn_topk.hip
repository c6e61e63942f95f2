// fdnn_topk.hip -- the dense output with a TOP-K RETURN: of every row of probabilities the k first-ranked nodes and their
// values (fdnn_topk.hpp: the order, the plan, the host restatement).
//
//   CalculateOutput (dnn.cc:428-454) hands every caller output_dim floats per frame; a caller that keeps the best few
//   senones of a frame -- first-pass pruning, posteriorgrams, confidence, keyword spotting -- throws the rest away after
//   3.2 MB per 100 frames of the 8000-node net have crossed PCIe.  Here the device chooses: n x k x 8 bytes leave it.
//
// One workgroup of 256 threads per row, exact selection, no special case for inf / NaN (the key is a total order):
//
//   * RESIDENT form (width <= kTopkResidentWidth): the row is read from memory ONCE -- 16-byte loads from the first
//     16-byte boundary of the row on, the up to three values before it and after the last whole vector one by one -- and
//     kept in LDS as keys, shifted by the row's misalignment so that a 16-byte load lands as a 16-byte LDS store.
//   * the k-th key by a radix select over the 32-bit keys, eight bits a pass, most significant first: a digit histogram
//     of the keys that still match the prefix (LDS atomics on integer counts: their order cannot change the result), a
//     scan from the top bin down, the bin that holds the k-th element extends the prefix.  After four passes the prefix IS
//     the threshold key and the scan's remainder says how many of its ties belong to the result.
//   * every key above the threshold is compacted (a ballot per 64 nodes, one LDS atomic per wave and chunk); the ties at
//     the threshold are taken in ascending node order: each wave walks a quarter of the row in 64-node chunks, counts its
//     ties, and after one exchange of the four counts places them by ballot / prefix count.
//   * the k (key, ~node) words are put in rank order by a rank sort in LDS (each counts the words above its own) and the
//     pairs leave as two whole [k] segments.
//   * STREAMING form (wider rows, fdnn_debug_set_topk_kernel(2)): the same passes re-reading the row from memory -- six
//     reads of a row that stays in L2 / Infinity Cache.  Same code, same bytes.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_topk.hpp"

namespace fdnn {
namespace {

using namespace topk;

LaunchCounts<2> g_topk_launches;  // resident, streaming
std::atomic<int> g_topk_mode{0};  // fdnn_debug_set_topk_kernel

template <bool RESIDENT>
__global__ __launch_bounds__(kThreads) void topk_kernel(const float *rows, int width, int k, int32_t *nodes, float *vals) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t *hist = smem;                                                // [kBins][kHistCopies]; at the end: nodes [256], values [256]
  uint64_t *cand = reinterpret_cast<uint64_t *>(smem + kHistWords);     // [kTopkMaxK] pair words
  uint32_t *misc = smem + kHistWords + kCandWords;                      // [0..3] wave sums, [4] digit, [5] k left, [6] compacted, [8..11] ties per wave
  uint32_t *keys = smem + kKeysAt;                                      // resident: [width + 4]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t *row = reinterpret_cast<const uint32_t *>(rows) + static_cast<size_t>(blockIdx.x) * width;
  const int off = RESIDENT ? static_cast<int>((reinterpret_cast<uintptr_t>(row) >> 2) & 3) : 0;
  auto load = [&](int i) -> uint32_t { return RESIDENT ? keys[off + i] : key(row[i]); };

  for (int i = t; i < kHistWords; i += kThreads) hist[i] = 0;
  if (t < kMiscWords) misc[t] = 0;
  if (RESIDENT) {
    const int head = min(width, (4 - off) & 3), nvec = (width - head) >> 2, tail = head + 4 * nvec;
    if (t < head) keys[off + t] = key(row[t]);
    for (int v = t; v < nvec; v += kThreads) {
      uint4 q = *reinterpret_cast<const uint4 *>(row + head + 4 * v);
      q.x = key(q.x), q.y = key(q.y), q.z = key(q.z), q.w = key(q.w);
      *reinterpret_cast<uint4 *>(keys + off + head + 4 * v) = q;
    }
    if (t < width - tail) keys[off + tail + t] = key(row[tail + t]);
  }
  __syncthreads();

  // ---- radix select: the k-th key
  uint32_t prefix = 0, decided = 0;
  int k_left = k;
  for (int shift = 32 - kDigitBits; shift >= 0; shift -= kDigitBits) {
    for (int i = t; i < width; i += kThreads) {
      const uint32_t kk = load(i);
      if ((kk & decided) == prefix) atomicAdd(&hist[(((kk >> shift) & (kBins - 1)) << 2) | (lane & 3)], 1u);
    }
    __syncthreads();
    const int bin = kBins - 1 - t;  // thread order = descending bins: the inclusive scan counts the keys at or above a bin
    const uint4 h = *reinterpret_cast<const uint4 *>(hist + 4 * bin);
    *reinterpret_cast<uint4 *>(hist + 4 * bin) = uint4{0, 0, 0, 0};
    const int c = static_cast<int>(h.x + h.y + h.z + h.w);
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    if (lane == 63) misc[wave] = static_cast<uint32_t>(incl);
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += static_cast<int>(misc[w]);
    if (incl - c < k_left && k_left <= incl) {
      misc[4] = static_cast<uint32_t>(bin);
      misc[5] = static_cast<uint32_t>(k_left - (incl - c));
    }
    __syncthreads();
    prefix |= misc[4] << shift;
    decided |= static_cast<uint32_t>(kBins - 1) << shift;
    k_left = static_cast<int>(misc[5]);
  }
  const uint32_t thr = prefix;   // the k-th key; k_left of the nodes that hold it belong to the result
  const int above = k - k_left;  // keys above it

  // ---- compaction: each wave walks its quarter of the row in index order
  const int span = (((width + 3) >> 2) + 63) & ~63;
  const int lo = min(width, wave * span), hi = min(width, lo + span);
  const unsigned long long below = (1ull << lane) - 1;
  int ties = 0;
  for (int i0 = lo; i0 < hi; i0 += 64) {
    const int i = i0 + lane;
    const uint32_t kk = i < hi ? load(i) : 0u;
    const unsigned long long gt = __ballot(i < hi && kk > thr), eq = __ballot(i < hi && kk == thr);
    ties += __popcll(eq);
    if (gt != 0) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&misc[6], static_cast<uint32_t>(__popcll(gt)));
      base = static_cast<uint32_t>(__shfl(static_cast<int>(base), 0));
      const uint32_t slot = base + static_cast<uint32_t>(__popcll(gt & below));
      if (i < hi && kk > thr && slot < static_cast<uint32_t>(kTopkMaxK)) cand[slot] = pair_word(kk, i);
    }
  }
  if (lane == 0) misc[8 + wave] = static_cast<uint32_t>(ties);
  __syncthreads();
  int seen = 0;  // ties at lower nodes than this wave's
  for (int w = 0; w < wave; ++w) seen += static_cast<int>(misc[8 + w]);
  if (ties > 0) {
    for (int i0 = lo; i0 < hi && seen < k_left; i0 += 64) {
      const int i = i0 + lane;
      const bool mine = i < hi && load(i) == thr;
      const unsigned long long eq = __ballot(mine);
      const int rank = seen + __popcll(eq & below);
      if (mine && rank < k_left) cand[above + rank] = pair_word(thr, i);
      seen += __popcll(eq);
    }
  }
  __syncthreads();

  // ---- rank order, then the pairs as whole segments
  if (t < k) {
    const uint64_t mine = cand[t];
    int rank = 0;
    for (int j = 0; j < k; ++j) rank += cand[j] > mine ? 1 : 0;
    hist[rank] = ~static_cast<uint32_t>(mine);
    hist[kTopkMaxK + rank] = unkey(static_cast<uint32_t>(mine >> 32));
  }
  __syncthreads();
  if (t < k) {
    const size_t at = static_cast<size_t>(blockIdx.x) * k + t;
    nodes[at] = static_cast<int32_t>(hist[t]);
    reinterpret_cast<uint32_t *>(vals)[at] = hist[kTopkMaxK + t];
  }
}

}  // namespace

void launch_topk(const float *d_rows, int n, int width, int k, int32_t *d_nodes, float *d_vals, hipStream_t s) {
  if (n <= 0 || !topk::args_ok(width, k)) return;
  const Plan p = topk::plan(n, width, g_topk_mode.load(std::memory_order_relaxed));
  static std::atomic<unsigned long long> attr_set{0};  // per device: the resident form's LDS may pass the default limit
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(topk_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              topk::plan(1, kTopkResidentWidth, 0).lds_bytes);
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  for (int r = 0; r < n; r += p.rows_per_launch) {
    const int cnt = std::min(p.rows_per_launch, n - r);
    const float *rows = d_rows + static_cast<size_t>(r) * width;
    int32_t *nd = d_nodes + static_cast<size_t>(r) * k;
    float *vl = d_vals + static_cast<size_t>(r) * k;
    g_topk_launches.bump(p.form == kResident ? 0 : 1);
    if (p.form == kResident)
      hipLaunchKernelGGL(topk_kernel<true>, dim3(cnt), dim3(kThreads), p.lds_bytes, s, rows, width, k, nd, vl);
    else
      hipLaunchKernelGGL(topk_kernel<false>, dim3(cnt), dim3(kThreads), p.lds_bytes, s, rows, width, k, nd, vl);
  }
}

void topk_launch_counts(unsigned long long out[2]) { g_topk_launches.read(out); }
int topk_kernel_mode() { return g_topk_mode.load(std::memory_order_relaxed); }
void topk_kernel_mode(int mode) { g_topk_mode.store(mode, std::memory_order_relaxed); }

}  // namespace fdnn
