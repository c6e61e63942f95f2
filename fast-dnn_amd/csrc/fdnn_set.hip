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
// partial 64 x 32 int32 tiles meet in LDS.
#include <algorithm>
#include <atomic>

#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"

namespace fdnn {
namespace {

constexpr int kStWaves = 8;
constexpr int kStThreads = 64 * kStWaves;
constexpr int kStSlice = 256;                            // bytes of K per wave
constexpr int kStFT = set::kFrameTile;
constexpr int kStABuf = kStWaves * kStFT * kStSlice;     // one activation tile: 64 KiB
constexpr int kStLds = 2 * kStABuf;
static_assert(kStWaves * kStSlice == set::kMaxK && set::kNodeTile == 64 && kStFT == 32, "fdnn_set.hpp states this kernel's sizes");
static_assert(kStLds <= 160 * 1024, "LDS");

std::atomic<unsigned long long> g_set_launches[3];  // MFMA kernel without / with the pair walk, calls served by the list kernels
std::atomic<int> g_set_mode{0};                     // fdnn_debug_set_kernel

// chunk c (16 bytes) of row r of a 256-byte-row LDS image lives at chunk position c ^ (r & 15) (as fdnn_small.hip)
[[maybe_unused]] __device__ __forceinline__ int st_pos(int row, int chunk) { return (row << 8) + (((chunk ^ row) & 15) << 4); }

// FIX: the layer has saturating pairs (the walk over a node's own list); FAST: validated 3-operation division
template <bool FIX, bool FAST>
__global__ __launch_bounds__(kStThreads, 2) void set_score_kernel(SetParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const set::Tile tile = set::block_tile(p.plan, blockIdx.x);
  const int m0 = tile.m0, t_begin = tile.t_begin, t_end = tile.t_end;
  if (t_begin >= t_end) return;

  // ---- the epilogue's four entries of this thread: (frame f, entries je .. je + 3); what belongs to their nodes is
  // gathered once, in front of the operand loads (an older load never makes a wait for the operands longer)
  const int f = (tid >> 3) & 31, q = tid & 7, h = tid >> 8;
  const int je = m0 + 32 * h + 4 * q;
  bool ok[4];
  int wsum4[4], fb[4], fe[4];
  float bias4[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int32_t node = je + i < p.len ? p.nodes[je + i] : -1;
    ok[i] = set::node_ok(node, p.rows);
    wsum4[i] = 0, fb[i] = 0, fe[i] = 0, bias4[i] = 0.0f;
    if (ok[i]) {
      wsum4[i] = p.wsum[node];  // 128 * sum_k w[node][k]: the s8 = u8 - 128 activation offset
      bias4[i] = p.bias[node];
      if (FIX) {
        fb[i] = p.fix_off[node];
        fe[i] = p.fix_off[node + 1];
      }
    }
  }

  // this wave's K slice; lanes past the layer's K (K is a multiple of 16, the slice 256) fetch nothing
  const int k0 = wave * kStSlice;
  const bool slice_live = k0 < p.K;
  const int r4 = lane >> 4, c16 = lane & 15;
  char *const abuf0 = smem + wave * (kStFT * kStSlice);  // this wave's 8 KiB of activation buffer 0; buffer 1 at + kStABuf
  // per-lane offsets of the eight 1-KiB loads of a 32-row image (rows 4i + r4): SOURCE chunk = lane chunk XOR row; a
  // source chunk past K, a row without a node and a row past the call are not fetched
  int voff_w[2][8], voff_a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ch = ((c16 ^ r4 ^ (4 * i)) & 15) << 4;
    const bool live = k0 + ch < p.K;
    voff_a[i] = live ? (4 * i + r4) * p.lda + ch : set::kOutOfRange;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int j = m0 + 32 * half + 4 * i + r4;
      const int32_t node = j < p.len ? p.nodes[j] : -1;
      const int off = set::row_offset(node, p.rows, p.ldw);
      voff_w[half][i] = live && off != set::kOutOfRange ? off + ch : set::kOutOfRange;
    }
  }
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(p.w), 0, p.rows * p.ldw, 0x00020000);
  // the descriptor of frame tile t ends at the call's last row (readfirstlane: a descriptor in VGPRs turns every load
  // into a waterfall loop)
  auto a_rsrc = [&](int t) {
    const int f0 = t * kStFT;
    const int bytes = __builtin_amdgcn_readfirstlane(max(0, min(kStFT, p.count - f0)) * p.lda);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(p.a + static_cast<size_t>(f0) * p.lda), 0, bytes, 0x00020000);
  };
  auto load_w = [&](int half, char *dst) {  // 32 gathered weight rows x this wave's slice -> dst (8 KiB, wave private)
#pragma unroll
    for (int i = 0; i < 8; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, FDNN_LDS_PTR(dst + i * 1024), 16, voff_w[half][i], k0, 0, 0);
  };
  auto load_a = [&](int t, char *dst) {
    const __amdgpu_buffer_rsrc_t rsrc_a = a_rsrc(t);
#pragma unroll
    for (int i = 0; i < 8; ++i) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, FDNN_LDS_PTR(dst + i * 1024), 16, voff_a[i], k0, 0, 0);
  };
  const int frow = lane & 31, fch = lane >> 5;
  v4i wf[2][8];
  auto read_w = [&](int half, const char *src) {
#pragma unroll
    for (int s = 0; s < 8; ++s) wf[half][s] = *reinterpret_cast<const v4i *>(src + st_pos(frow, 2 * s + fch));
  };

  // ---- prologue: W half 0 through the (not yet needed) second activation buffer into registers, the first activation
  // tile beside it; half 1 follows through the same buffer while half 0's MFMAs run (first pass of the tile loop)
  if (slice_live) {
    load_w(0, abuf0 + kStABuf);
    load_a(t_begin, abuf0);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // older loads complete first: W half 0 has landed
    read_w(0, abuf0 + kStABuf);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    load_w(1, abuf0 + kStABuf);
  } else {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int s = 0; s < 8; ++s) wf[hh][s] = v4i{0, 0, 0, 0};
  }

  for (int t = t_begin; t < t_end; ++t) {
    const int cur = (t - t_begin) & 1;
    char *at = abuf0 + cur * kStABuf;
    const int f0 = t * kStFT;
    // D layout (32x32): column (frame) = lane & 31, row (node) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    v16i acc[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[hh][r] = 0;
    if (slice_live) {
      v4i b[8];
      auto read_b = [&]() {
#pragma unroll
        for (int s = 0; s < 8; ++s) b[s] = *reinterpret_cast<const v4i *>(at + st_pos(frow, 2 * s + fch));
      };
      if (t == t_begin) {
        // in flight are this tile (8 loads) and W half 1 (8 loads, younger)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        read_b();
#pragma unroll
        for (int s = 0; s < 8; ++s) acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[0][s], b[s], acc[0], 0, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        read_w(1, abuf0 + kStABuf);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < t_end) load_a(t + 1, abuf0 + kStABuf);
#pragma unroll
        for (int s = 0; s < 8; ++s) acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[1][s], b[s], acc[1], 0, 0, 0);
      } else {
        if (t + 1 < t_end)
          asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // tile t landed, tile t + 1 (8 loads) may still fly
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        read_b();
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) acc[hh] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[hh][s], b[s], acc[hh], 0, 0, 0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    // partial tile -> this wave's own (just consumed) 8 KiB of the activation buffer: [half][frame][32 nodes] int32,
    // 16-byte chunk c of a frame row at position c ^ (frame & 7)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<v4i *>(at + hh * 4096 + frow * 128 + ((((2 * g + fch) ^ frow) & 7) << 4)) =
            v4i{acc[hh][g * 4], acc[hh][g * 4 + 1], acc[hh][g * 4 + 2], acc[hh][g * 4 + 3]};
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // ---- reduce + epilogue: thread -> (frame f, entries je .. je + 3)
    {
      v4i sum = v4i{wsum4[0], wsum4[1], wsum4[2], wsum4[3]};
#pragma unroll
      for (int w = 0; w < kStWaves; ++w)
        sum += *reinterpret_cast<const v4i *>(smem + cur * kStABuf + w * (kStFT * kStSlice) + h * 4096 + f * 128 + (((q ^ f) & 7) << 4));
      const int sv[4] = {sum.x, sum.y, sum.z, sum.w};
      const int ff = f0 + f;
      if (ff < p.count) {
        const int8_t *arow = p.a + static_cast<size_t>(ff) * p.lda;
        const size_t o = static_cast<size_t>(ff) * p.len + je;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (je + i >= p.len) continue;
          float e = __builtin_nanf("");  // a node outside the layer: NaN, and so is its row's total
          int a32 = 0;
          if (ok[i]) {
            a32 = sv[i];
            if (FIX) {
              // saturating pairs (rare): the reference clamps a[2j]*w[2j] + a[2j+1]*w[2j+1] to int16 (dnn.cc:337-340)
              for (int x = fb[i]; x < fe[i]; ++x) {
                const uint32_t raw = p.fix_pairs[x];
                const int k = static_cast<int>(raw & 0xffffu);
                const int w0 = static_cast<int8_t>(raw >> 16), w1 = static_cast<int8_t>(raw >> 24);
                const uint32_t pair = *reinterpret_cast<const uint16_t *>(arow + k);  // k is even
                const int a0 = static_cast<int>((pair & 0xff) ^ 0x80), a1 = static_cast<int>((pair >> 8) ^ 0x80);  // back to u8
                const int prod = a0 * w0 + a1 * w1;
                a32 += max(-32768, min(32767, prod)) - prod;
              }
            }
            const float z = dequant<FAST>(a32, p.coef, p.rcp_coef) + bias4[i];
            const float y = z * 1.44269504088896340736f;
            e = __builtin_amdgcn_exp2f(y);
          }
          p.probs[o + i] = e;
          if (p.acc != nullptr) p.acc[o + i] = a32;  // parity tests only (fdnn_debug_ctx_set_acc)
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every partial is read: the buffer may be refilled
    asm volatile("" ::: "memory");
    if (t + 2 < t_end && slice_live) load_a(t + 2, at);
  }
#endif  // __HIP_DEVICE_COMPILE__
}

// The fallback's lists: row r of the call is entries [r * len, (r + 1) * len), each row the set itself.
__global__ __launch_bounds__(256) void set_expand_kernel(const int32_t *nodes, int len, int count, int32_t *row_ptr, int32_t *rep) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < static_cast<long long>(count) * len) rep[i] = nodes[i % len];
  if (i <= count) row_ptr[i] = static_cast<int32_t>(i * len);
}

template <bool FIX, bool FAST>
void launch_set_cfg(const SetParams &p, hipStream_t s) {
  auto k = set_score_kernel<FIX, FAST>;
  static std::atomic<unsigned long long> attr_set{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, kStLds);
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(k, dim3(p.plan.blocks), dim3(kStThreads), kStLds, s, p);
}

}  // namespace

void launch_set_score(const SetParams &p, hipStream_t s) {
  if (p.plan.blocks <= 0) return;
  const bool fix = p.fix_off != nullptr && p.fix_pairs != nullptr;
  g_set_launches[fix ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
  if (fix && p.fastdiv)
    launch_set_cfg<true, true>(p, s);
  else if (fix)
    launch_set_cfg<true, false>(p, s);
  else if (p.fastdiv)
    launch_set_cfg<false, true>(p, s);
  else
    launch_set_cfg<false, false>(p, s);
}

void launch_set_expand(const int32_t *nodes, int len, int count, int32_t *row_ptr, int32_t *rep, hipStream_t s) {
  const long long items = std::max<long long>(static_cast<long long>(count) * len, static_cast<long long>(count) + 1);
  g_set_launches[2].fetch_add(1, std::memory_order_relaxed);
  hipLaunchKernelGGL(set_expand_kernel, dim3(static_cast<unsigned>((items + 255) / 256)), dim3(256), 0, s, nodes, len, count, row_ptr, rep);
}

void set_launch_counts(unsigned long long out[3]) {
  for (int i = 0; i < 3; ++i) out[i] = g_set_launches[i].load(std::memory_order_relaxed);
}

int set_kernel_mode() { return g_set_mode.load(std::memory_order_relaxed); }
void set_kernel_mode(int mode) { g_set_mode.store(mode, std::memory_order_relaxed); }

}  // namespace fdnn
