// fdnn_set_tile.hpp -- the tile of the set kernels: 64 gathered nodes x 32 frames on the int8 MFMA, run once per workgroup.
// fdnn_set.hip (one set for a row range) and fdnn_sets.hip (one set per segment, several segments in one launch) build a
// SetView for their workgroup and call set_tile: the operations on a (row, node) pair are the same instructions in the same
// order in both, which is what makes a row's bytes depend on the row and its set only.  How the tile works: fdnn_set.hip.
// fdnn_lists_union.hip runs the same tile on the union of a frame group's lists and, through a store policy of its own,
// hands back only the entries the caller listed.
#pragma once
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_tile.hpp"  // row256_pos; brings fdnn_pair.hpp

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

// The launch of a score kernel over set_tile: kStThreads threads and kStLds of dynamic LDS, whose limit is raised once per
// device and kernel instance (the bit set below belongs to this instantiation, hence the kernel as a template argument).
template <auto Kernel, class... Args>
void launch_set_tile(unsigned blocks, hipStream_t s, const Args &...args) {
  static std::atomic<unsigned long long> attr_set{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kStLds);
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(kStThreads), kStLds, s, args...);
}

// What one workgroup scores: rows [0, count) at `a`, entries [m0, m0 + 64) of the set nodes[len], frame tiles
// [t_begin, t_end) counted from a's first row; e of (row r, entry j) goes where the store policy says (DenseStore:
// probs[r * len + j]).  Everything here is
// workgroup-uniform.  The layer itself (w, bias, wsum, the pair index, rows, K, ldw, coef) is read from SetParams.
struct SetView {
  const int8_t *a;
  int count, lda;
  const int32_t *nodes;
  int len;
  float *probs;
  int32_t *acc;
  int m0, t_begin, t_end;
};

// Where a tile's results go.  The tile hands every (row, entry) of the view it has scored to entry(): o = row * len + entry,
// both counted inside the view, (f, jl) the same pair inside the 32 x 64 tile, `cur` the activation buffer the tile has just
// consumed; and calls tile_done() once per frame tile, by every thread, between the last entry() and the barrier that
// releases that buffer (f0: the tile's first row).
//
// DenseStore, the set kernels': e of (row r, entry j) to probs[r * len + j], nothing else.
struct DenseStore {
  __device__ __forceinline__ void entry(const SetView &v, size_t o, int, int, int, float e, int a32) const {
    v.probs[o] = e;
    if (v.acc != nullptr) v.acc[o] = a32;  // parity tests only (fdnn_debug_ctx_set_acc)
  }
  __device__ __forceinline__ void tile_done(const SetView &, int, int) const {}
};

// Byte offset, inside one activation buffer, of the 16 bytes that epilogue thread (f, jl / 4) owns in wave region 0: of the
// eight partial chunks it has summed (one per region, same offset), this is the first.  No other thread reads or writes them.
[[maybe_unused]] __device__ __forceinline__ int st_park(int f, int jl) {
  return (jl >> 5) * 4096 + f * 128 + (((((jl >> 2) & 7) ^ f) & 7) << 4) + ((jl & 3) << 2);
}

// FIX: the layer has saturating pairs (the walk over a node's own list); FAST: validated 3-operation division
template <bool FIX, bool FAST, class Store = DenseStore>
__device__ __forceinline__ void set_tile(const SetParams &p, const SetView &v, const Store &st = Store()) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = v.m0, t_begin = v.t_begin, t_end = v.t_end;
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
    const int32_t node = je + i < v.len ? v.nodes[je + i] : -1;
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
    voff_a[i] = live ? (4 * i + r4) * v.lda + ch : set::kOutOfRange;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int j = m0 + 32 * half + 4 * i + r4;
      const int32_t node = j < v.len ? v.nodes[j] : -1;
      const int off = set::row_offset(node, p.rows, p.ldw);
      voff_w[half][i] = live && off != set::kOutOfRange ? off + ch : set::kOutOfRange;
    }
  }
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(p.w), 0, p.rows * p.ldw, 0x00020000);
  // the descriptor of frame tile t ends at the call's last row (readfirstlane: a descriptor in VGPRs turns every load
  // into a waterfall loop)
  auto a_rsrc = [&](int t) {
    const int f0 = t * kStFT;
    const int bytes = __builtin_amdgcn_readfirstlane(max(0, min(kStFT, v.count - f0)) * v.lda);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(v.a + static_cast<size_t>(f0) * v.lda), 0, bytes, 0x00020000);
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
    for (int s = 0; s < 8; ++s) wf[half][s] = *reinterpret_cast<const v4i *>(src + row256_pos(frow, 2 * s + fch));
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
        for (int s = 0; s < 8; ++s) b[s] = *reinterpret_cast<const v4i *>(at + row256_pos(frow, 2 * s + fch));
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
      if (ff < v.count) {
        const int8_t *arow = v.a + static_cast<size_t>(ff) * v.lda;
        const size_t o = static_cast<size_t>(ff) * v.len + je;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (je + i >= v.len) continue;
          float e = __builtin_nanf("");  // a node outside the layer: NaN, and so is its row's total
          int a32 = 0;
          if (ok[i]) {
            a32 = sv[i];
            if (FIX) {
              // saturating pairs (rare): the reference clamps a[2j]*w[2j] + a[2j+1]*w[2j+1] to int16 (dnn.cc:337-340)
              for (int x = fb[i]; x < fe[i]; ++x) {
                const PairEntry en = decode_pair(p.fix_pairs[x]);
                const uint32_t pair = *reinterpret_cast<const uint16_t *>(arow + en.k);  // k is even
                a32 += pair_excess(pair, en.w0, en.w1);
              }
            }
            const float z = dequant<FAST>(a32, p.coef, p.rcp_coef) + bias4[i];
            e = logit_exp(z);
          }
          st.entry(v, o + i, f, 32 * h + 4 * q + i, cur, e, a32);
        }
      }
    }
    st.tile_done(v, f0, cur);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every partial is read: the buffer may be refilled
    asm volatile("" ::: "memory");
    if (t + 2 < t_end && slice_live) load_a(t + 2, at);
  }
#endif  // __HIP_DEVICE_COMPILE__
}

}  // namespace
}  // namespace fdnn
