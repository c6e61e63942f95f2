// fdnn_half_set.hip -- the half net's LAZY OUTPUT FOR PER-SEGMENT NODE SETS on v_mfma_f32_32x32x16_f16.  Contract, LDS image
// and grid arithmetic: fdnn_half_set.hpp; C-ABI: fdnn_half_api.cpp; DESIGN section 34.
//
//   hset_kernel<TAP, FT>     W-STATIONARY, where hgemm_kernel and hsmall_kernel stream both operands.  A workgroup of 256
//                            threads owns ONE 32-entry tile of one segment's set and frame tiles [t_begin, t_end) of that
//                            segment (hset::block_tile over the by-value sets::Launch table, up to 64 segments a launch).
//   the W tile               the tile's 32 gathered weight rows, K_pad <= 2048, are brought to LDS ONCE, by direct
//                            global-to-LDS loads (buffer_load_dwordx4 .. lds), each lane with its own row base under
//                            hset::row_offset's guard: a slot past `len`, a node outside [0, O) and a k >= K_pad carry an
//                            offset past the descriptor, fetch nothing and leave zeros.  32 loads per wave at K_pad 2048, one
//                            wait, one barrier -- the only barrier of the kernel.  The 32 biases go beside the tile, NaN
//                            for a bad node, so its z and e are NaN by the epilogue's own arithmetic.
//   the frame loop           after the barrier the four waves are independent: wave w takes frame tiles t_begin + FT w ..,
//                            stepping 4 FT, FT = 1 or 2 tiles of 32 frames against every W fragment it reads.  A wave that
//                            reads the whole tile per frame tile moves 128 KB; four of them 4096 clocks of the LDS's 128
//                            bytes / clock against 4096 clocks of that wave's 128 MFMAs.  So where a workgroup has more than
//                            four frame tiles (FT = 2) a fragment serves two: LDS : MFMA = 0.5.  Up to four tiles go one to
//                            a wave (FT = 1): four waves at ratio 1 finish sooner than two at 0.5.
//   X                        straight from global memory (L2) to registers, no LDS: a lane's fragment is the 16 contiguous
//                            bytes k = 16 kk + 8 (lane >> 5) .. + 7 of its frame row, lanes l and l + 32 together 32.  A k-STAGE
//                            is 8 MFMA steps = 128 k: the loads of stage s + 1 (8 FT x 16 bytes a lane) are issued before the
//                            MFMAs of stage s, two register buffers.  The descriptor ends at the SEGMENT's last row, so the
//                            next segment's rows that fall into a tile's 32 read zeros, and nothing is stored for them.
//   same bytes               instruction, operand roles (A = 32 nodes of W, B = 32 frames of X), the lane's k, kk ascending
//                            in ONE chain per output from +0, exactly K_pad / 16 steps (a zero past K_pad would be a +0
//                            product: never issued), the bias in the epilogue: hgemm_kernel's.
//   epilogue                 D[node][frame]: lane & 31 is the frame, register 4 q + t entry 8 q + 4 (lane >> 5) + t of the tile.
//                            z = acc + bias, e = exp2(z log2 e) to probs[out_off + r len + j]; TAP also stores z.
//   hset_gather_kernel       the fallback of K_pad > 2048: the listed entries out of the dense exp launch's e [m][O].
// No inline assembly, no atomics, no device state.
#include <hip/hip_runtime.h>

#include <atomic>

#include "fdnn_act.hpp"     // kLog2e
#include "fdnn_device.hpp"  // FDNN_LDS_PTR
#include "fdnn_half_set.hpp"
#include "fdnn_launch.hpp"

namespace fdnn {
namespace hset {
namespace {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));

LaunchCounts<kLaunchKinds> g_set_launches;

[[maybe_unused]] constexpr int kStageSteps = 8;  // MFMA steps per k-stage: 128 k, half a block of the image
// s_waitcnt vmcnt(0) alone (gfx9 encoding: vmcnt in bits 3:0 and 15:14; expcnt and lgkmcnt left at their maxima)
[[maybe_unused]] constexpr int kVmcnt0 = 0x0f70;

template <bool TAP, int FT>
__global__ __launch_bounds__(256) void hset_kernel(Params p, sets::Launch l) {
  static_assert(FT == 1 || FT == 2, "one or two frame tiles per W fragment");
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const sets::Tile tile = hset::block_tile(l, blockIdx.x);
  const int s = __builtin_amdgcn_readfirstlane(tile.seg);
  const int m0 = __builtin_amdgcn_readfirstlane(tile.m0);
  const int t_begin = __builtin_amdgcn_readfirstlane(tile.t_begin), t_end = __builtin_amdgcn_readfirstlane(tile.t_end);
  const int row0 = l.row0[s], rows = l.rows[s], len = l.len[s], out_off = l.out_off[s];
  const int32_t *set = p.nodes + l.set_off[s];

  // ---- the gather: 16 pieces per block of 256 k, four per wave; lane l of a piece is slot l & 31 of row piece + 16 (l >> 5)
  {
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(p.w), 0, p.rows_pad * p.K_pad * 2, 0x00020000);
    int roff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = m0 + wave * 4 + i + 16 * (lane >> 5);
      roff[i] = row_offset(j < len ? set[j] : -1, p.rows, p.K_pad);
    }
    const int blocks = (p.K_pad + kBlockK - 1) / kBlockK;
    for (int b = 0; b < blocks; ++b) {
      const int k = b * kBlockK + 8 * (lane & 31);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int voff = k < p.K_pad && roff[i] != kNoRead ? roff[i] + 2 * k : kNoRead;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, FDNN_LDS_PTR(lds + b * kBlockBytes + (wave * 4 + i) * kPieceStride), 16, voff, 0, 0, 0);
      }
    }
    if (tid < kNodeTile) {
      const int32_t node = m0 + tid < len ? set[m0 + tid] : -1;
      reinterpret_cast<float *>(lds + kWBytes)[tid] = set::node_ok(node, p.rows) ? p.bias[node] : __builtin_nanf("");
    }
    __builtin_amdgcn_s_waitcnt(kVmcnt0);
    __syncthreads();  // every wave's pieces have landed: the tile is read-only from here on
  }

  // ---- the frame loop: no barrier, the waves are independent
  const __amdgpu_buffer_rsrc_t rsrc_x =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(p.a + static_cast<size_t>(row0) * p.lda), 0, ((rows - 1) * p.lda + p.K_pad) * 2, 0x00020000);
  // row lane & 31 of the tile, k = 8 (lane >> 5) .. + 7 of an MFMA's 16
  const char *wfrag = lds + (lane & 15) * kPieceStride + ((lane >> 4) & 1) * 512 + 16 * (lane >> 5);
  const float *bias_s = reinterpret_cast<const float *>(lds + kWBytes);
  const int steps = p.K_pad / 16, full = steps / kStageSteps;

  for (int u = t_begin + FT * wave; u < t_end; u += 4 * FT) {
    int xoff[FT];  // byte offset of the lane's first fragment, or past the descriptor: a tile of another workgroup, a row of another segment
#pragma unroll
    for (int i = 0; i < FT; ++i) {
      const int frame = (u + i) * kFrameTile + (lane & 31);
      xoff[i] = u + i < t_end && frame < rows ? (frame * p.lda + 8 * (lane >> 5)) * 2 : kNoRead;
    }
    v16f acc[FT];
#pragma unroll
    for (int i = 0; i < FT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    auto load_x = [&](v4u(&x)[FT][kStageSteps], int st) {  // in the order the MFMAs take them: a step waits for its own loads only
#pragma unroll
      for (int kk = 0; kk < kStageSteps; ++kk)
#pragma unroll
        for (int i = 0; i < FT; ++i) x[i][kk] =__builtin_amdgcn_raw_buffer_load_b128(rsrc_x, xoff[i] + 32 * (kStageSteps * st + kk), 0, 0);
    };
    auto mfmas = [&](const v4u(&x)[FT][kStageSteps], int st) {
      const char *wt = wfrag + (st >> 1) * kBlockBytes + (st & 1) * (32 * kStageSteps);
      v8h a[kStageSteps];
#pragma unroll
      for (int kk = 0; kk < kStageSteps; ++kk) a[kk] = *reinterpret_cast<const v8h *>(wt + 32 * kk);
#pragma unroll
      for (int kk = 0; kk < kStageSteps; ++kk)
#pragma unroll
        for (int i = 0; i < FT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk], __builtin_bit_cast(v8h, x[i][kk]), acc[i], 0, 0, 0);
    };

    v4u xa[FT][kStageSteps], xb[FT][kStageSteps];
    if (full > 0) load_x(xa, 0);
    int st = 0;
    for (; st + 1 < full; st += 2) {
      load_x(xb, st + 1);
      __builtin_amdgcn_sched_barrier(0);  // (the next stage's loads stay ahead of this stage's MFMAs)
      mfmas(xa, st);
      if (st + 2 < full) load_x(xa, st + 2);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(xb, st + 1);
    }
    if (st < full) mfmas(xa, st);
    for (int kk = full * kStageSteps; kk < steps; ++kk) {  // a K_pad that is no multiple of 128: the last 2, 4 or 6 steps
      const v8h a = *reinterpret_cast<const v8h *>(wfrag + (kk >> 4) * kBlockBytes + (kk & 15) * 32);
#pragma unroll
      for (int i = 0; i < FT; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(v8h, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, xoff[i] + 32 * kk, 0, 0)), acc[i], 0, 0, 0);
    }

#pragma unroll
    for (int i = 0; i < FT; ++i) {
      const int frame = (u + i) * kFrameTile + (lane & 31);
      const bool live = u + i < t_end && frame < rows;
      const size_t row = static_cast<size_t>(out_off) + static_cast<size_t>(frame) * len;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int jl = 8 * q + 4 * (lane >> 5) + t;
          const float z = acc[i][4 * q + t] + bias_s[jl];  // NaN for a bad node
          if (live && m0 + jl < len) {
            if (TAP) p.z[row + m0 + jl] = z;
            p.probs[row + m0 + jl] = __builtin_amdgcn_exp2f(z * kLog2e);
          }
        }
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

// Workgroup (s, y) copies entries y, y + gridDim.y, .. of segment s's block, 256 at a time.
__global__ __launch_bounds__(256) void hset_gather_kernel(Params p, const float *e, const float *zd, sets::Launch l) {
  const int s = blockIdx.x;
  const int row0 = l.row0[s], len = l.len[s], out_off = l.out_off[s];
  const int32_t *set = p.nodes + l.set_off[s];
  const int total = l.rows[s] * len;
  for (int i = blockIdx.y * 256 + threadIdx.x; i < total; i += gridDim.y * 256) {
    const int r = i / len, j = i - r * len;
    const int32_t node = set[j];
    const bool ok = set::node_ok(node, p.rows);
    const size_t src = static_cast<size_t>(row0 + r) * p.rows + (ok ? node : 0);
    p.probs[out_off + i] = ok ? e[src] : __builtin_nanf("");
    if (zd != nullptr) p.z[out_off + i] = ok ? zd[src] : __builtin_nanf("");
  }
}

template <bool TAP, int FT>
void launch_instance(const Params &p, const sets::Launch &l, hipStream_t s) {
  auto kernel = hset_kernel<TAP, FT>;
  static std::atomic<unsigned long long> attr_set{0};  // dynamic LDS above 64 KB: once per device
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(sets::blocks(l))), dim3(256), kLdsBytes, s, p, l);
}

}  // namespace

void launch_score(const Params &p, const sets::Launch &l, ihipStream_t *s) {
  if (sets::blocks(l) <= 0 || p.K_pad > kMaxK) return;  // (set_step asks hset::applies first)
  const bool tap = p.z != nullptr, two = l.tiles_per_group > 4;
  g_set_launches.bump(tap ? 1 : 0);
  if (tap && two) launch_instance<true, 2>(p, l, s);
  else if (tap) launch_instance<true, 1>(p, l, s);
  else if (two) launch_instance<false, 2>(p, l, s);
  else launch_instance<false, 1>(p, l, s);
}

void launch_gather(const Params &p, const float *e, const float *zd, const sets::Launch &l, ihipStream_t *s) {
  if (sets::blocks(l) <= 0) return;
  g_set_launches.bump(2);
  hipLaunchKernelGGL(hset_gather_kernel, dim3(static_cast<unsigned>(l.n_segs), 32), dim3(256), 0, s, p, e, zd, l);
}

void launch_counts(unsigned long long out[kLaunchKinds]) { g_set_launches.read(out); }

}  // namespace hset
}  // namespace fdnn
