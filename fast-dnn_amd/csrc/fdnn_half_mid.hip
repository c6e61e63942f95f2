// fdnn_half_mid.hip -- the half net's MID-BATCH GEMM: calls of 129 .. 4096 frames (hf::mid_applies), the bytes of
// hgemm_kernel (fdnn_half.hip).  Contract: fdnn_half.hpp; DESIGN section 35.
//
//   hmid_kernel<ACT, TAP>    act(X[m][K] . W[rows][K]^T + bias) for any m >= 1.  hgemm_kernel's 256 x 128 tile puts 64 workgroups
//                            on 256 CUs for a 2048-wide layer at 1000 frames, each of them 64 k-steps with the global-load
//                            latency exposed at every one.  This kernel is built around WORKGROUPS IN FLIGHT: a tile small
//                            enough to fill the device at these sizes, two workgroups to a CU, and the operands requested two
//                            stages ahead of the MFMAs that use them.
//   work split               a workgroup of 256 threads takes 64 frames x 64 nodes, the waves 2 x 2 (wm = wave >> 1 the frame
//                            half, wn = wave & 1 the node half), ONE 32 x 32 MFMA tile in 16 accumulator registers each.  The
//                            grid is (ceil(m / 64), rows_pad / 64): 512 workgroups for 2048 nodes at 1000 frames.  64 nodes
//                            are one soft-max partial: the output form owns whole partials.
//   same bytes               the instruction (v_mfma_f32_32x32x16_f16), the operand roles (A = 32 nodes of W, B = 32 frames of
//                            X), the lane's k (16 kk + 8 (lane >> 5) + 0 .. 7), kk ascending in ONE chain per output from +0,
//                            exactly K_pad / 16 steps (a step past K_pad would add +0 products: an s = -0 would turn +0), the
//                            bias in the epilogue, the epilogue's fp32 sequences and v_cvt_f16_f32: all hgemm_kernel's.  No
//                            split-K, no atomics.
//   the ring                 LDS is a ring of kRingStages = 2 STAGES of 128 k; a stage is the W tile (64 nodes) and the X tile
//                            (64 frames), 64 rows x 256 bytes each.  Every tile is loaded by direct global-to-LDS loads
//                            (buffer_load_dwordx4 .. lds): no register holds ring data.  A stage's fragments (8 MFMA steps x 2
//                            operands = 64 registers) are read to registers in one round, which FREES the stage's slot: it is
//                            refilled with stage s + 2 before stage s's MFMAs are issued.  Under a stage's MFMAs the loads
//                            of the two stages behind it are in flight; with the registers the pipeline is three stages deep
//                            on 66 560 bytes, so two workgroups (133 120 bytes) share a CU and one's barriers and epilogue run
//                            under the other's k-loop.  (A third ring stage is 99 840 bytes: one workgroup per CU.)
//   LDS image                a direct load writes the wave's 64 x 16 bytes CONTIGUOUSLY.  A row of a stage is 128 k = 256 bytes
//                            = 16 slots of 16 bytes, so one load is a PIECE of FOUR rows: rows r, r + 16, r + 32, r + 48 of
//                            the tile (r = 0 .. 15), lane l taking slot l & 15 of row r + 16 (l >> 4): a global read of four
//                            256-byte runs.  Inside a piece the four rows are 16 slots apart -- the same slot mod 16, and the
//                            LDS has 64 banks x 4 bytes = 16 slots: they would collide in one fragment read, which is why they
//                            are rows of four DIFFERENT groups of 16.  Pieces are 1040 bytes = 65 slots apart (one slot of
//                            padding): row r of the tile is at slot 65 (r & 15) + 16 (r >> 4) + c.  A fragment read takes the
//                            SAME slot c of 32 consecutive rows per half wave, and the LDS serves a b128 read in groups of 16
//                            consecutive lanes = 16 consecutive rows, all with the same r >> 4: 65 r mod 16 = r mod 16 (65 is
//                            odd, here 1 mod 16) is a permutation of the 16 rows, so the group falls on 16 distinct slots --
//                            no conflict, against the 16-way one of rows 256 bytes apart.  A fragment stays ONE ds_read_b128
//                            at a constant offset (32 kk) from the lane's base.  A tile is 16 pieces = 16 640 bytes.
//   pads                     a lane whose frame is >= m, or whose k is >= K_pad (the last stage of a K_pad that is no multiple
//                            of 128), carries an offset past its buffer descriptor's extent: it reads nothing from memory
//                            and the load writes zeros.  The X descriptor begins at the workgroup's first frame and ends with
//                            its last one's column K_pad.  Every wave issues every load (8 per wave and stage: pieces 4 wave
//                            .. 4 wave + 3 of W, then of X), so a wave's count of outstanding loads tells it which stages
//                            have landed, oldest first.
//   schedule                 per stage s: wait until the wave's own loads of stage s have landed (at most the 8 of stage s + 1
//                            outstanding), barrier, 16 fragment reads; where a stage s + 2 exists: wait for the reads,
//                            barrier, request stage s + 2 into the slot; then the 8 MFMAs.  A last stage of fewer than 8
//                            steps reads and multiplies step by step.
//   paper ratio              per 16 k a wave reads one W and one X fragment (2 KB) for one 32-cycle MFMA; four waves are 8 KB
//                            = 64 clocks of the LDS's 128 bytes / clock against 32 MFMA clocks per SIMD: the loop is LDS-bound
//                            at half the MFMA rate.  hgemm_kernel's tile has 0.75 and stays under 0.15 of the peak up to 1000
//                            frames: here the workgroups in flight count for more than the ratio.  (128 frames x 64 nodes: 1.5
//                            and half the workgroups)
//   epilogue                 D[node][frame] as in hgemm_kernel.  sigmoid: four consecutive nodes per lane leave as one 8-byte
//                            store; pad columns [rows, ldo) are written +0.  exp: the workgroup's e [64 frames][64 nodes] goes
//                            through the dead ring, rows 65 floats apart; the four waves send the rows out as 256-byte runs
//                            and lane = frame of wave 0 adds the 64-node partial, 32 + 32 sequential additions, then the
//                            halves (softmax_ref: DEPTH).  The tap forms also store z.
#include <hip/hip_runtime.h>

#include <atomic>

#include "fdnn_act.hpp"     // kLog2e
#include "fdnn_device.hpp"  // FDNN_LDS_PTR
#include "fdnn_half.hpp"
#include "fdnn_launch.hpp"

namespace fdnn {
namespace hf {
namespace {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef _Float16 v4h __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

LaunchCounts<kMidLaunchKinds> g_mid_launches;

constexpr int kStageK = 128;                                   // k per stage: a tile row is 256 bytes
[[maybe_unused]] constexpr int kStageSteps = kStageK / 16;                   // MFMA steps per full stage
constexpr int kPieceStride = 1040;                             // bytes between pieces: 65 slots
constexpr int kTileBytes = 16 * kPieceStride;                  // 64 rows x 128 k and 16 slots of padding
constexpr int kStageBytes = 2 * kTileBytes;                    // [W | X]
constexpr int kRingStages = 2;
constexpr int kMidLds = kRingStages * kStageBytes;             // 66 560
constexpr int kLoadsPerStage = 8;                              // per wave: 2 tiles x 16 pieces over four waves
constexpr int kEStride = 65;                                   // output epilogue: e [64 frames][64 nodes], rows 65 floats apart
[[maybe_unused]] constexpr int kNoRead = static_cast<int>(0x80000000u);  // an offset past every descriptor's extent
static_assert(kMidFrameTile == 64 && kMidNodeTile == 64 && kMidNodeTile == kPartialNodes, "hmid_kernel is written for 64 x 64: one partial");
static_assert(2 * kMidLds <= 160 * 1024, "two workgroups share a CU's LDS");
static_assert(kLoadsPerStage < 64, "the outstanding-load counter has 6 bits");
static_assert(kMidFrameTile * kEStride * 4 <= kMidLds, "the output epilogue's e tile reuses the ring");
static_assert(kPieceStride % 16 == 0 && (kPieceStride / 16) % 2 == 1, "pieces an odd number of 16-byte slots apart");

// s_waitcnt (gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt in 6:4, lgkmcnt in 11:8), the other counters left at their maxima
[[maybe_unused]] constexpr int vmcnt_imm(int c) { return (c & 15) | ((c >> 4) << 14) | 0x0f70; }
[[maybe_unused]] constexpr int kLdsReadsDone = 0xc07f;  // lgkmcnt(0)

template <int ACT, bool TAP>
__global__ __launch_bounds__(256, 2) void hmid_kernel(GemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char ring[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;  // the wave's 32 frames and 32 nodes inside the tile
  const int f0 = blockIdx.x * kMidFrameTile, nb = blockIdx.y * kMidNodeTile;
  const int frames = min(kMidFrameTile, p.n - f0);  // >= 1 by the grid
  const int stages = (p.K_pad + kStageK - 1) / kStageK;

  // the workgroup's rows of W, and its rows of X up to the last column read
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(p.w + static_cast<size_t>(nb) * p.K_pad), 0,
                                                                          kMidNodeTile * p.K_pad * 2, 0x00020000);  // nb + 64 <= rows_pad
  const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(p.a + static_cast<size_t>(f0) * p.lda), 0,
                                                                          ((frames - 1) * p.lda + p.K_pad) * 2, 0x00020000);

  // lane l of a piece: slot l & 15 of row piece + 16 (l >> 4)
  const int lrow = 16 * (lane >> 4), lk = 8 * (lane & 15);
  auto issue_stage = [&](int st) {
    const int k = st * kStageK + lk;
    const bool kin = k < p.K_pad;
    char *dst = ring + (st & (kRingStages - 1)) * kStageBytes + wave * 4 * kPieceStride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wave * 4 + i + lrow;
      const int voff = kin ? (row * p.K_pad + k) * 2 : kNoRead;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, FDNN_LDS_PTR(dst + i * kPieceStride), 16, voff, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wave * 4 + i + lrow;
      const int voff = kin && row < frames ? (row * p.lda + k) * 2 : kNoRead;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, FDNN_LDS_PTR(dst + kTileBytes + i * kPieceStride), 16, voff, 0, 0, 0);
    }
  };
  static_assert((kRingStages & (kRingStages - 1)) == 0, "the slot of a stage is its low bits");

  v16f acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

  issue_stage(0);
  if (stages > 1) issue_stage(1);

  // row lane & 31 of the wave's half of a tile, k = 8 (lane >> 5) .. + 7 of an MFMA's 16
  const int frag = (lane & 15) * kPieceStride + ((lane >> 4) & 1) * 256 + 16 * (lane >> 5);
  for (int s = 0; s < stages; ++s) {
    if (s + 1 < stages) __builtin_amdgcn_s_waitcnt(vmcnt_imm(kLoadsPerStage));  // stage s + 1 may be on its way
    else __builtin_amdgcn_s_waitcnt(vmcnt_imm(0));
    __builtin_amdgcn_s_barrier();  // every wave's share of the stage has landed
    const char *wt = ring + (s & (kRingStages - 1)) * kStageBytes + 512 * wn + frag;
    const char *xt = ring + (s & (kRingStages - 1)) * kStageBytes + kTileBytes + 512 * wm + frag;
    const int steps = min(p.K_pad - s * kStageK, kStageK) / 16;  // K_pad is a multiple of 32: 8, or 2, 4, 6 in a last stage
    if (steps == kStageSteps) {
      v8h a[kStageSteps], b[kStageSteps];
#pragma unroll
      for (int kk = 0; kk < kStageSteps; ++kk) {
        a[kk] = *reinterpret_cast<const v8h *>(wt + 32 * kk);
        b[kk] = *reinterpret_cast<const v8h *>(xt + 32 * kk);
      }
      if (s + kRingStages < stages) {
        __builtin_amdgcn_s_waitcnt(kLdsReadsDone);
        __builtin_amdgcn_s_barrier();  // the stage's slot is free: every wave's fragments are in registers
        issue_stage(s + kRingStages);
      }
      __builtin_amdgcn_sched_barrier(0);  // (left alone, the scheduler sinks every read to its MFMA)
#pragma unroll
      for (int kk = 0; kk < kStageSteps; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk], b[kk], acc, 0, 0, 0);
    } else {
      // the last stage of a K_pad that is no multiple of 128: nothing is left to request
      for (int kk = 0; kk < steps; ++kk)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const v8h *>(wt + 32 * kk), *reinterpret_cast<const v8h *>(xt + 32 * kk), acc, 0, 0, 0);
    }
  }
  // every load has landed (the last stage waited for all of them)

  // epilogue.  D[node][frame]: column lane & 31 is the frame, register 4 q + t the node 8 q + 4 (lane >> 5) + t of the wave's tile
  float *es = reinterpret_cast<float *>(ring);  // kExp only
  if (ACT == kExp) __syncthreads();             // ... once every wave has read its last fragments: the ring is dead
  const int frow = wm * 32 + (lane & 31), frame = f0 + frow;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int col = wn * 32 + 8 * q + 4 * (lane >> 5), node = nb + col;  // a multiple of 4
    const v4f bias = *reinterpret_cast<const v4f *>(p.bias + node);
    v4h h;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float z = acc[4 * q + t] + bias[t];
      if (TAP && frame < p.n && node + t < p.rows) p.tap[static_cast<size_t>(frame) * p.rows + node + t] = z;
      if (ACT == kSigmoid) {
        const float e = __builtin_amdgcn_exp2f(z * -kLog2e);
        const float d = 1.0f + e;
        const float sg = 1.0f / d;
        h[t] = static_cast<_Float16>(node + t < p.rows ? sg : 0.0f);
      } else {
        es[frow * kEStride + col + t] = node + t < p.rows ? __builtin_amdgcn_exp2f(z * kLog2e) : 0.0f;
      }
    }
    if (ACT == kSigmoid && frame < p.n && node < p.ldo) *reinterpret_cast<v4h *>(p.act + static_cast<size_t>(frame) * p.ldo + node) = h;
  }
  if (ACT == kExp) {
    __syncthreads();
    const int node = nb + lane;
    if (node < p.rows)
      for (int fr = wave; fr < frames; fr += 4) p.e[static_cast<size_t>(f0 + fr) * p.rows + node] = es[fr * kEStride + lane];
    if (wave == 0 && lane < frames) {
      // lane = frame: the workgroup's 64 nodes are one partial; 32 + 32 sequential additions, then the halves (softmax_ref: DEPTH)
      const float *row = es + lane * kEStride;
      float h0 = 0.0f, h1 = 0.0f;
#pragma unroll
      for (int c = 0; c < 32; ++c) h0 += row[c];
#pragma unroll
      for (int c = 0; c < 32; ++c) h1 += row[32 + c];
      p.partial[static_cast<size_t>(nb / kPartialNodes) * p.partial_ld + f0 + lane] = h0 + h1;
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int ACT, bool TAP>
void launch_one(const GemmParams &p, hipStream_t s) {
  auto kernel = hmid_kernel<ACT, TAP>;
  static std::atomic<unsigned long long> attr_set{0};  // dynamic LDS above 64 KB: once per device
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMidLds);
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  unsigned gx, gy;
  mid_grid(p.n, p.rows_pad, &gx, &gy);
  hipLaunchKernelGGL(kernel, dim3(gx, gy), dim3(256), kMidLds, s, p);
}

}  // namespace

void launch_hmid(const GemmParams &p, Act act, ihipStream_t *s) {
  if (p.n <= 0) return;
  const bool tap = p.tap != nullptr;
  g_mid_launches.bump((tap ? 2 : 0) + (act == kExp ? 1 : 0));
  if (act == kSigmoid && !tap) launch_one<kSigmoid, false>(p, s);
  else if (act == kSigmoid) launch_one<kSigmoid, true>(p, s);
  else if (!tap) launch_one<kExp, false>(p, s);
  else launch_one<kExp, true>(p, s);
}

void mid_launch_counts(unsigned long long out[kMidLaunchKinds]) { g_mid_launches.read(out); }

}  // namespace hf
}  // namespace fdnn
