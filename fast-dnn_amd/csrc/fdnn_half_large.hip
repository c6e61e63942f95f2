// fdnn_half_large.hip -- the half net's LARGE-BATCH GEMM: calls of large_setting frames and more (hf::large_applies), the
// bytes of hgemm_kernel (fdnn_half.hip).  Contract: fdnn_half.hpp; DESIGN section 36.
//
//   hlarge_kernel<ACT, TAP>  act(X[m][K] . W[rows][K]^T + bias) for any m >= 1.  hgemm_kernel's 256 x 128 tile gives a 2048-wide
//                            layer over a 4096-frame chunk ONE workgroup per CU in one round, and its time is that workgroup's
//                            64 k-steps: the operands are requested one 32-k step ahead, through staging registers, so the
//                            global-load latency shows at every step and no second workgroup hides it.  This kernel keeps the
//                            tile (its operand reuse is what the large sizes need) and puts a DEEP RING behind it: stages of
//                            64 k, requested 128 k ahead, straight from global memory into LDS.
//   work split               hgemm_kernel's: a workgroup of 256 threads takes 256 frames x 128 nodes, the waves 2 x 2 (wm = wave
//                            >> 1 the frame half, wn = wave & 1 the node half), each 128 frames x 64 nodes = 4 x 2 tiles of
//                            32 x 32 in 128 accumulator registers.  The grid is hf::gemm_grid's.
//   same bytes               the instruction (v_mfma_f32_32x32x16_f16), the operand roles (A = 32 nodes of W, B = 32 frames of
//                            X), the lane's k (16 kk + 8 (lane >> 5) + 0 .. 7), kk ascending in ONE chain per output from +0,
//                            exactly K_pad / 16 steps (a step past K_pad would add +0 products: an s = -0 would turn +0), the
//                            bias in the epilogue, the epilogue's fp32 sequences and v_cvt_f16_f32: all hgemm_kernel's.  No
//                            split-K, no atomics, no inline assembly.
//   the ring                 LDS is a ring of kRingStages = 3 STAGES of 64 k; a stage is the W tile (128 nodes) and the X
//                            tile (256 frames), rows of 128 bytes: three TILES of 128 rows, [W | X frames 0 .. 127 | X frames
//                            128 .. 255].  Every tile is loaded by direct global-to-LDS loads (buffer_load_dwordx4 .. lds):
//                            no register holds ring data (hgemm_kernel stages through 24).  Before stage s's MFMAs are issued
//                            every wave has requested stage s + 2, into the slot that stage s - 1 left: the loads run 128 k
//                            ahead of the MFMAs, four times hgemm_kernel's distance, with one barrier per 64 k instead of one
//                            per 32 k.  3 x 49 920 = 149 760 bytes of the CU's 160 KB, dynamic: one workgroup per CU, which
//                            is what the tile gives a 2048-wide layer at 4096 frames anyway.
//   LDS image                a direct load writes the wave's 64 x 16 bytes CONTIGUOUSLY.  A row of a stage is 64 k = 128 bytes
//                            = 8 slots of 16 bytes, so one load is a PIECE of EIGHT rows: rows r, r + 16, .., r + 112 of the
//                            tile (r = 0 .. 15), lane l taking slot l & 7 of row r + 16 (l >> 3): a global read of eight
//                            128-byte runs.  Pieces are 1040 bytes = 65 slots apart (one slot of padding): row r of a tile is
//                            at slot 65 (r & 15) + 8 (r >> 4) + c.  A fragment read takes the SAME slot c of 32 consecutive
//                            rows per half wave, and the LDS serves a b128 read in groups of 16 consecutive lanes = 16
//                            consecutive rows, all with the same r >> 4 (the LDS has 64 banks x 4 bytes = 16 slots): 65 r mod
//                            16 = r mod 16 is a permutation of the 16 rows, so the group falls on 16 distinct slots -- no
//                            conflict, against the 8-way one of rows 128 bytes apart.  The eight rows of ONE piece share
//                            their slot mod 8, which is why they are rows of eight DIFFERENT groups of 16.  A fragment is
//                            ONE ds_read_b128 at a constant offset (256 per 32 rows, 32 per kk) from the lane's base.  A
//                            tile is 16 pieces = 16 640 bytes.
//   pads                     a lane whose frame is >= m, or whose k is >= K_pad (the second half of the last stage where
//                            K_pad is no multiple of 64), carries an offset past its buffer descriptor's extent: it reads
//                            nothing from memory and the load writes zeros.  The X descriptor begins at the workgroup's first
//                            frame and ends with its last one's column K_pad.  Every wave issues every load (12 per wave and
//                            stage: pieces 4 wave .. 4 wave + 3 of each of the three tiles), so a wave's count of outstanding
//                            loads tells it which stages have landed, oldest first.
//   schedule                 per stage s: wait until the wave's own loads of stage s have landed (at most the 12 of stage s + 1
//                            outstanding) and its own fragment reads are done; barrier -- every wave's share of stage s is in
//                            LDS and every wave is done with stage s - 1; the fragment reads of the stage's first step;
//                            request stage s + 2 into stage s - 1's slot; then the stage's four steps (two in the last stage
//                            of a K_pad that is no multiple of 64; K_pad is a multiple of 32), the fragment reads of step
//                            kk + 1 issued in front of the MFMAs of step kk: at one wave per SIMD nothing else hides an LDS
//                            read.
//   paper ratio              hgemm_kernel's: per 16 k a wave reads 4 + 2 fragments = 6 KB for 8 MFMAs of 32 cycles; four waves
//                            are 24 KB = 192 clocks of the LDS's 128 bytes / clock against 256 MFMA clocks per SIMD: 0.75.
//   epilogue                 hgemm_kernel's, line for line.  D[node][frame]: sigmoid: four consecutive nodes per lane leave as
//                            one 8-byte store; pad columns [rows, ldo) are written +0.  exp: 32 frames at a time a wave's e
//                            [32 frames][64 nodes] goes through the dead ring (rows 65 floats apart), leaves as 256-byte runs,
//                            and lane = frame adds the 64-node partial, 32 + 32 sequential additions, then the halves
//                            (softmax_ref: DEPTH).  The tap forms also store z.
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

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

LaunchCounts<kLargeLaunchKinds> g_large_launches;

constexpr int kStageK = 64;                                    // k per stage: a tile row is 128 bytes
constexpr int kStageSteps = kStageK / 16;                      // MFMA steps per full stage
constexpr int kTileRows = 128;                                 // rows per tile: W, X frames 0 .. 127, X frames 128 .. 255
constexpr int kPieceStride = 1040;                             // bytes between pieces: 65 slots
constexpr int kTileBytes = 16 * kPieceStride;                  // 128 rows x 64 k and 16 slots of padding
constexpr int kStageBytes = 3 * kTileBytes;                    // [W | X lo | X hi]: 49 920
constexpr int kRingStages = 3;
constexpr int kLargeLds = kRingStages * kStageBytes;           // 149 760
constexpr int kLoadsPerStage = 12;                             // per wave: 3 tiles x 16 pieces over four waves
constexpr int kEStride = 65;                                   // output epilogue: a wave's e [32 frames][64 nodes], rows 65 floats apart
[[maybe_unused]] constexpr int kNoRead = static_cast<int>(0x80000000u);  // an offset past every descriptor's extent
static_assert(kFrameTile == 2 * kTileRows && kNodeTile == kTileRows, "hlarge_kernel is written for 256 x 128");
static_assert(kKStep * 2 == kStageK, "K_pad is a multiple of half a stage: the last stage is whole or half");
static_assert(kLargeLds <= 160 * 1024, "one workgroup owns a CU's LDS");
static_assert(kLoadsPerStage < 64, "the outstanding-load counter has 6 bits");
static_assert(4 * 32 * kEStride * 4 <= kLargeLds, "the output epilogue's e tiles reuse the ring");
static_assert(kPieceStride % 16 == 0 && (kPieceStride / 16) % 2 == 1, "pieces an odd number of 16-byte slots apart");

// s_waitcnt (gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt in 6:4, lgkmcnt in 11:8): at most c loads outstanding AND every
// LDS read done, expcnt left at its maximum
[[maybe_unused]] constexpr int wait_imm(int c) { return (c & 15) | ((c >> 4) << 14) | 0x0070; }

template <int ACT, bool TAP>
__global__ __launch_bounds__(256, 1) void hlarge_kernel(GemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char ring[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;  // the wave's 128 frames and 64 nodes inside the tile
  const int f0 = blockIdx.x * kFrameTile, nb = blockIdx.y * kNodeTile;
  const int frames = min(kFrameTile, p.n - f0);  // >= 1 by the grid
  const int stages = (p.K_pad + kStageK - 1) / kStageK;

  // the workgroup's rows of W, and its rows of X up to the last column read
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(p.w + static_cast<size_t>(nb) * p.K_pad), 0,
                                                                          kNodeTile * p.K_pad * 2, 0x00020000);  // nb + 128 <= rows_pad
  const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(p.a + static_cast<size_t>(f0) * p.lda), 0,
                                                                          ((frames - 1) * p.lda + p.K_pad) * 2, 0x00020000);

  // lane l of a piece: slot l & 7 of row piece + 16 (l >> 3).  An offset with its top bit set lies past every extent; the bit is
  // put there by arithmetic (the sign of frames - 1 - row, of K_pad - 1 - k), so a load stays ONE instruction whatever its lanes
  // hold and the count of outstanding loads stays 12 per stage
  const int lrow = 16 * (lane >> 3), lk = 8 * (lane & 7);
  auto issue_stage = [&](int st, int slot) {
    const int k = st * kStageK + lk;
    const int kpast = (p.K_pad - 1 - k) & kNoRead;
    char *dst = ring + slot * kStageBytes + wave * 4 * kPieceStride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wave * 4 + i + lrow;
      const int voff = ((row * p.K_pad + k) * 2) | kpast;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, FDNN_LDS_PTR(dst + i * kPieceStride), 16, voff, 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = t * kTileRows + wave * 4 + i + lrow;
        const int voff = ((row * p.lda + k) * 2) | kpast | ((frames - 1 - row) & kNoRead);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, FDNN_LDS_PTR(dst + (1 + t) * kTileBytes + i * kPieceStride), 16, voff, 0, 0, 0);
      }
  };

  v16f acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  issue_stage(0, 0);
  if (stages > 1) issue_stage(1, 1);

  // row lane & 31 of a group of 32 rows of a tile (256 bytes per group), k = 8 (lane >> 5) .. + 7 of an MFMA's 16
  const int frag = (lane & 15) * kPieceStride + ((lane >> 4) & 1) * 128 + 16 * (lane >> 5);
  int slot = 0;  // s mod 3
  // stage s in STEPS MFMA steps: kStageSteps, or half of them in the last stage of a K_pad that is no multiple of 64 -- never a
  // step on the zeros behind them
  auto run_stage = [&](int s, auto steps) {
    constexpr int STEPS = decltype(steps)::value;
    if (s + 1 < stages) __builtin_amdgcn_s_waitcnt(wait_imm(kLoadsPerStage));  // stage s + 1 may be on its way
    else __builtin_amdgcn_s_waitcnt(wait_imm(0));
    __builtin_amdgcn_s_barrier();  // every wave's share of stage s has landed, and every wave has read stage s - 1 out
    const char *wt = ring + slot * kStageBytes + 512 * wn + frag;               // the wave's 64 nodes: two groups of 32
    const char *xt = ring + slot * kStageBytes + (1 + wm) * kTileBytes + frag;  // the wave's 128 frames: one tile
    v8h a[2][2], b[2][4];  // the fragments of two steps: one under the MFMAs, one on its way
    auto read_step = [&](int buf, int kk) {
      a[buf][0] = *reinterpret_cast<const v8h *>(wt + 32 * kk);
      a[buf][1] = *reinterpret_cast<const v8h *>(wt + 256 + 32 * kk);
#pragma unroll
      for (int i = 0; i < 4; ++i) b[buf][i] = *reinterpret_cast<const v8h *>(xt + 256 * i + 32 * kk);
    };
    read_step(0, 0);
    const int next = slot == 0 ? kRingStages - 1 : slot - 1;  // (s + 2) mod 3: the slot of stage s - 1
    if (s + 2 < stages) issue_stage(s + 2, next);
#pragma unroll
    for (int kk = 0; kk < STEPS; ++kk) {
      if (kk + 1 < STEPS) read_step((kk + 1) & 1, kk + 1);
      __builtin_amdgcn_sched_barrier(0);  // (left alone, the scheduler sinks every read to its MFMA)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk & 1][0], b[kk & 1][i], acc[i][0], 0, 0, 0);
        acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk & 1][1], b[kk & 1][i], acc[i][1], 0, 0, 0);
      }
    }
    slot = slot + 1 == kRingStages ? 0 : slot + 1;
  };
  const int whole = p.K_pad / kStageK;
  for (int s = 0; s < whole; ++s) run_stage(s, std::integral_constant<int, kStageSteps>{});
  if (whole < stages) run_stage(whole, std::integral_constant<int, kStageSteps / 2>{});
  // every load has landed (the last stage waited for all of them)

  // epilogue.  D[node][frame]: column lane & 31 is the frame, register 4 q + t the node 8 q + 4 (lane >> 5) + t of the tile
  float *es = reinterpret_cast<float *>(ring) + wave * 32 * kEStride;  // kExp only
  if (ACT == kExp) __syncthreads();                                    // ... once every wave has read its last fragments: the ring is dead
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int frame = f0 + wm * 128 + i * 32 + (lane & 31);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = j * 32 + 8 * q + 4 * (lane >> 5), node = nb + wn * 64 + col;  // a multiple of 4
        const v4f bias = *reinterpret_cast<const v4f *>(p.bias + node);
        v4h h;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float z = acc[i][j][4 * q + t] + bias[t];
          if (TAP && frame < p.n && node + t < p.rows) p.tap[static_cast<size_t>(frame) * p.rows + node + t] = z;
          if (ACT == kSigmoid) {
            const float e = __builtin_amdgcn_exp2f(z * -kLog2e);
            const float d = 1.0f + e;
            const float sg = 1.0f / d;
            h[t] = static_cast<_Float16>(node + t < p.rows ? sg : 0.0f);
          } else {
            es[(lane & 31) * kEStride + col + t] = node + t < p.rows ? __builtin_amdgcn_exp2f(z * kLog2e) : 0.0f;
          }
        }
        if (ACT == kSigmoid && frame < p.n && node < p.ldo) *reinterpret_cast<v4h *>(p.act + static_cast<size_t>(frame) * p.ldo + node) = h;
      }
    if (ACT == kExp) {
      __syncthreads();
      const int fbase = f0 + wm * 128 + i * 32, node = nb + wn * 64 + lane;
      if (node < p.rows)
        for (int fr = 0; fr < 32 && fbase + fr < p.n; ++fr) p.e[static_cast<size_t>(fbase + fr) * p.rows + node] = es[fr * kEStride + lane];
      if (lane < 32 && fbase + lane < p.n) {
        // lane = frame: the wave's 64 nodes are one partial; 32 + 32 sequential additions, then the halves (softmax_ref: DEPTH)
        const float *row = es + lane * kEStride;
        float h0 = 0.0f, h1 = 0.0f;
#pragma unroll
        for (int c = 0; c < 32; ++c) h0 += row[c];
#pragma unroll
        for (int c = 0; c < 32; ++c) h1 += row[32 + c];
        p.partial[static_cast<size_t>((nb + wn * 64) / kPartialNodes) * p.partial_ld + fbase + lane] = h0 + h1;
      }
      __syncthreads();  // before the next 32 frames overwrite the tile
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int ACT, bool TAP>
void launch_one(const GemmParams &p, hipStream_t s) {
  auto kernel = hlarge_kernel<ACT, TAP>;
  static std::atomic<unsigned long long> attr_set{0};  // dynamic LDS above 64 KB: once per device
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLargeLds);
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  unsigned gx, gy;
  gemm_grid(p.n, p.rows_pad, &gx, &gy);
  hipLaunchKernelGGL(kernel, dim3(gx, gy), dim3(256), kLargeLds, s, p);
}

}  // namespace

void launch_hlarge(const GemmParams &p, Act act, ihipStream_t *s) {
  if (p.n <= 0) return;
  const bool tap = p.tap != nullptr;
  g_large_launches.bump((tap ? 2 : 0) + (act == kExp ? 1 : 0));
  if (act == kSigmoid && !tap) launch_one<kSigmoid, false>(p, s);
  else if (act == kSigmoid) launch_one<kSigmoid, true>(p, s);
  else if (!tap) launch_one<kExp, false>(p, s);
  else launch_one<kExp, true>(p, s);
}

void large_launch_counts(unsigned long long out[kLargeLaunchKinds]) { g_large_launches.read(out); }

}  // namespace hf
}  // namespace fdnn
