// fdnn_half_small.hip -- the half net's SMALL-BATCH GEMM: calls of 1 .. 128 frames (hf::small_applies), the bytes of
// hgemm_kernel (fdnn_half.hip).  Contract: fdnn_half.hpp; DESIGN section 33.
//
//   hsmall_kernel<ACT, TAP, NT, FT>  act(X[n][K] . W[rows][K]^T + bias) for n <= 128.  A call this small is one pass over the layer's
//                            weights: the MFMAs of 32 frames x 32 nodes x 2048 k are 128 instructions, the weights behind them
//                            128 KB.  So the kernel is built around BYTES IN FLIGHT, not MFMA issue.
//   work split               a workgroup of 256 threads takes 32 NT nodes (NT = 1 or 2) and ALL the call's frames: FT = 1 .. 4
//                            frame tiles of 32.  The grid is (rows_pad / (32 NT)).  Waves 0 .. NT - 1 COMPUTE, one 32-node
//                            tile each against every frame tile (FT accumulators of 16 registers: a W fragment is read once
//                            and used FT times); ALL four waves STAGE.  With 149 760 bytes of LDS a CU holds one workgroup,
//                            one wave per SIMD: a wave may use all 512 registers, so a staging wave costs the compute wave
//                            nothing (the kernel's count and occupancy: profiles/kernel_resources_half_small.txt).
//   same bytes               the instruction (v_mfma_f32_32x32x16_f16), the operand roles (A = 32 nodes of W, B = 32 frames of
//                            X), the lane's k (16 kk + 8 (lane >> 5) + 0 .. 7), kk ascending in ONE chain per output from +0,
//                            the bias in the epilogue, the epilogue's fp32 sequences: all hgemm_kernel's.  No split-K.
//   the ring                 LDS is a ring of kRingTiles = 9 TILES; a tile is 32 rows (nodes of W or frames of X) x 256 k.  A
//                            k-stage of 256 is NT + FT tiles in the order W .. X ..; the tiles of all stages form one stream
//                            and tile t lives in slot t mod 9.  The ring is always full: at FT = 1, NT = 1 that is 4.5 stages
//                            = 74 KB of weights and 74 KB of frames requested ahead of the MFMAs, at FT = 4, NT = 2 one and
//                            a half stages.  Every tile is loaded by direct global-to-LDS loads (buffer_load_dwordx4 .. lds):
//                            no register holds ring data.
//   LDS image                a direct load writes the wave's 64 x 16 bytes CONTIGUOUSLY.  One load is a PIECE: rows r and
//                            r + 16 of the tile (r = 0 .. 15), 256 k = 512 bytes = 32 slots of 16 bytes each, lane l taking slot
//                            l & 31 of row r + 16 (l >> 5): a global read of two 512-byte runs.  Pieces are 1040 bytes = 65
//                            slots apart (one slot of padding).  A fragment read takes the SAME slot c of 32 consecutive
//                            rows per half wave: row r of the tile is at slot 65 (r & 15) + 32 (r >> 4) + c.  The LDS serves
//                            a b128 read in groups of 16 consecutive lanes = 16 consecutive rows, all with the same r >> 4:
//                            65 r mod 16 = r mod 16 (65 is odd, here 1 mod 16) is a permutation of the 16 rows, so the
//                            group falls on 16 distinct slots -- no conflict, as with hgemm_kernel's 5 r + c, against the
//                            16-way one of rows 512 bytes apart.  A fragment stays ONE ds_read_b128.
//   pads                     a lane whose frame is >= n, or whose k is >= K_pad (the last stage of a K_pad that is no multiple
//                            of 256), carries an offset past its buffer descriptor's extent: it reads nothing from memory
//                            and the load writes zeros.  Every wave issues every load, so a wave's count of outstanding loads
//                            tells it which tiles have landed (4 loads per wave and tile, oldest first).
//   schedule                 per stage: wait until the wave's own loads of the stage's tiles have landed, barrier, the
//                            compute waves' MFMAs (up to 16 per frame tile), barrier, every wave refills the NT + FT freed
//                            slots.  Two barriers per 256 k.
//   epilogue                 D[node][frame] as in hgemm_kernel.  sigmoid: four consecutive nodes per lane leave as one 8-byte
//                            store; pad columns [rows, ldo) are written +0.  exp (NT = 2): the workgroup's e [32 frames][64
//                            nodes] goes through the dead ring, rows 65 floats apart; the four waves send the rows out as
//                            256-byte runs and lane = frame of wave 0 adds the 64-node partial, 32 + 32 sequential additions,
//                            then the halves (softmax_ref: DEPTH).  The tap forms also store z.
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

LaunchCounts<kSmallLaunchKinds> g_small_launches;

[[maybe_unused]] constexpr int kStageK = 256;                                 // k per stage: a tile row is 512 bytes
constexpr int kPieceStride = 1040;                            // bytes between pieces: 65 slots
constexpr int kTileBytes = 16 * kPieceStride;                 // 32 rows x 256 k and 16 slots of padding
#ifndef FDNN_HSMALL_RING_TILES
#define FDNN_HSMALL_RING_TILES 9  // (a build switch for the measurement of section 33 only)
#endif
constexpr int kRingTiles = FDNN_HSMALL_RING_TILES;
constexpr int kSmallLds = kRingTiles * kTileBytes;            // 149 760
constexpr int kLoadsPerTile = 4;                              // per wave: 16 pieces over four waves
constexpr int kEStride = 65;                                  // output epilogue: e [32 frames][64 nodes], rows 65 floats apart
[[maybe_unused]] constexpr int kNoRead = static_cast<int>(0x80000000u);        // an offset past every descriptor's extent
static_assert(kSmallLds <= 160 * 1024, "the ring exceeds the CU's LDS");
static_assert(kRingTiles >= 2 + kSmallMaxFrames / 32, "the ring holds a whole stage");
static_assert((kRingTiles - 2) * kLoadsPerTile < 64, "the outstanding-load counter has 6 bits");
static_assert(32 * kEStride * 4 <= kSmallLds, "the output epilogue's e tile reuses the ring");
static_assert(kPieceStride % 16 == 0 && (kPieceStride / 16) % 2 == 1, "pieces an odd number of 16-byte slots apart");

// s_waitcnt vmcnt(c) alone (gfx9 encoding: vmcnt in bits 3:0 and 15:14; expcnt and lgkmcnt left at their maxima)
constexpr int vmcnt_imm(int c) { return (c & 15) | ((c >> 4) << 14) | 0x0f70; }
// until at most `tiles` tiles' worth of this wave's loads are outstanding
[[maybe_unused]] __device__ __forceinline__ void wait_tiles_behind(int tiles) {
  switch (tiles) {
    case 0: __builtin_amdgcn_s_waitcnt(vmcnt_imm(0)); break;
    case 1: __builtin_amdgcn_s_waitcnt(vmcnt_imm(1 * kLoadsPerTile)); break;
    case 2: __builtin_amdgcn_s_waitcnt(vmcnt_imm(2 * kLoadsPerTile)); break;
    case 3: __builtin_amdgcn_s_waitcnt(vmcnt_imm(3 * kLoadsPerTile)); break;
    case 4: __builtin_amdgcn_s_waitcnt(vmcnt_imm(4 * kLoadsPerTile)); break;
    case 5: __builtin_amdgcn_s_waitcnt(vmcnt_imm(5 * kLoadsPerTile)); break;
    case 6: __builtin_amdgcn_s_waitcnt(vmcnt_imm(6 * kLoadsPerTile)); break;
    default: __builtin_amdgcn_s_waitcnt(vmcnt_imm(7 * kLoadsPerTile)); break;
  }
}

template <int ACT, bool TAP, int NT, int FT>
__global__ __launch_bounds__(256) void hsmall_kernel(GemmParams p) {
  static_assert(ACT == kSigmoid || NT == 2, "the output form owns whole 64-node groups");
  static_assert(FT >= 1 && FT <= kSmallMaxFrames / 32, "1 .. 4 frame tiles");
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char ring[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nb = blockIdx.x * 32 * NT;
  const int stages = (p.K_pad + kStageK - 1) / kStageK;
  constexpr int per = NT + FT;  // tiles per stage
  const int total = stages * per;

  // the workgroup's rows of W, and the call's rows of X up to the last column read
  const __amdgpu_buffer_rsrc_t rsrc_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(p.w + static_cast<size_t>(nb) * p.K_pad), 0, 32 * NT * p.K_pad * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_x =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(p.a), 0, ((p.n - 1) * p.lda + p.K_pad) * 2, 0x00020000);

  // the stream's next tile to request: its stage, its place in the stage, its slot
  int is = 0, ij = 0, islot = 0, issued = 0;
  const int lrow = lane >> 5, lk = 8 * (lane & 31);
  auto issue_tile = [&]() {
    const int k = is * kStageK + lk;
    const bool kin = k < p.K_pad;
    char *dst = ring + islot * kTileBytes;
#pragma unroll
    for (int i = 0; i < kLoadsPerTile; ++i) {
      const int piece = wave * kLoadsPerTile + i, row = piece + 16 * lrow;
      if (ij < NT) {
        const int voff = kin ? ((ij * 32 + row) * p.K_pad + k) * 2 : kNoRead;  // nb + ij * 32 + row < rows_pad
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, FDNN_LDS_PTR(dst + piece * kPieceStride), 16, voff, 0, 0, 0);
      } else {
        const int frame = (ij - NT) * 32 + row;
        const int voff = kin && frame < p.n ? (frame * p.lda + k) * 2 : kNoRead;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, FDNN_LDS_PTR(dst + piece * kPieceStride), 16, voff, 0, 0, 0);
      }
    }
    ++issued;
    if (++ij == per) ij = 0, ++is;
    if (++islot == kRingTiles) islot = 0;
  };

  v16f acc[FT];
#pragma unroll
  for (int i = 0; i < FT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

  while (issued < kRingTiles && issued < total) issue_tile();

  // row lane & 31 of a tile, k = 8 (lane >> 5) .. + 7 of an MFMA's 16
  const int frag = (lane & 15) * kPieceStride + ((lane >> 4) & 1) * 512 + 16 * (lane >> 5);
  int cslot = 0;  // the slot of the stage's first tile
  for (int s = 0; s < stages; ++s) {
    wait_tiles_behind(issued - (s + 1) * per);
    __builtin_amdgcn_s_barrier();  // every wave's share of the stage has landed
    if (wave < NT) {
      const int ws = cslot + wave >= kRingTiles ? cslot + wave - kRingTiles : cslot + wave;
      const char *wt = ring + ws * kTileBytes + frag;
      const char *xt[FT];
#pragma unroll
      for (int i = 0; i < FT; ++i) {
        const int xs = cslot + NT + i >= kRingTiles ? cslot + NT + i - kRingTiles : cslot + NT + i;
        xt[i] = ring + xs * kTileBytes + frag;
      }
      auto mfmas = [&](int kk) {
        const v8h a = *reinterpret_cast<const v8h *>(wt + 32 * kk);
#pragma unroll
        for (int i = 0; i < FT; ++i) {
          const v8h b = *reinterpret_cast<const v8h *>(xt[i] + 32 * kk);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[i], 0, 0, 0);
        }
      };
      const int pairs = min(p.K_pad - s * kStageK, kStageK) / 32;  // K_pad is a multiple of 32: 8 pairs of MFMAs, fewer in a last stage
      if (pairs == kStageK / 32) {
        // eight MFMA steps' fragments to registers, then their MFMAs: the LDS latency is paid twice a stage, not per step
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          v8h a[8], b[FT][8];
#pragma unroll
          for (int kk = 0; kk < 8; ++kk) {
            a[kk] = *reinterpret_cast<const v8h *>(wt + 32 * (8 * h + kk));
#pragma unroll
            for (int i = 0; i < FT; ++i) b[i][kk] = *reinterpret_cast<const v8h *>(xt[i] + 32 * (8 * h + kk));
          }
          __builtin_amdgcn_sched_barrier(0);  // (left alone, the scheduler sinks every read to its MFMA)
#pragma unroll
          for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int i = 0; i < FT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk], b[i][kk], acc[i], 0, 0, 0);
        }
      } else {
        for (int g = 0; g < pairs; ++g) mfmas(2 * g), mfmas(2 * g + 1);
      }
    }
    __builtin_amdgcn_s_barrier();  // the stage's slots are free: their fragments are in registers
    cslot = cslot + per >= kRingTiles ? cslot + per - kRingTiles : cslot + per;
    for (int j = 0; j < per && issued < total; ++j) issue_tile();
  }
  // every load has landed (the last stage waited for all of them): the ring is dead

  // epilogue.  D[node][frame]: column lane & 31 is the frame, register 4 q + t the node 8 q + 4 (lane >> 5) + t of the wave's tile
  float *es = reinterpret_cast<float *>(ring);  // kExp only
#pragma unroll
  for (int i = 0; i < FT; ++i) {
    const int frame = i * 32 + (lane & 31);
    if (wave < NT) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = wave * 32 + 8 * q + 4 * (lane >> 5), node = nb + col;  // a multiple of 4
        const v4f bias = *reinterpret_cast<const v4f *>(p.bias + node);
        v4h h;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float z = acc[i][4 * q + t] + bias[t];
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
    }
    if (ACT == kExp) {
      __syncthreads();
      const int fbase = i * 32, node = nb + lane;
      if (node < p.rows)
        for (int fr = wave; fr < 32 && fbase + fr < p.n; fr += 4) p.e[static_cast<size_t>(fbase + fr) * p.rows + node] = es[fr * kEStride + lane];
      if (wave == 0 && lane < 32 && fbase + lane < p.n) {
        // lane = frame: the workgroup's 64 nodes are one partial; 32 + 32 sequential additions, then the halves (softmax_ref: DEPTH)
        const float *row = es + lane * kEStride;
        float h0 = 0.0f, h1 = 0.0f;
#pragma unroll
        for (int c = 0; c < 32; ++c) h0 += row[c];
#pragma unroll
        for (int c = 0; c < 32; ++c) h1 += row[32 + c];
        p.partial[static_cast<size_t>(nb / kPartialNodes) * p.partial_ld + fbase + lane] = h0 + h1;
      }
      __syncthreads();  // before the next 32 frames overwrite the tile
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int ACT, bool TAP, int NT, int FT>
void launch_tiles(const GemmParams &p, hipStream_t s) {
  auto kernel = hsmall_kernel<ACT, TAP, NT, FT>;
  static std::atomic<unsigned long long> attr_set{0};  // dynamic LDS above 64 KB: once per device
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kSmallLds);
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  static_assert(NT == (ACT == kExp ? 2 : kSmallHiddenTiles), "small_grid states this kernel's node tile");
  hipLaunchKernelGGL(kernel, dim3(small_grid(p.rows_pad, static_cast<Act>(ACT))), dim3(256), kSmallLds, s, p);
}

template <int ACT, bool TAP, int NT>
void launch_one(const GemmParams &p, hipStream_t s) {
  switch (small_frame_tiles(p.n)) {
    case 1: launch_tiles<ACT, TAP, NT, 1>(p, s); break;
    case 2: launch_tiles<ACT, TAP, NT, 2>(p, s); break;
    case 3: launch_tiles<ACT, TAP, NT, 3>(p, s); break;
    default: launch_tiles<ACT, TAP, NT, 4>(p, s); break;
  }
}

}  // namespace

static_assert(kSmallHiddenTiles == 1 || kSmallHiddenTiles == 2, "a hidden workgroup owns 32 or 64 nodes");

void launch_hsmall(const GemmParams &p, Act act, ihipStream_t *s) {
  if (p.n <= 0 || p.n > kSmallMaxFrames) return;  // (run_layer asks small_applies first)
  const bool tap = p.tap != nullptr;
  g_small_launches.bump((tap ? 2 : 0) + (act == kExp ? 1 : 0));
  if (act == kSigmoid && !tap) launch_one<kSigmoid, false, kSmallHiddenTiles>(p, s);
  else if (act == kSigmoid) launch_one<kSigmoid, true, kSmallHiddenTiles>(p, s);
  else if (!tap) launch_one<kExp, false, 2>(p, s);
  else launch_one<kExp, true, 2>(p, s);
}

void small_launch_counts(unsigned long long out[kSmallLaunchKinds]) { g_small_launches.read(out); }

}  // namespace hf
}  // namespace fdnn
