// fdnn_half.hip -- the HALF-PRECISION net on the device: fp16 weights and activations on v_mfma_f32_32x32x16_f16, fp32 sums,
// fp32 sigmoid and soft-max.  Contract and layout: fdnn_half.hpp; C-ABI: fdnn_half_api.cpp; DESIGN section 32.
//
//   hgemm_kernel<ACT, TAP>   act(X[n][K] . W[rows][K]^T + bias): 256 frames x 128 nodes x 32 k per 256-thread workgroup, the
//                            waves 2 x 2, each 128 frames x 64 nodes = 4 x 2 tiles of 32 x 32 in 128 accumulator registers.
//   operands                 the instruction's A is the W fragment (32 nodes), its B the X fragment (32 frames), so
//                            D[node][frame]: a lane holds ONE frame (lane & 31) and, in registers 4 q .. 4 q + 3, the four
//                            CONSECUTIVE nodes 8 q + 4 (lane >> 5) + 0 .. 3: a sigmoid's four halves leave as one 8-byte store.
//                            A lane's operand is 8 consecutive k of one row, k = 8 (lane >> 5) + 0 .. 7: with k contiguous in
//                            LDS that is ONE 16-byte read (ds_read_b128) per lane and fragment.
//   LDS image                a row of a stage is 32 halves = 64 bytes = four 16-byte slots; rows are 80 bytes apart (40
//                            halves: one slot of padding).  A fragment read takes the SAME slot c of 32 consecutive rows
//                            per half wave, byte address 80 r + 16 c: in units of 16 bytes 5 r + c.  The LDS serves a
//                            b128 read in groups of lanes that together fill its 64 banks x 4 bytes = 16 slots (or 8 slots
//                            where a group is 8 lanes); 5 is odd, so 5 r mod 16 is a permutation of any 16 consecutive r
//                            (and 5 r mod 8 of any 8): every group of consecutive lanes falls on distinct slots, no
//                            conflict -- against the 4-way one of rows 64 bytes apart (4 r + c mod 16 repeats every 4 rows).
//                            The staging stores (16 bytes per thread, four threads to a row) are two-way at worst.
//   wave tile                per k-step of 32 a wave issues 4 x 2 x 2 = 16 MFMAs of 32 cycles (8 passes): 512 cycles on its
//                            SIMD.  It reads (4 + 2) fragments x 2 = 12 KB, the four waves 48 KB: 384 cycles of the LDS's
//                            128 bytes / clock.  0.75: the k-loop is bound by MFMA issue.  (2 x 2 tiles per wave would be 8
//                            MFMAs = 256 cycles against 32 KB = 256 cycles: the LDS saturated.)
//   staging                  two stages in LDS (2 x 30 KB): step s + 1's global loads (6 x 16 bytes per thread) are issued
//                            before step s's MFMAs and stored to the other stage after them; one barrier per k-step.  At 60 KB
//                            and <= 256 registers two workgroups share a CU, so one's barrier hides under the other's MFMAs.
//   k order                  k-steps ascend, the two MFMAs of a step in order, ONE accumulator chain per output, starting at
//                            +0; the bias is added in the epilogue, a rounding of its own.  No split-K.
//   epilogue                 sigmoid: the float kernel's fp32 sequence, then v_cvt_f16_f32 (round to nearest even), four
//                            halves per store; pad columns [rows, ldo) are written +0.  exp: 32 frames at a time, a wave's
//                            e [32 frames][64 nodes] goes through the dead operand LDS (rows 65 floats apart): out of it the
//                            rows leave as 256-byte runs and lane = frame adds the 64-node partial, 32 + 32 sequential
//                            additions and the halves (softmax_ref: DEPTH).  The tap forms also store z.
//   pads                     pad frames are neither read nor written; pad nodes contribute e = 0.
#include <hip/hip_runtime.h>

#include "fdnn_act.hpp"  // kLog2e
#include "fdnn_half.hpp"
#include "fdnn_launch.hpp"

namespace fdnn {
namespace hf {
namespace {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef _Float16 v4h __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

LaunchCounts<kLaunchKinds> g_half_launches;

constexpr int kLdsStride = kKStep + 8;                                // halves between rows of an operand tile in LDS: 80 bytes
constexpr int kXHalves = kFrameTile * kLdsStride;                     // the frame tile of one stage
constexpr int kStageHalves = (kFrameTile + kNodeTile) * kLdsStride;   // [X | W]
constexpr int kEStride = 65;                                          // output epilogue: a wave's e [32 frames][64 nodes], rows 65 apart
static_assert(kFrameTile == 256 && kNodeTile == 128 && kKStep == 32, "hgemm_kernel is written for 256 x 128 x 32");
static_assert(kLdsStride * 2 % 16 == 0, "a fragment is one aligned 16-byte read");
static_assert(4 * 32 * kEStride * 4 <= 2 * kStageHalves * 2, "the output epilogue's e tiles reuse the operand stages");
static_assert(2 * kStageHalves * 2 <= 65536, "static LDS");

template <int ACT, bool TAP>
__global__ __launch_bounds__(256, 2) void hgemm_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * kStageHalves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;  // the wave's 128 frames and 64 nodes inside the tile
  const int f0 = blockIdx.x * kFrameTile, nb = blockIdx.y * kNodeTile;
  const int steps = p.K_pad / kKStep;

  // staging: the frame tile is 256 rows x 4 slots of 8 k (thread t takes slots t + 256 i, i < 4), the node tile 128 x 4 (i < 2)
  uint4 rx[4], rw0, rw1;
  auto load_global = [&](int step) {
    const int k0 = step * kKStep;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + 256 * i, row = idx >> 2, c = idx & 3;
      rx[i] = f0 + row < p.n ? *reinterpret_cast<const uint4 *>(p.a + static_cast<size_t>(f0 + row) * p.lda + k0 + 8 * c) : make_uint4(0u, 0u, 0u, 0u);
    }
    const uint16_t *w = p.w + static_cast<size_t>(nb + (tid >> 2)) * p.K_pad + k0 + 8 * (tid & 3);  // nb + row < rows_pad
    rw0 = *reinterpret_cast<const uint4 *>(w);
    rw1 = *reinterpret_cast<const uint4 *>(w + static_cast<size_t>(64) * p.K_pad);
  };
  auto store_lds = [&](int buf) {
    uint16_t *xs = lds + buf * kStageHalves, *ws = xs + kXHalves;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<uint4 *>(xs + (idx >> 2) * kLdsStride + 8 * (idx & 3)) = rx[i];
    }
    *reinterpret_cast<uint4 *>(ws + (tid >> 2) * kLdsStride + 8 * (tid & 3)) = rw0;
    *reinterpret_cast<uint4 *>(ws + (64 + (tid >> 2)) * kLdsStride + 8 * (tid & 3)) = rw1;
  };

  v16f acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  load_global(0);
  store_lds(0);
  __syncthreads();
  const int frag = (lane & 31) * kLdsStride + 8 * (lane >> 5);  // row lane & 31, k = 8 (lane >> 5) .. + 7 of an MFMA's 16
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) load_global(s + 1);
    const uint16_t *xs = lds + (s & 1) * kStageHalves + (wm * 128) * kLdsStride + frag;
    const uint16_t *ws = lds + (s & 1) * kStageHalves + kXHalves + (wn * 64) * kLdsStride + frag;
#pragma unroll
    for (int kk = 0; kk < kKStep / 16; ++kk) {
      const v8h a0 = *reinterpret_cast<const v8h *>(ws + 16 * kk), a1 = *reinterpret_cast<const v8h *>(ws + 32 * kLdsStride + 16 * kk);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const v8h b = *reinterpret_cast<const v8h *>(xs + i * 32 * kLdsStride + 16 * kk);
        acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b, acc[i][0], 0, 0, 0);
        acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b, acc[i][1], 0, 0, 0);
      }
    }
    if (s + 1 < steps) store_lds((s + 1) & 1);  // the stage step s - 1 read: every wave is past the barrier that ended it
    __syncthreads();
  }

  // epilogue.  D[node][frame]: column lane & 31 is the frame, register 4 q + t the node 8 q + 4 (lane >> 5) + t of the tile
  float *es = reinterpret_cast<float *>(lds) + wave * 32 * kEStride;  // kExp only; the operand stages are dead
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
}

__global__ __launch_bounds__(256) void half_input_step_kernel(const float *x, const float *shift, const float *scale, uint16_t *xs, float *lin,
                                                              int n, int dim, int ld) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<size_t>(n) * ld) return;
  const int f = static_cast<int>(i / ld), k = static_cast<int>(i % ld);
  float v = 0.0f;
  if (k < dim) {
    const float t = x[static_cast<size_t>(f) * dim + k] + shift[k];  // the float net's two roundings
    if (lin) lin[static_cast<size_t>(f) * dim + k] = t;
    v = t * scale[k];
  }
  xs[i] = half_bits(v);  // the third, in integer arithmetic: a conversion would fuse with the product (fdnn_half.hpp)
}

}  // namespace

void launch_hgemm(const GemmParams &p, Act act, ihipStream_t *s) {
  if (p.n <= 0) return;
  unsigned gx, gy;
  gemm_grid(p.n, p.rows_pad, &gx, &gy);
  const dim3 grid(gx, gy), block(256);
  const bool tap = p.tap != nullptr;
  g_half_launches.bump((tap ? 2 : 0) + (act == kExp ? 1 : 0));
  if (act == kSigmoid && !tap) hipLaunchKernelGGL((hgemm_kernel<kSigmoid, false>), grid, block, 0, s, p);
  else if (act == kSigmoid) hipLaunchKernelGGL((hgemm_kernel<kSigmoid, true>), grid, block, 0, s, p);
  else if (!tap) hipLaunchKernelGGL((hgemm_kernel<kExp, false>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((hgemm_kernel<kExp, true>), grid, block, 0, s, p);
}

void launch_half_input_step(const float *x, const float *shift, const float *scale, uint16_t *xs, float *lin, int n, int dim, int ld,
                            ihipStream_t *s) {
  if (n <= 0) return;
  g_half_launches.bump(4);
  const size_t total = static_cast<size_t>(n) * ld;
  hipLaunchKernelGGL(half_input_step_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, x, shift, scale, xs,
                     lin, n, dim, ld);
}

void launch_counts(unsigned long long out[kLaunchKinds]) { g_half_launches.read(out); }

}  // namespace hf
}  // namespace fdnn
