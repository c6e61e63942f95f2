// fdnn_float.hip -- the UNQUANTIZED net on the device (FeedForwardNetwork.calculate, FeedForwardNetwork.java:133-148,
// :360-414) and the kernels of the quantization report (FuncTest.diff, FuncTest.java:59-74).  Contract and layout:
// fdnn_float.hpp; C-ABI: fdnn_float_api.cpp.
//
//   fgemm_kernel<ACT, TAP>   act(X[n][K] . W[rows][K]^T + bias) on v_mfma_f32_32x32x2_f32: 128 frames x 128 nodes x 32 k per
//                            256-thread workgroup, each wave 2 x 2 tiles of 32 x 32 in 64 accumulator registers, the two
//                            operand tiles double-buffered in LDS (the next k-step's global loads are in flight while
//                            this one's MFMAs run; one barrier per k-step).
//   LDS image                an MFMA operand is ONE float per lane, A[l & 31][k = l >> 5]: rows are staged row-major with
//                            the row stride PADDED to 33 floats, so the 32 rows of a fragment read fall on 32 different
//                            banks, and the k + 1 half of the wave on the same pattern shifted by one: one two-way
//                            conflict per read (lane 63 meets lane 0 on bank 0: 31 * 33 + 1 = 0 mod 64) instead of the
//                            32-way one of stride 32.  (Stores into it are scalar.)
//   k order                  k ascends through the whole K for every output: k-steps in order, the 16 MFMAs of a step in
//                            order, the two k of an MFMA in order (lanes 0-31 hold k, lanes 32-63 k + 1).  No split-K.
//                            Accumulators start at +0; the bias is added in the epilogue, a rounding of its own.
//   sigmoid                  e = exp2(RN(-z * RN32(log2 e))), d = RN(1 + e), s = 1 / d by IEEE division: the exp2 sequence of
//                            fdnn_small.hip (softmax_ref.C_E_PATH["exp2.small"]).  z <= -89 gives e = inf, s = 0; z >= 104
//                            gives e = 0, s = 1: the ends come from the arithmetic.
//   output                   e = exp2(RN(z * RN32(log2 e))), unstabilised like the reference (:404-414), and the 64-node
//                            partial sums of e: each half of 32 nodes added one after the other, the halves added -- then
//                            normalize_kernel / normalize_small_kernel (fdnn_kernels.hip) own the row total.
//   pads                     pad activations are written +0 (a sigmoid would make 0.5 of them), pad frames are neither read
//                            nor written, pad nodes contribute e = 0.
#include <hip/hip_runtime.h>

#include <climits>

#include "fdnn_act.hpp"  // kLog2e
#include "fdnn_float.hpp"
#include "fdnn_launch.hpp"

namespace fdnn {
namespace fl {
namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

LaunchCounts<kLaunchKinds> g_float_launches;

constexpr int kLdsStride = kKStep + 1;                    // floats between rows of an operand tile in LDS
constexpr int kTileFloats = kFrameTile * kLdsStride;      // one operand tile (kNodeTile == kFrameTile)
constexpr int kEStride = 65;                              // output epilogue: a wave's e [64 frames][64 nodes], rows 65 apart
static_assert(kFrameTile == 128 && kNodeTile == 128 && kKStep == 32, "fgemm_kernel is written for 128 x 128 x 32");
static_assert(4 * 64 * kEStride <= 4 * kTileFloats, "the output epilogue's e tiles reuse the operand buffers");

template <int ACT, bool TAP>
__global__ __launch_bounds__(256) void fgemm_kernel(GemmParams p) {
  __shared__ float lds[4 * kTileFloats];  // [buffer][A | W][128][33]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;  // the wave's 64 frames and 64 nodes inside the tile
  const int f0 = blockIdx.x * kFrameTile, nb = blockIdx.y * kNodeTile;
  const int steps = p.K_pad / kKStep;

  // staging: a tile is 128 rows x 8 groups of 4 k; thread t takes the groups t, t + 256, t + 512, t + 768
  float4 ra[4], rw[4];
  auto load_global = [&](int step) {
    const int k0 = step * kKStep;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + 256 * i, row = idx >> 3, c4 = idx & 7;
      ra[i] = f0 + row < p.n ? *reinterpret_cast<const float4 *>(p.a + static_cast<size_t>(f0 + row) * p.lda + k0 + 4 * c4)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
      rw[i] = *reinterpret_cast<const float4 *>(p.w + static_cast<size_t>(nb + row) * p.K_pad + k0 + 4 * c4);  // nb + row < rows_pad
    }
  };
  auto store_lds = [&](int buf) {
    float *as = lds + buf * 2 * kTileFloats, *ws = as + kTileFloats;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + 256 * i, o = (idx >> 3) * kLdsStride + 4 * (idx & 7);
      as[o] = ra[i].x, as[o + 1] = ra[i].y, as[o + 2] = ra[i].z, as[o + 3] = ra[i].w;
      ws[o] = rw[i].x, ws[o + 1] = rw[i].y, ws[o + 2] = rw[i].z, ws[o + 3] = rw[i].w;
    }
  };

  v16f acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  load_global(0);
  store_lds(0);
  __syncthreads();
  const int frag = (lane & 31) * kLdsStride + (lane >> 5);  // A[l & 31][k = l >> 5], and B[k = l >> 5][l & 31] = W[node][k]
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) load_global(s + 1);
    const float *as = lds + (s & 1) * 2 * kTileFloats + (wm * 64) * kLdsStride + frag;
    const float *ws = lds + (s & 1) * 2 * kTileFloats + kTileFloats + (wn * 64) * kLdsStride + frag;
#pragma unroll
    for (int kk = 0; kk < kKStep / 2; ++kk) {
      const float a0 = as[2 * kk], a1 = as[32 * kLdsStride + 2 * kk];
      const float b0 = ws[2 * kk], b1 = ws[32 * kLdsStride + 2 * kk];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (s + 1 < steps) store_lds((s + 1) & 1);  // the buffer step s - 1 read: every wave is past the barrier that ended it
    __syncthreads();
  }

  // epilogue.  D[i][j]: column j = lane & 31 is the node, row i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) the frame
  float *es = lds + wave * 64 * kEStride;  // kExp only; every wave is past the last step's barrier: the operand tiles are dead
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wn * 64 + j * 32 + (lane & 31), node = nb + col;
    const float bias = p.bias[node];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int fr = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), frame = f0 + wm * 64 + fr;
        const float z = acc[i][j][r] + bias;
        if (TAP && frame < p.n && node < p.rows) p.tap[static_cast<size_t>(frame) * p.rows + node] = z;
        if (ACT == kSigmoid) {
          const float e = __builtin_amdgcn_exp2f(z * -kLog2e);
          const float d = 1.0f + e;
          const float sg = 1.0f / d;
          if (frame < p.n && node < p.ldo) p.out[static_cast<size_t>(frame) * p.ldo + node] = node < p.rows ? sg : 0.0f;
        } else {
          const float e = node < p.rows ? __builtin_amdgcn_exp2f(z * kLog2e) : 0.0f;
          if (frame < p.n && node < p.rows) p.out[static_cast<size_t>(frame) * p.rows + node] = e;
          es[fr * kEStride + j * 32 + (lane & 31)] = e;
        }
      }
  }
  if (ACT == kExp) {
    __syncthreads();
    // lane = frame: the wave's 64 nodes are one partial; 32 + 32 sequential additions, then the halves (softmax_ref: DEPTH)
    const float *row = es + lane * kEStride;
    float h0 = 0.0f, h1 = 0.0f;
#pragma unroll
    for (int c = 0; c < 32; ++c) h0 += row[c];
#pragma unroll
    for (int c = 0; c < 32; ++c) h1 += row[32 + c];
    const int frame = f0 + wm * 64 + lane;
    if (frame < p.n) p.partial[static_cast<size_t>((nb + wn * 64) / kPartialNodes) * p.partial_ld + frame] = h0 + h1;
  }
}

__global__ __launch_bounds__(256) void input_step_kernel(const float *x, const float *shift, const float *scale, float *xs, float *lin,
                                                         int n, int dim, int ld) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<size_t>(n) * ld) return;
  const int f = static_cast<int>(i / ld), k = static_cast<int>(i % ld);
  float v = 0.0f;
  if (k < dim) {
    const float t = x[static_cast<size_t>(f) * dim + k] + shift[k];  // FeedForwardNetwork.java:121-128: two roundings
    if (lin) lin[static_cast<size_t>(f) * dim + k] = t;
    v = t * scale[k];
  }
  xs[i] = v;
}

// ---------------------------------------------------------------- quantization report
// One wave per row: a NaN in either matrix, else the arg max of each (first index on ties) and whether they agree.
__global__ __launch_bounds__(256) void report_rows_kernel(ReportParams p) {
  const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.n) return;
  const float *r = p.ref + static_cast<size_t>(f) * p.O, *q = p.q + static_cast<size_t>(f) * p.O;
  float br = -INFINITY, bq = -INFINITY;
  int ir = INT_MAX, iq = INT_MAX, nan = 0;
  if (lane < p.O) br = r[lane], bq = q[lane], ir = iq = lane;
  for (int c = lane; c < p.O; c += 64) {
    const float vr = r[c], vq = q[c];
    nan |= (vr != vr) || (vq != vq);
    if (vr > br) br = vr, ir = c;
    if (vq > bq) bq = vq, iq = c;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const float or_ = __shfl_xor(br, d), oq = __shfl_xor(bq, d);
    const int jr = __shfl_xor(ir, d), jq = __shfl_xor(iq, d);
    nan |= __shfl_xor(nan, d);
    if (or_ > br || (or_ == br && jr < ir)) br = or_, ir = jr;
    if (oq > bq || (oq == bq && jq < iq)) bq = oq, iq = jq;
  }
  if (lane == 0) {
    p.row_nan[f] = static_cast<unsigned char>(nan);
    atomicAdd(&p.cnt[0], 1ull);  // integers: the order of the additions does not show
    if (nan) atomicAdd(&p.cnt[1], 1ull);
    else if (ir == iq) atomicAdd(&p.cnt[2], 1ull);
  }
}

// One thread owns a node over kReportRows rows (coalesced across nodes): sum and maximum of |double(q) - double(ref)|, rows
// ascending, NaN rows left out.
__global__ __launch_bounds__(256) void report_nodes_kernel(ReportParams p) {
  const int node = blockIdx.x * 256 + threadIdx.x;
  if (node >= p.O) return;
  const int fa = blockIdx.y * kReportRows, fb = min(p.n, fa + kReportRows);
  double s = 0.0, m = 0.0;
  for (int f = fa; f < fb; ++f) {
    if (p.row_nan[f]) continue;
    const size_t i = static_cast<size_t>(f) * p.O + node;
    const double d = fabs(static_cast<double>(p.q[i]) - static_cast<double>(p.ref[i]));
    s += d;
    m = fmax(m, d);
  }
  p.blk_sum[static_cast<size_t>(blockIdx.y) * p.O + node] = s;
  p.blk_max[static_cast<size_t>(blockIdx.y) * p.O + node] = m;
}

// The block partials into the accumulators, in block order.
__global__ __launch_bounds__(256) void report_fold_kernel(ReportParams p) {
  const int node = blockIdx.x * 256 + threadIdx.x;
  if (node >= p.O) return;
  const int blocks = (p.n + kReportRows - 1) / kReportRows;
  double s = p.node_sum[node], m = p.node_max[node];
  for (int b = 0; b < blocks; ++b) {
    s += p.blk_sum[static_cast<size_t>(b) * p.O + node];
    m = fmax(m, p.blk_max[static_cast<size_t>(b) * p.O + node]);
  }
  p.node_sum[node] = s;
  p.node_max[node] = m;
}

}  // namespace

void launch_fgemm(const GemmParams &p, Act act, ihipStream_t *s) {
  if (p.n <= 0) return;
  unsigned gx, gy;
  gemm_grid(p.n, p.rows_pad, &gx, &gy);
  const dim3 grid(gx, gy), block(256);
  const bool tap = p.tap != nullptr;
  g_float_launches.bump((tap ? 2 : 0) + (act == kExp ? 1 : 0));
  if (act == kSigmoid && !tap) hipLaunchKernelGGL((fgemm_kernel<kSigmoid, false>), grid, block, 0, s, p);
  else if (act == kSigmoid) hipLaunchKernelGGL((fgemm_kernel<kSigmoid, true>), grid, block, 0, s, p);
  else if (!tap) hipLaunchKernelGGL((fgemm_kernel<kExp, false>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((fgemm_kernel<kExp, true>), grid, block, 0, s, p);
}

void launch_input_step(const float *x, const float *shift, const float *scale, float *xs, float *lin, int n, int dim, int ld, ihipStream_t *s) {
  if (n <= 0) return;
  g_float_launches.bump(4);
  const size_t total = static_cast<size_t>(n) * ld;
  hipLaunchKernelGGL(input_step_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, x, shift, scale, xs, lin, n, dim, ld);
}

void launch_report(const ReportParams &p, ihipStream_t *s) {
  if (p.n <= 0) return;
  const unsigned nodes = static_cast<unsigned>((p.O + 255) / 256), blocks = static_cast<unsigned>((p.n + kReportRows - 1) / kReportRows);
  g_float_launches.bump(5);
  hipLaunchKernelGGL(report_rows_kernel, dim3(static_cast<unsigned>((p.n + 3) / 4)), dim3(256), 0, s, p);
  g_float_launches.bump(6);
  hipLaunchKernelGGL(report_nodes_kernel, dim3(nodes, blocks), dim3(256), 0, s, p);
  g_float_launches.bump(7);
  hipLaunchKernelGGL(report_fold_kernel, dim3(nodes), dim3(256), 0, s, p);
}

void launch_counts(unsigned long long out[kLaunchKinds]) { g_float_launches.read(out); }

}  // namespace fl
}  // namespace fdnn
