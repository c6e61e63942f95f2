// fdnn_align.hip -- FORCED ALIGNMENT: the best monotone path of a transcript's states over a segment's rows, and its score
// (fdnn_align.hpp: the emission, the step, the plan, the host restatement -- the arithmetic is the header's, called from here).
//
//   The caller of LazyOutputActivations (dnn.cc:355-392) that the per-segment node sets were built for fetched rows x len
//   probabilities per utterance, took the logarithm, subtracted the priors and ran the Viterbi recursion on the host, one
//   utterance at a time.  Here the recursion runs where the probabilities are, and 4 bytes per frame leave the device.
//
// The row loop is sequential in t: both kernels keep the dependent chain of a frame short and everything that does not depend
// on d off it.
//
// align_wave_kernel<K, TYPE>: one wave per segment, S <= 64 K.  Lane l owns states [l K, l K + K): their d, column, prior and
// transition values live in registers.  Per frame the only communication is lane l - 1's last d, ONE DPP move (wave_shr:1;
// lane 0 keeps -inf); no LDS for d, no barrier.  Emissions do not depend on d: the loads of the next kFramesInFlight rows are
// issued, and the score() of the current ones is computed, before the steps that consume them, so the chain of
// a frame is the move, two additions, a compare and a select per owned state.  The take bits of the wave's lanes for slot k are
// the compare's own lane mask (a ballot); lane k stores word k.  At K = 16 a lane packs its sixteen bits into a 16-bit word
// of its own instead (sixteen ballots' selects held more lane masks than there are scalar registers): the same 32 words a frame.
// align_wg_kernel<TYPE>: 256 threads per segment, any S <= kMaxStates.  d lives as two rows in LDS, one barrier per frame;
// thread i owns states i, i + 256, ..  Column, node, prior and transition values are read again every frame (the L2 serves
// them): a transcript of 16384 states leaves no LDS and no registers to keep them.  The emissions are computed inside the
// frame: scoring frame t + 1 ahead of frame t's barrier was built and measured, and changed nothing.
// Back-trace: T dependent reads by one lane, from LDS where the segment's take words fit (align::kBpLdsWords), else from the
// call's scratch (written through to the L2, read back after a fence).
//
// No atomics, no inline assembly, no device state that outlives a launch.  Built WITHOUT a flush-to-zero or fast-math flag
// and with -ffp-contract=off (csrc/Makefile): the header's sequence is what runs.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_align.hpp"

namespace fdnn {
namespace {

using namespace align;

LaunchCounts<2> g_align_launches;  // wave form, workgroup form
std::atomic<int> g_align_mode{0};  // fdnn_debug_set_align_kernel

struct Args {
  const float *rows;
  const int32_t *col, *node;  // node: null without a handle
  const float *prior;         // the handle's log priors [width]
  int width;
  float floor;
  const float *self_lp, *next_lp;  // null: +0
  uint32_t *scratch;
  int32_t *path;
  float *total;
};

// the value of lane - 1 (lane 0: `first`): DPP wave_shr:1, a full-rate VALU move
__device__ inline float from_lane_below(float v, float first) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, first), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

// what a thread keeps of one state: the column (-1 unless the state exists and its column and node are in range: the
// validity is one register, not a lane mask held in scalar registers across the row loop) and the prior
struct State {
  int col;
  float prior;
  __device__ bool valid() const { return col >= 0; }
};

template <int TYPE>
__device__ inline State load_state(const Args &a, int at, bool in, int ld) {
  State st{-1, 0.0f};
  if (!in) return st;
  const int c = a.col[at];
  st.col = (c >= 0 && c < ld) ? c : -1;
  if constexpr (TYPE != kScores) {
    const int nd = a.node[at];
    if (nd >= 0 && nd < a.width) st.prior = a.prior[nd];
    else st.col = -1;
  }
  return st;
}

// K: the wave form's states per lane, 0 for the workgroup form
template <int K>
__device__ inline void finish(const Launch &L, int seg, const Args &a, float tot, const uint64_t *bp, int words64_per_frame, bool first_thread) {
  // (the callers have made the take words visible: a fence and a barrier)
  const int T = L.T[seg], S = L.S[seg];
  int32_t *path = a.path + L.path_off[seg];
  const uint32_t tb = total_bits(tot);
  if (!finite_bits(tb)) {
    for (int t = static_cast<int>(threadIdx.x); t < T; t += static_cast<int>(blockDim.x)) path[t] = -1;
  } else if (first_thread) {
    int j = S - 1;
    for (int t = T - 1; t >= 1; --t) {
      path[t] = j;
      if constexpr (K == 16) {  // wave form, 16 states a lane: 16-bit word j / 16, bit j % 16
        j -= (reinterpret_cast<const uint16_t *>(bp)[static_cast<size_t>(t) * kWaveLanes + (j >> 4)] >> (j & 15)) & 1;
      } else {  // wave form: 64-bit word j % K, bit j / K; workgroup form: word j / 64, bit j % 64
        const int word = K ? (j & (K - 1)) : (j >> 6), bit = K ? j / (K ? K : 1) : (j & 63);
        j -= static_cast<int>((bp[static_cast<size_t>(t) * words64_per_frame + word] >> bit) & 1u);
      }
    }
    path[0] = j;
  }
  if (first_thread) a.total[L.total_off[seg]] = float_of(tb);
}

template <int K, int TYPE>
__global__ __launch_bounds__(kWaveLanes) void align_wave_kernel(const Launch L, const Args a) {
  extern __shared__ uint64_t lds64[];
  constexpr int U = frames_in_flight(K);
  const int seg = static_cast<int>(blockIdx.x), lane = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg];
  const float *rows = a.rows + L.row_off[seg];
  uint64_t *bp = L.bp_off[seg] < 0 ? lds64 : reinterpret_cast<uint64_t *>(a.scratch + L.bp_off[seg]);
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);

  State st[K];
  float self[K], next[K];  // next[k]: next_lp of the state BELOW slot k's
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = lane * K + k;
    st[k] = load_state<TYPE>(a, s0 + j, j < S, ld);
    self[k] = (j < S && a.self_lp) ? a.self_lp[s0 + j] : 0.0f;
    next[k] = (j < S && j > 0 && a.next_lp) ? a.next_lp[s0 + j - 1] : 0.0f;
  }
  auto load_row = [&](int t, float (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (st[k].valid() && t < T) ? rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(st[k].col)] : nan;
  };

  float d[K];
  {
    float v[K];
    load_row(0, v);
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = ninf;
    if (lane == 0) d[0] = emission(v[0], st[0].prior, a.floor, TYPE);
  }
  float v[U][K];
#pragma unroll
  for (int u = 0; u < U; ++u) load_row(1 + u, v[u]);
  for (int t0 = 1; t0 < T; t0 += U) {
    float e[U][K];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) e[u][k] = emission(v[u][k], st[k].prior, a.floor, TYPE);
#pragma unroll
    for (int u = 0; u < U; ++u) load_row(t0 + U + u, v[u]);  // in flight during the steps below
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u;
      if (t >= T) break;  // (uniform)
      const float below = from_lane_below(d[K - 1], ninf);
      float nd[K];
      uint64_t mine = 0;
      uint32_t bits = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        bool take;
        nd[k] = step(d[k], self[k], k ? d[k - 1] : below, next[k], e[u][k], &take);
        if constexpr (K == 16) {
          bits |= take ? (1u << k) : 0u;  // a lane's sixteen bits are one 16-bit word of its own
        } else {
          const uint64_t m = __ballot(take);  // (the compare's own lane mask)
          if (lane == k) mine = m;
        }
      }
#pragma unroll
      for (int k = 0; k < K; ++k) d[k] = nd[k];
      if constexpr (K == 16)
        reinterpret_cast<uint16_t *>(bp)[static_cast<size_t>(t) * kWaveLanes + lane] = static_cast<uint16_t>(bits);
      else if (lane < K)
        bp[static_cast<size_t>(t) * K + lane] = mine;
    }
  }

  // the total: slot (S - 1) % K of lane (S - 1) / K
  float last = d[0];
#pragma unroll
  for (int k = 1; k < K; ++k)
    if (((S - 1) & (K - 1)) == k) last = d[k];
  const float tot = __shfl(last, (S - 1) / K);
  __threadfence();
  __syncthreads();
  finish<K>(L, seg, a, tot, bp, K, lane == 0);
}

template <int TYPE>
__global__ __launch_bounds__(kWgThreads) void align_wg_kernel(const Launch L, const Args a) {
  extern __shared__ uint64_t lds64[];
  const int seg = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
  const int T = L.T[seg], S = L.S[seg], ld = L.ld[seg], s0 = L.state0[seg];
  const int S64 = (S + 63) / 64 * 64, wpf = S64 / 64;  // whole waves walk the states: a wave's ballot is one take word
  const float *rows = a.rows + L.row_off[seg];
  float *cur = reinterpret_cast<float *>(lds64), *nxt = cur + L.d_floats;
  uint64_t *bp = L.bp_off[seg] < 0 ? lds64 + L.d_floats : reinterpret_cast<uint64_t *>(a.scratch + L.bp_off[seg]);
  const float ninf = float_of(kMinusInf), nan = float_of(kQuietNaN);

  auto emit = [&](int t, int j) {
    const State st = load_state<TYPE>(a, s0 + j, true, ld);
    const float v = st.valid() ? rows[static_cast<size_t>(t) * static_cast<size_t>(ld) + static_cast<size_t>(st.col)] : nan;
    return emission(v, st.prior, a.floor, TYPE);
  };
  for (int j = tid; j < S64; j += kWgThreads) cur[j] = ninf;
  if (tid == 0) cur[0] = emit(0, 0);
  __syncthreads();
  for (int t = 1; t < T; ++t) {
    for (int j = tid; j < S64; j += kWgThreads) {
      const bool in = j < S;
      float e = 0.0f, self = 0.0f, next = 0.0f;
      if (in) {  // (none of these depends on d)
        e = emit(t, j);
        if (a.self_lp) self = a.self_lp[s0 + j];
        if (a.next_lp && j > 0) next = a.next_lp[s0 + j - 1];
      }
      bool take;
      const float dj = step(cur[j], self, j ? cur[j - 1] : ninf, next, e, &take);
      nxt[j] = in ? dj : ninf;  // (the padding past S is kept at -inf: nothing below S reads it, and its bits are masked out)
      const uint64_t m = __ballot(in && take);
      if ((tid & 63) == 0) bp[static_cast<size_t>(t) * wpf + (j >> 6)] = m;
    }
    __syncthreads();
    float *sw = cur;
    cur = nxt, nxt = sw;
  }
  const float tot = cur[S - 1];
  __threadfence();
  __syncthreads();
  finish<0>(L, seg, a, tot, bp, wpf, tid == 0);
}

template <class Kernel>
void launch_wg(Kernel kernel, const Launch &l, const Args &a, hipStream_t s) {
  // 2 x kMaxStates floats and the take words: above the 64 KiB a launch gets unasked.  Per device, like every sibling launcher
  // (one mask per kernel instance: the static is this template instance's)
  static std::atomic<unsigned long long> attr_set{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (2 * kMaxStates + kBpLdsWords));
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(kernel, dim3(l.n_segs), dim3(kWgThreads), l.lds_bytes, s, l, a);
}

template <int TYPE>
void launch_typed(const Launch &l, const Args &a, hipStream_t s) {
  const dim3 grid(l.n_segs);
  if (l.form == kWorkgroup) {
    launch_wg(align_wg_kernel<TYPE>, l, a, s);
    return;
  }
  switch (l.K) {
    case 1: hipLaunchKernelGGL((align_wave_kernel<1, TYPE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    case 2: hipLaunchKernelGGL((align_wave_kernel<2, TYPE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    case 4: hipLaunchKernelGGL((align_wave_kernel<4, TYPE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    case 8: hipLaunchKernelGGL((align_wave_kernel<8, TYPE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
    default: hipLaunchKernelGGL((align_wave_kernel<16, TYPE>), grid, dim3(kWaveLanes), l.lds_bytes, s, l, a); break;
  }
}

}  // namespace

void launch_align(const align::Plan &p, const AlignArgs &g, hipStream_t s) {
  const Args a{g.d_rows, g.d_col, g.d_state_node, g.d_log_prior, g.width, g.floor, g.d_self_lp, g.d_next_lp, g.d_scratch, g.d_path, g.d_total};
  for (const Launch &l : p.launches) {
    g_align_launches.bump(l.form == kWave ? 0 : 1);
    if (g.type == kScores) launch_typed<kScores>(l, a, s);
    else if (g.type == loglik::kF16) launch_typed<loglik::kF16>(l, a, s);
    else launch_typed<loglik::kF32>(l, a, s);
  }
}

void align_launch_counts(unsigned long long out[2]) { g_align_launches.read(out); }
int align_kernel_mode() { return g_align_mode.load(std::memory_order_relaxed); }
void align_kernel_mode(int mode) { g_align_mode.store(mode, std::memory_order_relaxed); }

}  // namespace fdnn
