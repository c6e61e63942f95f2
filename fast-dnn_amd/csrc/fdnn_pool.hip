// fdnn_pool.hip -- the dense output POOLED over a node -> class map: of every row of probabilities the sum over each class
// of output nodes (fdnn_pool.hpp: the map, the order of the additions, the plan, the host restatement).
//
//   CalculateOutput (dnn.cc:428-454) hands every caller output_dim floats per frame; a caller that wants the posterior of a
//   CLASS of senones -- silence for VAD and end-pointing, phones for posteriorgrams and keyword spotting -- adds them up on
//   the host after 3.2 MB per 100 frames of the 8000-node net have crossed PCIe.  Here the device adds: n x C x 4 bytes leave.
//
// One workgroup of 256 threads per row, sixteen groups of 16 lanes (four to a wave), a class at a time per group:
//
//   * RESIDENT form (width <= kPoolResidentWidth): the row is read from memory ONCE -- 16-byte loads from the first 16-byte
//     boundary of the row on, the up to three values before it and after the last whole vector one by one -- and kept in
//     LDS, shifted by the row's misalignment so that a 16-byte load lands as a 16-byte LDS store.
//   * group g takes classes g, g + 16, ...: lane j reads the class's members j, j + 16, ... from the CSR (16 consecutive
//     indices a step: one 64-byte segment per group), gathers their values from LDS and adds them IN THAT ORDER into one
//     register, starting from +0.  Four members are in flight per lane; the additions stay sequential.
//   * the sixteen partial sums meet in four DPP steps -- quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
//     row_mirror: at lane 0 the xor-1/2/4/8 butterfly, i.e. the header's tree (a + b is commutative bit for bit away from
//     NaN payloads) -- and lane 0 stores q_c.
//   * STREAMING form (wider rows, fdnn_debug_set_pool_kernel(2)): the members are gathered from memory -- L2 / Infinity Cache
//     after the dense pass wrote them.  Same code, same bytes.
//
// No atomics, no device state that outlives a launch.  Built WITHOUT a flush-to-zero or fast-math flag (csrc/Makefile): the
// header's rule keeps denormals.
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"
#include "fdnn_launch.hpp"
#include "fdnn_pool.hpp"

namespace fdnn {
namespace {

using namespace pool;

LaunchCounts<2> g_pool_launches;  // resident, streaming
std::atomic<int> g_pool_mode{0};  // fdnn_debug_set_pool_kernel

// s + (s of the lane the DPP control names, inside the 16-lane row): one fp32 addition
template <int CTRL>
__device__ inline float dpp_add(float s) {
  const float o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), CTRL, 0xf, 0xf, false));
  return s + o;
}

template <bool RESIDENT>
__global__ __launch_bounds__(kThreads) void pool_kernel(const float *rows, int width, const int32_t *class_ptr, const int32_t *member,
                                                        int n_classes, float *out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t vals[];  // resident: [width + 4]
  const int t = threadIdx.x, lane = t & (kPoolLanes - 1), group = t / kPoolLanes;
  const uint32_t *row = reinterpret_cast<const uint32_t *>(rows) + static_cast<size_t>(blockIdx.x) * width;
  const int off = RESIDENT ? static_cast<int>((reinterpret_cast<uintptr_t>(row) >> 2) & 3) : 0;
  auto load = [&](int i) -> float { return __uint_as_float(RESIDENT ? vals[off + i] : row[i]); };

  if (RESIDENT) {
    const int head = min(width, (4 - off) & 3), nvec = (width - head) >> 2, tail = head + 4 * nvec;
    if (t < head) vals[off + t] = row[t];
    for (int v = t; v < nvec; v += kThreads) *reinterpret_cast<uint4 *>(vals + off + head + 4 * v) = *reinterpret_cast<const uint4 *>(row + head + 4 * v);
    if (t < width - tail) vals[off + tail + t] = row[tail + t];
    __syncthreads();
  }

  float *q = out + static_cast<size_t>(blockIdx.x) * n_classes;
  for (int c = group; c < n_classes; c += kGroups) {
    const int end = class_ptr[c + 1];
    int i = class_ptr[c] + lane;
    float s = 0.0f;
    for (; i + 3 * kPoolLanes < end; i += 4 * kPoolLanes) {  // four members in flight, added in member order
      const int m0 = member[i], m1 = member[i + kPoolLanes], m2 = member[i + 2 * kPoolLanes], m3 = member[i + 3 * kPoolLanes];
      const float v0 = load(m0), v1 = load(m1), v2 = load(m2), v3 = load(m3);
      s = s + v0;
      s = s + v1;
      s = s + v2;
      s = s + v3;
    }
    for (; i < end; i += kPoolLanes) s = s + load(member[i]);
    s = dpp_add<0xB1>(s);   // quad_perm [1,0,3,2]: lane ^ 1
    s = dpp_add<0x4E>(s);   // quad_perm [2,3,0,1]: lane ^ 2
    s = dpp_add<0x141>(s);  // row_half_mirror: lane 0 reads lane 7, which holds the other quad's sum
    s = dpp_add<0x140>(s);  // row_mirror: lane 0 reads lane 15, which holds the other half's sum
    if (lane == 0) q[c] = s;
  }
}

}  // namespace

void launch_pool(const float *d_rows, int n, int width, const int32_t *d_class_ptr, const int32_t *d_member, int n_classes, float *d_out, hipStream_t s) {
  if (n <= 0 || width < 1 || width > kMaxWidth || n_classes < 1 || n_classes > width) return;
  const Plan p = pool::plan(n, width, g_pool_mode.load(std::memory_order_relaxed));
  static std::atomic<unsigned long long> attr_set{0};  // per device: the resident form's LDS may pass the default limit
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_acquire) & dev_bit)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(pool_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              pool::plan(1, kPoolResidentWidth, 0).lds_bytes);
    attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  for (int r = 0; r < n; r += p.rows_per_launch) {
    const int cnt = std::min(p.rows_per_launch, n - r);
    const float *rows = d_rows + static_cast<size_t>(r) * width;
    float *q = d_out + static_cast<size_t>(r) * n_classes;
    g_pool_launches.bump(p.form == kResident ? 0 : 1);
    if (p.form == kResident)
      hipLaunchKernelGGL(pool_kernel<true>, dim3(cnt), dim3(kThreads), p.lds_bytes, s, rows, width, d_class_ptr, d_member, n_classes, q);
    else
      hipLaunchKernelGGL(pool_kernel<false>, dim3(cnt), dim3(kThreads), p.lds_bytes, s, rows, width, d_class_ptr, d_member, n_classes, q);
  }
}

void pool_launch_counts(unsigned long long out[2]) { g_pool_launches.read(out); }
int pool_kernel_mode() { return g_pool_mode.load(std::memory_order_relaxed); }
void pool_kernel_mode(int mode) { g_pool_mode.store(mode, std::memory_order_relaxed); }

}  // namespace fdnn
