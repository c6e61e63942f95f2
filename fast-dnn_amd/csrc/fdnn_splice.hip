// fdnn_splice.hip -- the <Splice> block of a Kaldi nnet1 feature transform on the device (gfx950).
//
// Every net this library runs reads spliced input: row t is the raw feature frames f(t + o_0) .. f(t + o_{C-1}) side by
// side, then zeros up to the padded layer-0 width (BatchData.alignDimension; convert.splice_frames is the host
// definition).  The reference receives those rows from the caller, spliced on the host: 11 copies of every 39-float
// frame over PCIe.  Here the raw frames travel once and splice_kernel materialises the rows in the context's frame buffer,
// which the pass then reads as it reads any caller's rows -- the same bytes, so every result is bit-identical.
//
// Rows are cut into segments (utterances, or the part of one that a chunk, a shard or a server piece covers): a row reads
// raw frames of its own segment only, clamped to that segment's first and last frame (Kaldi's edge rule).
#include "fdnn_device.hpp"
#include "fdnn_kernels.hpp"

#include <algorithm>
#include <atomic>

namespace fdnn {
namespace {

// One lane builds 16 contiguous bytes of a row (one dwordx4 store; a wave writes 1 KiB).  D = 39 is not a multiple of 4,
// so a float4 can straddle two D-blocks: the four values are gathered one by one, walking (block, column) from the lane's
// first column with one division per lane.  Raw frames are re-read up to C times; at 156 B per frame they stay in L2.
// The offsets and the segment table are indexed per lane: read from the kernel arguments, every such read is a memory load
// the raw read behind it waits for, and each wait drains the gathers before it.  So a workgroup first copies them to LDS,
// and a lane works out all four source addresses before it issues any of its four gathers.
__global__ __launch_bounds__(256) void splice_kernel(const float *__restrict__ raw, float *__restrict__ x, int row0, int rows,
                                                     int raw_frames, SpliceArgs a) {
  __shared__ int s_off[kSpliceMaxOffsets];
  __shared__ int s_row[kSpliceMaxSegs], s_center[kSpliceMaxSegs], s_lo[kSpliceMaxSegs], s_hi[kSpliceMaxSegs];
  for (int i = threadIdx.x; i < a.count; i += 256) s_off[i] = a.offsets[i];
  for (int i = threadIdx.x; i < a.n_segs; i += 256) {
    s_row[i] = a.seg_row[i];
    s_center[i] = a.seg_center[i];
    s_lo[i] = a.seg_lo[i];
    s_hi[i] = a.seg_hi[i];
  }
  __syncthreads();
  const unsigned q4 = static_cast<unsigned>(a.input_dim) >> 2;
  const int D = a.raw_dim;
  const int width = a.count * D;  // columns that carry frames; the rest are zero
  const unsigned total = static_cast<unsigned>(rows) * q4;  // (< 2^31: launch_splice cuts larger ranges)
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const int r = static_cast<int>(i / q4);
    const int col = static_cast<int>(i - static_cast<unsigned>(r) * q4) * 4;
    const int t = row0 + r;
    int sg = 0, hi = a.n_segs - 1;  // sg: the last segment starting at or before row t (starts ascend)
    while (sg < hi) {
      const int mid = (sg + hi + 1) >> 1;
      if (s_row[mid] <= t)
        sg = mid;
      else
        hi = mid - 1;
    }
    const int center = s_center[sg] + (t - s_row[sg]);
    const int f_lo = max(s_lo[sg], 0), f_hi = min(s_hi[sg], raw_frames - 1);  // (never outside the buffer)
    int blk = col / D, k = col - blk * D;
    int src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // the four source indices first (-1: a pad column) ...
      src[j] = col + j < width ? min(max(center + s_off[blk], f_lo), f_hi) * D + k : -1;
      if (++k == D) {
        k = 0;
        ++blk;
      }
    }
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = src[j] >= 0 ? raw[src[j]] : 0.0f;  // ... then the four gathers, in flight together
    *reinterpret_cast<float4 *>(x + static_cast<size_t>(r) * a.input_dim + col) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// The same rows for a batch whose segment table is too long for the kernel arguments: a live batch of the scoring loop has
// one segment per push, hundreds of them.  The table lives in device memory -- segs[g] = (row, center, lo, hi), one 16-byte
// load -- and beside it one word per row, row_seg[r]: the index of row r's segment.  The host that builds the table knows it
// (4 B per row written there against 1 728 B of row here), so no lane searches: the lanes of a row read the same word, then
// the same segment, and from there on this is splice_kernel's lane for lane -- same layout, same clamping, same values.
// Only the offsets are kernel arguments (LDS, as above).  A row_seg outside the table is clamped into it, and a frame index
// never leaves [max(lo, 0), min(hi, raw_frames - 1)]: whatever the table says, nothing is read outside the raw buffer.
__global__ __launch_bounds__(256) void splice_table_kernel(const float *__restrict__ raw, float *__restrict__ x, int row0, int rows, int raw_frames,
                                                           const int4 *__restrict__ segs, const int *__restrict__ row_seg, int n_segs,
                                                           SpliceOffsets a) {
  __shared__ int s_off[kSpliceMaxOffsets];
  for (int i = threadIdx.x; i < a.count; i += 256) s_off[i] = a.offsets[i];
  __syncthreads();
  const unsigned q4 = static_cast<unsigned>(a.input_dim) >> 2;
  const int D = a.raw_dim;
  const int width = a.count * D;
  const unsigned total = static_cast<unsigned>(rows) * q4;  // (< 2^31: launch_splice_table cuts larger ranges)
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const int r = static_cast<int>(i / q4);
    const int col = static_cast<int>(i - static_cast<unsigned>(r) * q4) * 4;
    const int t = row0 + r;
    const int4 sg = segs[min(max(row_seg[t], 0), n_segs - 1)];  // (x, y, z, w) = (row, center, lo, hi)
    const int center = sg.y + (t - sg.x);
    // splice_kernel's [max(lo, 0), min(hi, raw_frames - 1)] for every segment that holds a frame of the buffer; a table from
    // device memory that does not (hi < 0, lo past the end) still reads inside it
    const int f_lo = min(max(sg.z, 0), raw_frames - 1), f_hi = min(max(sg.w, f_lo), raw_frames - 1);
    int blk = col / D, k = col - blk * D;
    int src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      src[j] = col + j < width ? min(max(center + s_off[blk], f_lo), f_hi) * D + k : -1;
      if (++k == D) {
        k = 0;
        ++blk;
      }
    }
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = src[j] >= 0 ? raw[src[j]] : 0.0f;
    *reinterpret_cast<float4 *>(x + static_cast<size_t>(r) * a.input_dim + col) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// the table kernel's own count (fdnn_debug_live_launches): not a name of the launch recorder (fdnn_note.hpp)
std::atomic<unsigned long long> g_table_launches{0}, g_table_max_segs{0};

}  // namespace

void launch_splice_table(const float *raw, int raw_frames, float *x, int rows, const int32_t *d_segs, const int32_t *d_row_seg, int n_segs,
                         const SpliceOffsets &a, hipStream_t s) {
  const int q4 = a.input_dim / 4;
  if (q4 < 1 || n_segs < 1 || raw_frames < 1 || rows < 1) return;
  unsigned long long seen = g_table_max_segs.load(std::memory_order_relaxed);
  while (seen < static_cast<unsigned long long>(n_segs) && !g_table_max_segs.compare_exchange_weak(seen, n_segs, std::memory_order_relaxed)) continue;
  // rows per launch: 32-bit lane indices.  19 million rows of 432 columns: ONE launch for every batch of the scoring loop
  const int step = std::max(1, (0x7fffffff - 256 * 4096) / q4);
  for (int r = 0; r < rows; r += step) {
    const int cnt = std::min(step, rows - r);
    const long long total = static_cast<long long>(cnt) * q4;
    const int blocks = static_cast<int>(std::min<long long>((total + 255) / 256, 256 * 16));
    g_table_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(splice_table_kernel, dim3(blocks), dim3(256), 0, s, raw, x + static_cast<size_t>(r) * a.input_dim, r, cnt, raw_frames,
                       reinterpret_cast<const int4 *>(d_segs), d_row_seg, n_segs, a);
  }
}

void splice_table_counts(unsigned long long *launches, unsigned long long *max_segs) {
  *launches = g_table_launches.load(std::memory_order_relaxed);
  *max_segs = g_table_max_segs.load(std::memory_order_relaxed);
}

void launch_splice(const float *raw, int raw_frames, float *x, int row0, int rows, const SpliceArgs &a, hipStream_t s) {
  const int q4 = a.input_dim / 4;
  if (q4 < 1 || a.n_segs < 1 || raw_frames < 1) return;
  const int step = std::max(1, (0x7fffffff - 256 * 4096) / q4);  // rows per launch: 32-bit lane indices
  for (int r = 0; r < rows; r += step) {
    const int cnt = std::min(step, rows - r);
    const long long total = static_cast<long long>(cnt) * q4;
    const int blocks = static_cast<int>(std::min<long long>((total + 255) / 256, 256 * 16));
    note_launch(kLn_splice);
    hipLaunchKernelGGL(splice_kernel, dim3(blocks), dim3(256), 0, s, raw, x + static_cast<size_t>(r) * a.input_dim, row0 + r, cnt,
                       raw_frames, a);
  }
}

}  // namespace fdnn
