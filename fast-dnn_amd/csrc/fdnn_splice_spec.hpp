// fdnn_splice_spec.hpp -- the splice types every raw-frame path shares, free of HIP: fdnn_server_plan.hpp builds without it.
#pragma once
#include <algorithm>
#include <memory>
#include <vector>

namespace fdnn {

// A splice spec (fdnn_model_set_splice): the <Splice> frame offsets and the raw frame width D.  Immutable once made: the
// model holds the current one, and every raw call, stream and queued server submission holds the one it started with.
struct SpliceSpec {
  std::vector<int> offsets;
  int raw_dim = 0;
  int left = 0, right = 0;  // max(-o, 0), max(o, 0): the context a row reads before and after its own frame
};
using SpliceRef = std::shared_ptr<const SpliceSpec>;

// A run of rows of one utterance: rows [row, next segment's row) read raw frames clamp(center + (t - row) + o, lo, hi) of the
// raw buffer (lo / hi: the buffer indices of the utterance's first and last frame).
struct SpliceSeg {
  int row, center, lo, hi;
};

// The raw frames rows [a, b) of an n-frame utterance reference: [*fa, *fb) (the halo of the offsets, clamped to it).
inline void splice_halo(const SpliceSpec &spec, int n, int a, int b, int *fa, int *fb) {
  *fa = std::max(0, a - spec.left);
  *fb = std::min(n, b + spec.right);
}

}  // namespace fdnn
