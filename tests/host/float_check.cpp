// Stand-alone checker of fdnn_float.hpp and the float loader of fdnn_model.cpp (no HIP, no GPU), built and run under
// -fsanitize=address,undefined by tests/test_float_host.py:
//   * the loader takes what load_host_model takes and rejects what it rejects, with the same code and message;
//   * the packed blob: sections inside the blob, pad rows +0, pad columns -0, and padding never changes a sum -- not even
//     the sign of a zero that an underflow left behind;
//   * the buffer counts of a call cover what every launch of every chunk touches, for n = 1 .. 5000 and every chunk size 1 .. 5001 (one shape; a list of
//     sizes for the others);
//   * float_layer_ref stays within gamma(K + 1) (sum |x w| + |b|) + K 2^-126 of a long double sum.
//     usage: float_check <scratch directory>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/fdnn.h"
#include "fdnn_float.hpp"
#include "fdnn_model.hpp"

namespace fl = fdnn::fl;

static int g_fail = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                 \
      std::printf("\n");                        \
      ++g_fail;                                 \
    }                                           \
  } while (0)

static void put_be32(std::vector<uint8_t> &b, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) b.push_back(uint8_t(v >> s));
}
static void put_f32(std::vector<uint8_t> &b, float f) {
  uint32_t v;
  std::memcpy(&v, &f, 4);
  put_be32(b, v);
}

// A .bin of the given topology with weights w(j, r, k) = small deterministic values.
static std::vector<uint8_t> make_bin(const std::vector<int> &topo, int n_layers_field = -1) {
  std::vector<uint8_t> b;
  const int L = int(topo.size()) - 1;
  put_be32(b, uint32_t(n_layers_field < 0 ? L : n_layers_field));
  for (int j = 0; j < L; ++j) {
    put_be32(b, uint32_t(topo[size_t(j)]));
    put_be32(b, uint32_t(topo[size_t(j) + 1]));
    for (int r = 0; r < topo[size_t(j) + 1]; ++r)
      for (int k = 0; k < topo[size_t(j)]; ++k) put_f32(b, 0.01f * float((r * 7 + k * 3 + j) % 19 - 9));
    for (int r = 0; r < topo[size_t(j) + 1]; ++r) put_f32(b, 0.1f * float(r % 5 - 2));
  }
  for (int k = 0; k < topo[0]; ++k) put_f32(b, 0.5f);
  for (int k = 0; k < topo[0]; ++k) put_f32(b, 0.25f);
  return b;
}

static std::string write_file(const std::string &dir, const char *name, const std::vector<uint8_t> &bytes) {
  const std::string p = dir + "/" + name;
  FILE *f = std::fopen(p.c_str(), "wb");
  if (!f) {
    std::printf("cannot write %s\n", p.c_str());
    std::exit(2);
  }
  if (!bytes.empty()) std::fwrite(bytes.data(), 1, bytes.size(), f);
  std::fclose(f);
  return p;
}

// Both loaders on one file: same code, same message; returns the code.
static int both(const std::string &path, const char *what, fl::FloatHostModel *keep = nullptr) {
  fdnn::HostModel q;
  fl::FloatHostModel f;
  std::string mq, mf;
  const int rq = fdnn::load_host_model(path, 3.0f, &q, &mq), rf = fdnn::load_float_host_model(path, &f, &mf);
  CHECK(rq == rf, "%s: quantized loader %d, float loader %d", what, rq, rf);
  CHECK(rq == 0 || mq == mf, "%s: messages differ: '%s' / '%s'", what, mq.c_str(), mf.c_str());
  if (rq == 0 && rf == 0) {
    CHECK(q.hdr.in_dim == f.in_dim && q.hdr.in_dim_file == f.in_dim_file && q.hdr.out_dim == f.out_dim() &&
              q.hdr.n_affine == int(f.layers.size()),
          "%s: the two loaders disagree on the shape", what);
    // layer 0 is fp32 in both blobs: the same bytes
    for (int r = 0; r < q.hdr.hidden; ++r)
      CHECK(std::memcmp(q.w0() + size_t(r) * q.hdr.in_dim, f.w(0) + size_t(r) * f.layers[0].K_pad, sizeof(float) * size_t(f.in_dim)) == 0,
            "%s: layer-0 row %d differs between the loaders", what, r);
  }
  if (keep) *keep = f;
  return rf;
}

static void check_loader(const std::string &dir) {
  fl::FloatHostModel fm;
  CHECK(both(write_file(dir, "ok.bin", make_bin({20, 48, 48, 48, 131})), "20-3x48-131", &fm) == FDNN_OK, "a good file is refused");
  CHECK(fm.in_dim == 20 && fm.layers.size() == 4 && fm.layers[0].K_pad == 32 && fm.layers[1].K_pad == 64 && fm.layers[3].rows_pad == 256,
        "padding of 20-3x48-131");
  CHECK(both(write_file(dir, "pad.bin", make_bin({18, 16, 16, 16, 5})), "input width 18", &fm) == FDNN_OK, "input width 18 is refused");
  CHECK(fm.in_dim == 20 && fm.in_dim_file == 18, "input width 18 pads to 20");
  for (int r = 0; r < 16; ++r)
    for (int k = 18; k < 20; ++k) CHECK(fm.w(0)[size_t(r) * 32 + k] == 0.0f && !std::signbit(fm.w(0)[size_t(r) * 32 + k]), "x4 pad weights are +0");
  CHECK(fm.shift()[18] == 0.0f && fm.scale()[19] == 0.0f, "x4 pad shift / scale are 0");
  CHECK(both(dir + "/missing.bin", "missing file") == FDNN_E_IO, "missing file");
  CHECK(both(write_file(dir, "empty.bin", {}), "empty file") == FDNN_E_IO, "empty file");
  CHECK(both(write_file(dir, "three.bin", make_bin({20, 16, 16, 5})), "three layers") == FDNN_E_FORMAT, "layer count 3");
  CHECK(both(write_file(dir, "many.bin", make_bin({20, 16, 16, 16, 5}, 40)), "forty layers") == FDNN_E_FORMAT, "layer count 40");
  CHECK(both(write_file(dir, "h24.bin", make_bin({20, 24, 24, 24, 5})), "hidden width 24") == FDNN_E_FORMAT, "hidden width 24");
  CHECK(both(write_file(dir, "uneq.bin", make_bin({20, 16, 32, 32, 5})), "unequal hidden widths") == FDNN_E_FORMAT, "unequal hidden widths");
  std::vector<uint8_t> t = make_bin({20, 16, 16, 16, 5});
  for (size_t cut : {size_t(1), size_t(40), t.size() / 2, size_t(7)}) {
    std::vector<uint8_t> s(t.begin(), t.end() - long(cut));
    CHECK(both(write_file(dir, "trunc.bin", s), "truncated") == FDNN_E_FORMAT, "truncated by %zu", cut);
  }
}

static void check_blob(const std::string &dir) {
  fl::FloatHostModel fm;
  both(write_file(dir, "ok.bin", make_bin({20, 48, 48, 48, 131})), "blob", &fm);
  for (size_t j = 0; j < fm.layers.size(); ++j) {
    const fl::LayerDesc &d = fm.layers[j];
    CHECK(d.off_w % 256 == 0 && d.off_bias % 256 == 0, "sections are 256-byte aligned");
    CHECK(d.off_w + sizeof(float) * size_t(d.rows_pad) * d.K_pad <= fm.blob.size() && d.off_bias + sizeof(float) * size_t(d.rows_pad) <= fm.blob.size(),
          "sections inside the blob");
    CHECK(d.K_pad % fl::kKStep == 0 && d.K_pad >= d.K && d.K_pad - d.K < fl::kKStep, "K_pad");
    CHECK(d.rows_pad % fl::kRowPad == 0 && d.rows_pad % fl::kNodeTile == 0 && d.rows_pad >= d.rows && d.rows_pad - d.rows < fl::kRowPad, "rows_pad");
    for (int r = 0; r < d.rows_pad; ++r)
      for (int k = 0; k < d.K_pad; ++k) {
        const float v = fm.w(int(j))[size_t(r) * d.K_pad + k];
        if (r >= d.rows) CHECK(v == 0.0f && !std::signbit(v), "pad rows are +0");
        else if (k >= d.K) CHECK(v == 0.0f && std::signbit(v), "pad columns are -0");
      }
    for (int r = d.rows; r < d.rows_pad; ++r) CHECK(fm.bias(int(j))[r] == 0.0f, "pad bias");
  }
  CHECK(fm.off_shift % 256 == 0 && fm.off_scale + sizeof(float) * size_t(fm.layers[0].K_pad) <= fm.blob.size(), "shift / scale sections");
}

static uint32_t bits(float f) {
  uint32_t v;
  std::memcpy(&v, &f, 4);
  return v;
}

// The sums over the padded K (pad columns of w -0, of x +0) are the sums over the true K, bit for bit.
static void check_padding() {
  std::mt19937 rng(5);
  std::uniform_real_distribution<float> u(-2.0f, 2.0f);
  for (int K : {1, 20, 31, 32, 33, 48, 75}) {
    const int K_pad = int(fl::align_up(size_t(K), fl::kKStep)), rows = 7, n = 5;
    std::vector<float> w(size_t(rows) * K_pad, -0.0f), x(size_t(n) * K_pad, 0.0f), b(rows);
    for (int r = 0; r < rows; ++r) {
      for (int k = 0; k < K; ++k) w[size_t(r) * K_pad + k] = u(rng);
      b[size_t(r)] = r == 3 ? -0.0f : u(rng);
    }
    for (int f = 0; f < n; ++f)
      for (int k = 0; k < K; ++k) x[size_t(f) * K_pad + k] = u(rng);
    // frame 0, node 3: every term but the last is +-0 (s stays +0), the LAST true product is tiny, negative and underflows:
    // s = -0, the bias is -0: z = -0
    for (int k = 0; k < K; ++k) x[k] = 0.0f;
    x[K - 1] = 1e-30f;
    w[size_t(3) * K_pad + K - 1] = -1e-30f;
    std::vector<float> a(size_t(n) * rows), p(size_t(n) * rows);
    fl::float_layer_ref(w.data(), K_pad, b.data(), rows, K, x.data(), K_pad, n, a.data());
    fl::float_layer_ref(w.data(), K_pad, b.data(), rows, K_pad, x.data(), K_pad, n, p.data());
    for (size_t i = 0; i < a.size(); ++i) CHECK(bits(a[i]) == bits(p[i]), "K %d: output %zu changes with the padding", K, i);
    CHECK(bits(a[3]) == 0x80000000u, "K %d: the underflow case is -0 (got %08x)", K, bits(a[3]));
    // and what a +0 pad would have done: the reason the pad is -0
    if (K_pad > K) {
      std::vector<float> w0(w);
      for (int k = K; k < K_pad; ++k) w0[size_t(3) * K_pad + k] = 0.0f;
      fl::float_layer_ref(w0.data(), K_pad, b.data(), rows, K_pad, x.data(), K_pad, 1, p.data());
      CHECK(bits(p[3]) == 0u, "K %d: a +0 pad turns the -0 into +0", K);
    }
  }
}

// Every chunk of a call stays inside the call's buffer counts, the chunks tile [0, n), the grid covers a chunk's frames.
static void check_call(const fl::Shape &s, int n, int chunk) {
  const fl::Counts c = fl::counts(s, n, chunk);
  int covered = 0;
  for (int i = 0; i < fl::n_chunks(n, chunk); ++i) {
    int first, m;
    fl::chunk_range(n, chunk, i, &first, &m);
    CHECK(first == covered && m >= 1 && m <= c.cap, "n %d chunk %d: chunk %d is [%d, +%d)", n, chunk, i, first, m);
    covered += m;
    unsigned gx, gy;
    fl::gemm_grid(m, s.out_rows_pad, &gx, &gy);
    CHECK(size_t(gx) * fl::kFrameTile >= size_t(m) && size_t(gx - 1) * fl::kFrameTile < size_t(m) && int(gy) * fl::kNodeTile == s.out_rows_pad,
          "grid of %d frames", m);
    if (fl::rows_extent(m, s.k0_pad, s.k0_pad) > c.xs || fl::rows_extent(m, s.act_ld, s.act_ld) > c.act ||
        fl::partial_extent(m, c.cap, s.out_rows_pad / fl::kPartialNodes) > c.partial)
      CHECK(false, "n %d chunk %d: a launch over %d frames leaves its buffers", n, chunk, m);
  }
  CHECK(covered == n, "n %d chunk %d: chunks cover %d frames", n, chunk, covered);
}

static void check_layout() {
  fl::Shape shapes[3];
  shapes[0] = fl::Shape{32, 64, 131, 256};
  shapes[1] = fl::Shape{448, 256, 1000, 1024};
  shapes[2] = fl::Shape{448, 2048, 8000, 8192};
  // EVERY chunk size a call of up to 5000 frames can tell apart (1 .. 5001; beyond n a chunk size is n), every n
  for (int chunk = 1; chunk <= 5001; ++chunk) {
    CHECK(fl::chunk_rows(chunk) == chunk, "chunk_rows(%d)", chunk);
    for (int n = 1; n <= 5000; ++n) check_call(shapes[0], n, chunk);
  }
  // the other shapes (the layout is linear in the row lengths) and the largest setting, over the sizes around the tiles
  const int chunks[] = {1, 2, 31, 127, 128, 129, 160, 1000, 4095, 4096, 4097, 5000, fl::kMaxChunk};
  for (const fl::Shape &s : shapes)
    for (int chunk : chunks) {
      CHECK(fl::chunk_rows(chunk) == chunk, "chunk_rows(%d)", chunk);
      for (int n = 1; n <= 5000; ++n) check_call(s, n, chunk);
    }
  CHECK(fl::chunk_rows(0) == fl::kDefaultChunk && fl::chunk_rows(-3) == fl::kDefaultChunk && fl::chunk_rows(1 << 30) == fl::kMaxChunk, "chunk_rows");
}

static void check_ref_bound() {
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  const long double uu = std::ldexp(1.0L, -24);
  for (int K : {1, 20, 48, 432, 2064}) {
    const int rows = 9, n = 6;
    std::vector<float> w(size_t(rows) * K), x(size_t(n) * K), b(rows), z(size_t(n) * rows);
    for (float &v : w) v = u(rng);
    for (float &v : x) v = 20.0f * u(rng);
    for (float &v : b) v = u(rng);
    fl::float_layer_ref(w.data(), K, b.data(), rows, K, x.data(), K, n, z.data());
    for (int f = 0; f < n; ++f)
      for (int r = 0; r < rows; ++r) {
        long double s = 0, S = 0;
        for (int k = 0; k < K; ++k) {
          const long double t = (long double)x[size_t(f) * K + k] * (long double)w[size_t(r) * K + k];
          s += t;
          S += std::fabs(t);
        }
        s += b[size_t(r)];
        S += std::fabs((long double)b[size_t(r)]);
        const long double g = (K + 1) * uu / (1 - (K + 1) * uu), bound = g * S + K * std::ldexp(1.0L, -126);
        CHECK(std::fabs((long double)z[size_t(f) * rows + r] - s) <= bound, "K %d: float_layer_ref outside the bound", K);
      }
  }
  // input step: two roundings
  const float sh[2] = {0.1f, -3.0f}, sc[2] = {0.0625f, 1.7f}, xx[4] = {1.0f, 2.0f, 1e-8f, 3.00001f};
  float lin[4], act[4];
  fl::float_input_ref(sh, sc, 2, xx, 2, lin, act);
  for (int i = 0; i < 4; ++i) {
    const float t = xx[i] + sh[i & 1];
    CHECK(bits(lin[i]) == bits(t) && bits(act[i]) == bits(t * sc[i & 1]), "input step %d", i);
  }
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: float_check <scratch directory>\n");
    return 2;
  }
  check_loader(argv[1]);
  check_blob(argv[1]);
  check_padding();
  check_layout();
  check_ref_bound();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("float ok\n");
  return 0;
}
