// serve_bench -- the serving shape, natively: T host threads, each scoring U utterances of F frames
// (100 frames = 1 s of speech) through the C-ABI, buffers reused, no interpreter in the loop.
//   serve_bench model.bin threads utts_per_thread frames mode [max_frames depth linger_us [c]]
//   mode: percall  = fdnn_calculate per utterance (what the JNI calculate() does)
//         server   = fdnn_server_submit + fdnn_server_wait (coalesced host submissions)
//         batcher  = fdnn_calculate on a model with fdnn_model_enable_batcher
//         fresh    = percall into a newly allocated, zero-filled result block per call (the reference shim's shape)
//         lazy       = fdnn_calculate_lazy_bits per utterance (one-call lazy scoring, 40 % of the nodes active per frame)
//         lazyserver = fdnn_server_submit_lazy_bits + fdnn_server_wait (bit-mask utterances coalesced, rows back compacted)
//         set        = fdnn_calculate_lazy_set per utterance: each caller its own node set of SET_LEN nodes (environment, 80)
//         setserver  = fdnn_server_submit_lazy_set + fdnn_server_wait (set utterances coalesced, no output layer, only
//                      probs [frames][SET_LEN] + inactive [frames] back)
//         topk       = fdnn_calculate_topk per utterance: the TOPK_K (environment, 32) best nodes of every frame, chosen on the
//                      device -- frames x TOPK_K x 8 bytes back instead of frames x output_dim x 4
//         topkserver = fdnn_server_submit_topk + fdnn_server_wait (top-k utterances coalesced, the dense rows stay on the device)
//         pool       = fdnn_calculate_pool per utterance: every frame's soft-max summed on the device over POOL_C (environment,
//                      48) classes of nodes (node i in class i mod POOL_C) -- frames x POOL_C x 4 bytes back
//         poolserver = fdnn_server_submit_pool + fdnn_server_wait (pool utterances of the one handle coalesced, the dense rows
//                      stay on the device)
//         loglik       = fdnn_calculate_loglik per utterance: every frame's soft-max as decoder scores ln p - log prior (uniform
//                        priors here, floor -30), computed on the device -- LOGLIK_TYPE (environment; 1 = fp16, the default,
//                        0 = fp32): frames x output_dim x 2 or 4 bytes back
//         loglikserver = fdnn_server_submit_loglik + fdnn_server_wait (loglik utterances of the one handle coalesced, the
//                        dense rows stay on the device, ONE transfer of the batch's scores)
//         live       = fdnn_stream_push: every feed its own stream, utterances of F raw frames (Kaldi +-5 x 39, set here) pushed in
//                      chunks of c frames, host-synchronous push by push
//         liveserver = fdnn_server_live_push + fdnn_server_wait: the same feeds through live handles of ONE scoring loop; a
//                      thread pushes the next chunk of each of its feeds, then waits for their tickets
//                      c is the trailing argument (default 10).  FEEDS=n (environment; default: one per thread): n feeds spread
//                      over the threads -- a few hundred live utterances are handles, not threads.
// SET_LEN=k with lazy / lazyserver: the masks are those sets (the same k nodes in every frame of a caller) instead of 40 %.
// INFLIGHT=k (environment, server modes): every caller keeps k utterances in flight (k result blocks per thread) instead of
// waiting for each one before submitting the next.
// Prints one JSON line.  Build: see tools/serve_bench.sh.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../include/fdnn.h"

// The live modes: n feeds over T threads, every feed U utterances of F raw frames in chunks of c.  One JSON line; push_us is
// the mean time from a feed's push to its rows being in the caller's memory.
static int run_live(fdnn_model *m, const std::string &mode, int T, int U, int F, int max_frames, int depth, int linger, int c) {
  const int feeds = std::max(T, std::getenv("FEEDS") ? std::atoi(std::getenv("FEEDS")) : T), RD = 39, R = 5;
  int offsets[11];
  for (int i = 0; i < 11; ++i) offsets[i] = i - 5;
  if (c < 1 || fdnn_model_set_splice(m, offsets, 11, RD)) {
    std::fprintf(stderr, "live: %s (c must be positive, the net's input must hold 11 x 39 columns)\n", fdnn_last_error());
    return 1;
  }
  const int O = fdnn_model_output_dim(m);
  const bool loop = mode == "liveserver";
  // POOL_C=C (environment): class sums [rows][C] come back instead of dense rows (node i in class i mod C) -- the stream scores
  // its hidden layers and pools through its context, the loop takes fdnn_server_live_push_pool
  const int pool_c = std::getenv("POOL_C") ? std::atoi(std::getenv("POOL_C")) : 0;
  fdnn_pool *pool = nullptr;
  if (pool_c > 0) {
    std::vector<int32_t> class_of(static_cast<size_t>(O));
    for (int i = 0; i < O; ++i) class_of[size_t(i)] = i % pool_c;
    if (!(pool = fdnn_pool_create(class_of.data(), O, pool_c))) {
      std::fprintf(stderr, "pool: %s\n", fdnn_last_error());
      return 1;
    }
  }
  const int W = pool ? pool_c : O;  // floats per returned row
  fdnn_server *srv = nullptr;
  if (loop && (fdnn_server_create(m, max_frames, depth, &srv) || fdnn_server_set_linger_us(srv, linger))) {
    std::fprintf(stderr, "server: %s\n", fdnn_last_error());
    return 1;
  }
  std::vector<fdnn_stream *> streams(size_t(feeds), nullptr);
  std::vector<fdnn_live *> lives(size_t(feeds), nullptr);
  std::vector<std::vector<float>> raw(static_cast<size_t>(feeds)), out(static_cast<size_t>(feeds));
  std::mt19937 rng(7);
  std::normal_distribution<float> nd(0.0f, 3.0f);
  for (int k = 0; k < feeds; ++k) {
    raw[size_t(k)].resize(size_t(F) * RD);
    for (float &v : raw[size_t(k)]) v = nd(rng);
    out[size_t(k)].assign(size_t(c + R) * size_t(W), 0.0f);
    if (loop ? fdnn_server_live_open(srv, c, &lives[size_t(k)]) : fdnn_stream_create(m, c, &streams[size_t(k)])) {
      std::fprintf(stderr, "feed %d: %s\n", k, fdnn_last_error());
      return 1;
    }
  }
  std::atomic<int> failed{0};
  std::atomic<long long> rows{0}, wait_ns{0}, pushes{0};
  auto body = [&](int t, int utts) {
    std::vector<uint64_t> tickets;
    std::vector<std::chrono::steady_clock::time_point> pushed;
    long long my_rows = 0, my_ns = 0, my_pushes = 0;
    for (int u = 0; u < utts; ++u) {
      for (int pos = 0; pos < F; pos += c) {
        const int n = std::min(c, F - pos), end = pos + c >= F;
        tickets.clear(), pushed.clear();
        for (int k = t; k < feeds; k += T) {
          int n_out = 0;
          uint64_t ticket = 0;
          const auto t0 = std::chrono::steady_clock::now();
          const float *chunk = raw[size_t(k)].data() + size_t(pos) * RD;
          float *o = out[size_t(k)].data();
          int rc;
          if (loop) {
            rc = pool ? fdnn_server_live_push_pool(lives[size_t(k)], chunk, n, end, pool, o, &n_out, &ticket)
                      : fdnn_server_live_push(lives[size_t(k)], chunk, n, end, o, &n_out, &ticket);
          } else {
            rc = fdnn_stream_push(streams[size_t(k)], chunk, n, end, pool ? nullptr : o, &n_out);
            if (!rc && pool && n_out > 0) rc = fdnn_ctx_output_pool(fdnn_stream_ctx(streams[size_t(k)]), pool, o);
          }
          if (rc) ++failed;
          my_rows += n_out, ++my_pushes;
          if (!loop) my_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
          if (ticket) tickets.push_back(ticket), pushed.push_back(t0);
        }
        for (size_t i = 0; i < tickets.size(); ++i) {
          if (fdnn_server_wait(srv, tickets[i])) ++failed;
          my_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - pushed[i]).count();
        }
      }
      for (int k = t; k < feeds; k += T)
        if (loop ? fdnn_server_live_reset(lives[size_t(k)]) : fdnn_stream_reset(streams[size_t(k)])) ++failed;
    }
    rows += my_rows, wait_ns += my_ns, pushes += my_pushes;
  };
  auto run = [&](int utts) {
    rows = 0, wait_ns = 0, pushes = 0;
    std::vector<std::thread> th;
    const auto t0 = std::chrono::steady_clock::now();
    for (int t = 0; t < T; ++t) th.emplace_back(body, t, utts);
    for (auto &x : th) x.join();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  };
  run(std::max(1, U / 10));  // warm-up
  const double sec = run(U);
  double sum = 0.0;  // the last row of feed 0's last push
  for (int i = 0; i < W; ++i) sum += out[0][size_t(i)];
  uint64_t batches = 0, frames = 0, reqs = 0, coal = 0;
  unsigned long long launches = 0, max_segs = 0;
  if (srv) fdnn_server_stats(srv, &batches, &frames, &reqs, &coal);
  fdnn_debug_live_launches(&launches, &max_segs);
  if (rows.load() != (long long)feeds * U * F) ++failed;  // every frame's row came back
  std::printf("{\"mode\": \"%s\", \"pool_c\": %d, \"threads\": %d, \"feeds\": %d, \"frames_per_utt\": %d, \"chunk\": %d, \"utts\": %d, \"seconds\": %.4f, "
              "\"frames_per_s\": %.1f, \"push_us\": %.1f, \"row0_sum\": %.6f, \"failed\": %d, \"batches\": %llu, \"requests\": %llu, "
              "\"max_segs\": %llu}\n",
              mode.c_str(), pool_c, T, feeds, F, c, feeds * U, sec, double(feeds) * U * F / sec, wait_ns.load() / 1e3 / double(std::max(1LL, pushes.load())),
              sum, failed.load(), (unsigned long long)batches, (unsigned long long)reqs, max_segs);
  for (int k = 0; k < feeds; ++k) {
    fdnn_server_live_close(lives[size_t(k)]);
    fdnn_stream_free(streams[size_t(k)]);
  }
  if (srv) fdnn_server_free(srv);
  fdnn_pool_free(pool);
  fdnn_model_free(m);
  return failed.load() ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: serve_bench model threads utts frames percall|server|batcher|live|liveserver|... [max_frames depth linger_us [c]]\n");
    return 2;
  }
  const char *path = argv[1];
  const int T = std::atoi(argv[2]), U = std::atoi(argv[3]), F = std::atoi(argv[4]);
  const std::string mode = argv[5];
  const int max_frames = argc > 6 ? std::atoi(argv[6]) : 6400, depth = argc > 7 ? std::atoi(argv[7]) : 3,
            linger = argc > 8 ? std::atoi(argv[8]) : 100;
  fdnn_model *m = nullptr;
  if (fdnn_model_load(path, 3.0f, &m)) {
    std::fprintf(stderr, "load: %s\n", fdnn_last_error());
    return 1;
  }
  if (mode == "live" || mode == "liveserver") return run_live(m, mode, T, U, F, max_frames, depth, linger, argc > 9 ? std::atoi(argv[9]) : 10);
  const int D = fdnn_model_input_dim(m), O = fdnn_model_output_dim(m);
  fdnn_server *srv = nullptr;
  const bool lazy = mode == "lazy" || mode == "lazyserver";
  const bool sets = mode == "set" || mode == "setserver";
  const int set_len = std::getenv("SET_LEN") ? std::atoi(std::getenv("SET_LEN")) : (sets ? 80 : 0);
  const bool topk = mode == "topk" || mode == "topkserver";
  const int topk_k = std::getenv("TOPK_K") ? std::atoi(std::getenv("TOPK_K")) : 32;
  const bool pooled = mode == "pool" || mode == "poolserver";
  const int pool_c = std::getenv("POOL_C") ? std::atoi(std::getenv("POOL_C")) : 48;
  const bool scored = mode == "loglik" || mode == "loglikserver";
  const int loglik_type = std::getenv("LOGLIK_TYPE") ? std::atoi(std::getenv("LOGLIK_TYPE")) : FDNN_LOGLIK_F16;
  if ((mode == "server" || mode == "lazyserver" || mode == "setserver" || mode == "topkserver" || mode == "poolserver" || mode == "loglikserver") && fdnn_server_create(m, max_frames, depth, &srv)) {
    std::fprintf(stderr, "server: %s\n", fdnn_last_error());
    return 1;
  }
  if (srv) fdnn_server_set_linger_us(srv, linger);
  if (mode == "batcher" && fdnn_model_enable_batcher(m, max_frames, depth, linger)) {
    std::fprintf(stderr, "batcher: %s\n", fdnn_last_error());
    return 1;
  }
  const int inflight = std::max(1, std::getenv("INFLIGHT") ? std::atoi(std::getenv("INFLIGHT")) : 1);
  std::vector<std::vector<float>> xs(static_cast<size_t>(T)), outs(static_cast<size_t>(T));
  std::vector<std::vector<std::vector<float>>> more(static_cast<size_t>(T));  // result blocks 1 .. inflight - 1 of a caller
  std::mt19937 rng(7);
  std::normal_distribution<float> nd(0.0f, 15.0f);
  for (int t = 0; t < T; ++t) {
    xs[size_t(t)].resize(size_t(F) * D);
    for (float &v : xs[size_t(t)]) v = nd(rng);
    outs[size_t(t)].assign(size_t(F) * O, 0.0f);  // resident, like a reused JVM float[]
    if (srv) more[size_t(t)].assign(size_t(inflight - 1), std::vector<float>(size_t(F) * O, 0.0f));
  }
  // lazy modes: per thread, masks with 40 % of the nodes active in every frame and 3 % churn from frame to frame
  // (FuncTest.java:121-154's statistics), as bits
  const size_t wpr = (size_t(O) + 63) / 64;
  std::vector<std::vector<uint64_t>> bits(static_cast<size_t>(T));
  // set modes (and lazy modes with SET_LEN): per thread one ascending set of set_len nodes, drawn without replacement
  std::vector<std::vector<int32_t>> nodes(static_cast<size_t>(T));
  std::vector<std::vector<float>> probs(static_cast<size_t>(T)), inact(static_cast<size_t>(T));
  if (set_len > 0) {
    if (set_len > O || (sets && inflight > 1)) {
      std::fprintf(stderr, "SET_LEN must be at most the output dimension; the set modes keep one utterance per caller in flight\n");
      return 1;
    }
    for (int t = 0; t < T; ++t) {
      std::vector<int32_t> perm(static_cast<size_t>(O));
      for (int i = 0; i < O; ++i) perm[size_t(i)] = i;
      std::shuffle(perm.begin(), perm.end(), rng);
      nodes[size_t(t)].assign(perm.begin(), perm.begin() + set_len);
      std::sort(nodes[size_t(t)].begin(), nodes[size_t(t)].end());
      probs[size_t(t)].assign(size_t(F) * size_t(set_len), 0.0f);
      inact[size_t(t)].assign(size_t(F), 0.0f);
    }
  }
  std::vector<std::vector<int32_t>> top_nodes(static_cast<size_t>(T));  // top-k modes: per thread [F][topk_k] nodes and values
  std::vector<std::vector<float>> top_probs(static_cast<size_t>(T));
  if (topk) {
    if (topk_k < 1 || topk_k > std::min(O, 256) || inflight > 1) {
      std::fprintf(stderr, "TOPK_K is 1 .. min(output dimension, 256); the top-k modes keep one utterance per caller in flight\n");
      return 1;
    }
    for (int t = 0; t < T; ++t) {
      top_nodes[size_t(t)].assign(size_t(F) * size_t(topk_k), 0);
      top_probs[size_t(t)].assign(size_t(F) * size_t(topk_k), 0.0f);
    }
  }
  fdnn_pool *pool = nullptr;  // pool modes: one handle for every caller, per thread [F][pool_c] class sums
  std::vector<std::vector<float>> pool_out(static_cast<size_t>(T));
  if (pooled) {
    std::vector<int32_t> class_of(static_cast<size_t>(O));
    for (int i = 0; i < O; ++i) class_of[size_t(i)] = pool_c > 0 ? i % pool_c : 0;
    if (inflight > 1 || !(pool = fdnn_pool_create(class_of.data(), O, pool_c))) {
      std::fprintf(stderr, "pool: %s (POOL_C is 1 .. output dimension; the pool modes keep one utterance per caller in flight)\n", fdnn_last_error());
      return 1;
    }
    for (int t = 0; t < T; ++t) pool_out[size_t(t)].assign(size_t(F) * size_t(pool_c), 0.0f);
  }
  fdnn_loglik *ll = nullptr;  // loglik modes: one handle for every caller, per thread [F][O] scores of 2 or 4 bytes
  std::vector<std::vector<uint16_t>> ll_out(static_cast<size_t>(T));
  const float ll_prior = -std::log(float(O));
  if (scored) {
    const std::vector<float> log_prior(static_cast<size_t>(O), ll_prior);
    if (inflight > 1 || !(ll = fdnn_loglik_create(log_prior.data(), O, -30.0f, loglik_type))) {
      std::fprintf(stderr, "loglik: %s (LOGLIK_TYPE is 0 or 1; the loglik modes keep one utterance per caller in flight)\n", fdnn_last_error());
      return 1;
    }
    for (int t = 0; t < T; ++t) ll_out[size_t(t)].assign(size_t(F) * size_t(O) * (loglik_type == FDNN_LOGLIK_F16 ? 1 : 2), 0);
  }
  if (lazy && set_len > 0) {
    for (int t = 0; t < T; ++t) {
      bits[size_t(t)].assign(size_t(F) * wpr, 0);
      for (int f = 0; f < F; ++f)
        for (int32_t i : nodes[size_t(t)]) bits[size_t(t)][size_t(f) * wpr + size_t(i >> 6)] |= uint64_t(1) << (i & 63);
    }
  } else if (lazy) {
    for (int t = 0; t < T; ++t) {
      std::vector<char> on(size_t(O), 0);
      std::vector<int> perm(static_cast<size_t>(O));
      for (int i = 0; i < O; ++i) perm[size_t(i)] = i;
      std::shuffle(perm.begin(), perm.end(), rng);
      const int active = int(O * 0.40), churn = int(O * 0.03);
      for (int i = 0; i < active; ++i) on[size_t(perm[size_t(i)])] = 1;
      bits[size_t(t)].assign(size_t(F) * wpr, 0);
      std::uniform_int_distribution<int> pick(0, O - 1);
      for (int f = 0; f < F; ++f) {
        if (f) {
          for (int c = 0, done = 0; done < churn && c < 100 * churn; ++c) { const int i = pick(rng); if (!on[size_t(i)]) { on[size_t(i)] = 1; ++done; } }
          for (int c = 0, done = 0; done < churn && c < 100 * churn; ++c) { const int i = pick(rng); if (on[size_t(i)]) { on[size_t(i)] = 0; ++done; } }
        }
        for (int i = 0; i < O; ++i)
          if (on[size_t(i)]) bits[size_t(t)][size_t(f) * wpr + size_t(i >> 6)] |= uint64_t(1) << (i & 63);
      }
    }
  }
  std::atomic<int> failed{0};
  static thread_local volatile float sink = 0.0f;
  auto body = [&](int t, int utts) {
    if (srv && inflight > 1) {  // a window of `inflight` tickets per caller
      std::vector<uint64_t> tk(size_t(inflight), 0);
      for (int u = 0; u < utts + inflight; ++u) {
        const size_t slot = size_t(u % inflight);
        if (u >= inflight && fdnn_server_wait(srv, tk[slot])) ++failed;
        if (u >= utts) continue;
        float *o = slot == 0 ? outs[size_t(t)].data() : more[size_t(t)][slot - 1].data();
        const int rc = lazy ? fdnn_server_submit_lazy_bits(srv, xs[size_t(t)].data(), F, bits[size_t(t)].data(), o, &tk[slot])
                            : fdnn_server_submit(srv, xs[size_t(t)].data(), F, nullptr, o, &tk[slot]);
        if (rc) ++failed;
      }
      return;
    }
    for (int u = 0; u < utts; ++u) {
      int rc;
      if (sets) {
        const std::vector<int32_t> &nd = nodes[size_t(t)];
        if (srv) {
          uint64_t ticket = 0;
          rc = fdnn_server_submit_lazy_set(srv, xs[size_t(t)].data(), F, nd.data(), set_len, probs[size_t(t)].data(), inact[size_t(t)].data(), &ticket);
          if (!rc) rc = fdnn_server_wait(srv, ticket);
        } else {
          rc = fdnn_calculate_lazy_set(m, xs[size_t(t)].data(), F, D, nd.data(), set_len, probs[size_t(t)].data(), inact[size_t(t)].data());
        }
      } else if (topk) {
        if (srv) {
          uint64_t ticket = 0;
          rc = fdnn_server_submit_topk(srv, xs[size_t(t)].data(), F, topk_k, top_nodes[size_t(t)].data(), top_probs[size_t(t)].data(), &ticket);
          if (!rc) rc = fdnn_server_wait(srv, ticket);
        } else {
          rc = fdnn_calculate_topk(m, xs[size_t(t)].data(), F, D, topk_k, top_nodes[size_t(t)].data(), top_probs[size_t(t)].data());
        }
      } else if (pooled) {
        if (srv) {
          uint64_t ticket = 0;
          rc = fdnn_server_submit_pool(srv, xs[size_t(t)].data(), F, pool, pool_out[size_t(t)].data(), &ticket);
          if (!rc) rc = fdnn_server_wait(srv, ticket);
        } else {
          rc = fdnn_calculate_pool(m, xs[size_t(t)].data(), F, D, pool, pool_out[size_t(t)].data());
        }
      } else if (scored) {
        if (srv) {
          uint64_t ticket = 0;
          rc = fdnn_server_submit_loglik(srv, xs[size_t(t)].data(), F, ll, ll_out[size_t(t)].data(), &ticket);
          if (!rc) rc = fdnn_server_wait(srv, ticket);
        } else {
          rc = fdnn_calculate_loglik(m, xs[size_t(t)].data(), F, D, ll, ll_out[size_t(t)].data());
        }
      } else if (srv && lazy) {
        uint64_t ticket = 0;
        rc = fdnn_server_submit_lazy_bits(srv, xs[size_t(t)].data(), F, bits[size_t(t)].data(), outs[size_t(t)].data(), &ticket);
        if (!rc) rc = fdnn_server_wait(srv, ticket);
      } else if (lazy) {
        rc = fdnn_calculate_lazy_bits(m, xs[size_t(t)].data(), F, D, bits[size_t(t)].data(), outs[size_t(t)].data());
      } else if (srv) {
        uint64_t ticket = 0;
        rc = fdnn_server_submit(srv, xs[size_t(t)].data(), F, nullptr, outs[size_t(t)].data(), &ticket);
        if (!rc) rc = fdnn_server_wait(srv, ticket);
      } else if (mode == "fresh") {  // the reference shim's shape: a new zero-filled result block per call (jni_dnn.cc:49-57)
        std::vector<float> fresh(size_t(F) * O);
        rc = fdnn_calculate(m, xs[size_t(t)].data(), F, D, 10, fresh.data());
        sink = sink + fresh[size_t(u) % fresh.size()];
      } else {
        rc = fdnn_calculate(m, xs[size_t(t)].data(), F, D, 10, outs[size_t(t)].data());
      }
      if (rc) ++failed;
    }
  };
  auto run = [&](int utts) {
    std::vector<std::thread> th;
    const auto t0 = std::chrono::steady_clock::now();
    for (int t = 0; t < T; ++t) th.emplace_back(body, t, utts);
    for (auto &x : th) x.join();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  };
  run(std::max(2, U / 10));  // warm-up: contexts, pinned staging, clocks
  const double sec = run(U);
  double sum = 0.0;
  for (int i = 0; i < O; ++i) sum += outs[0][size_t(i)];
  if (sets) {  // the same row as the lazy modes' row0_sum with SET_LEN: the listed nodes' probabilities + the others' inactive value
    sum = double(O - set_len) * inact[0][0];
    for (int j = 0; j < set_len; ++j) sum += probs[0][size_t(j)];
  }
  if (topk) {  // row 0's returned mass: the sum of its TOPK_K largest probabilities
    sum = 0.0;
    for (int j = 0; j < topk_k; ++j) sum += top_probs[0][size_t(j)];
  }
  if (pooled) {  // row 0's class sums: every node is in a class, so they add up to the row's total
    sum = 0.0;
    for (int j = 0; j < pool_c; ++j) sum += pool_out[0][size_t(j)];
  }
  if (scored) {  // row 0's scores back to probabilities: exp(s + log prior) adds up to the row's total (fp16: to three digits)
    sum = 0.0;
    for (int j = 0; j < O; ++j) {
      float sc;
      if (loglik_type == FDNN_LOGLIK_F16) {
        const uint16_t h = ll_out[0][size_t(j)];
        const int e = (h >> 10) & 31, f = h & 1023;
        sc = e == 0 ? std::ldexp(float(f), -24) : e == 31 ? (f ? NAN : INFINITY) : std::ldexp(float(f | 1024), e - 25);
        if (h & 0x8000) sc = -sc;
      } else {
        std::memcpy(&sc, reinterpret_cast<const char *>(ll_out[0].data()) + 4 * size_t(j), 4);
      }
      sum += std::exp(double(sc) + double(ll_prior));
    }
  }
  uint64_t batches = 0, frames = 0, reqs = 0, coal = 0;
  if (srv) fdnn_server_stats(srv, &batches, &frames, &reqs, &coal);
  std::printf("{\"mode\": \"%s\", \"threads\": %d, \"frames_per_utt\": %d, \"utts\": %d, \"seconds\": %.4f, \"utts_per_s\": %.1f, "
              "\"frames_per_s\": %.1f, \"row0_sum\": %.6f, \"failed\": %d, \"batches\": %llu, \"requests\": %llu}\n",
              mode.c_str(), T, F, T * U, sec, T * U / sec, double(T) * U * F / sec, sum, failed.load(), (unsigned long long)batches,
              (unsigned long long)reqs);
  if (srv) fdnn_server_free(srv);
  fdnn_pool_free(pool);
  fdnn_loglik_free(ll);
  fdnn_model_free(m);
  return failed.load() ? 1 : 0;
}
