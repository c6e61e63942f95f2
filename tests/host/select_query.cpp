// select_query.cpp -- the selection rules (fdnn_select.hpp) asked from a test: which kernel families will one pass launch?
// HIP-free like the header; tests/test_gpu_ctx_sequences.py builds it and predicts every step of its call sequences with
// it before asserting the prediction with the launch recorder.  One query per argument,
//   D,H,n_hid,O,has_fix,n,fuse,chain,ppo,l0_kernel,kind      kind: none | dense | bytes | bits
// (n_hid int8 hidden layers of width H behind the fp32 layer 0, an output layer of O nodes; fuse 0 / 1, chain 0 / 1 as
// fdnn_debug_set_chain(chain, 1), ppo -1 / 0 / 1, l0_kernel 0 .. 4; every layer with the validated division, 256 CUs,
// every other switch at its default), one line per query: the launch names' prefixes, blank-separated -- layer 0's, the hidden
// layers', the output layer's (none: no output launch), and "fused" or "unfused" for the output layer's soft-max.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "fdnn_select.hpp"

using namespace fdnn;
using namespace fdnn::sel;

namespace {
const char *shape_name(GemmShape s) {
  switch (s) {
    case gs_tdiv: return "tdiv";
    case gs_ft32w1: return "ft32.w1";
    case gs_ft32: return "ft32";
    case gs_ft64: return "ft64";
    case gs_ft128nt128: return "ft128.nt128";
    case gs_ft128bk128: return "ft128.bk128";
    case gs_ft128: return "ft128";
    case gs_ft256: return "ft256";
    case gs_ft320: return "ft320";
    default: return "ablation";
  }
}
int up(int v, int a) { return (v + a - 1) / a * a; }
}  // namespace

int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    int D, H, n_hid, O, has_fix, n, fuse, chain, ppo, l0k;
    char kind[16];
    if (std::sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%15s", &D, &H, &n_hid, &O, &has_fix, &n, &fuse, &chain, &ppo, &l0k, kind) != 11) {
      std::fprintf(stderr, "bad query: %s\n", argv[a]);
      return 2;
    }
    Tuning t;
    t.fuse_mode = fuse;
    t.chain_mode = chain;
    t.chain_min = chain == 1 ? 1 : 0;
    t.ppo_mode = ppo;
    const int h_ld = up(H, 128);
    std::string line;
    // ---- layer 0 (run_layer0: a full context has every scratch the kinds ask for; the planes where the shape allows them)
    const L0Call call{D, H, h_ld, n, n, false, l0k, false, true, true, l0_split_ok(D, H)};
    const L0Choice l0 = choose_l0(call, t);
    switch (l0.kind) {
      case L0Kind::mfma: line += "l0.mfma."; break;
      case L0Kind::small: line += "l0.small."; break;
      case L0Kind::split: line += "l0.digits l0.split.n" + std::to_string(64 * l0.split_wn) + " l0.fixlist.lpo" + std::to_string(l0.fix_lpo); break;
      case L0Kind::screened: line += "l0.screen.f128 l0.fix.tiles"; break;
      case L0Kind::chain: line += "l0.image.frames l0.chain."; break;
      case L0Kind::tile64: line += "l0.tile" + std::to_string(l0.tile) + "."; break;
    }
    // ---- the int8 hidden layers (run_hidden)
    const LayerShape hid{H, up(H, 256), up(H, 128), true, has_fix != 0, false};
    const HiddenPlan plan = plan_hidden(n_hid, [&](int) { return hid; }, n, true, t, {256});
    if (plan.chain) {
      line += " chain.ft" + std::to_string(plan.frame_tile) + ".";
    } else if (n_hid > 0) {
      const LayerChoice ch = choose_layer(hid, LayerCall{n}, t);
      if (ch.form == Form::small) line += " small.hid.nt" + std::to_string(32 * ch.small_ntm) + ".";
      else if (ch.form == Form::pp) line += " pp.hid.";
      else line += std::string(" gemm.hid.") + shape_name(ch.shape) + ".";
    }
    // ---- the output layer (run_output)
    const std::string k = kind;
    if (k != "none") {
      const LayerShape out{O, up(O, 256), up(H, 128), true, has_fix != 0, true};
      LayerCall c{n};
      c.byte_mask = k == "bytes";
      c.bit_mask = k == "bits";
      c.may_fuse = fuse == 1;
      const LayerChoice ch = choose_layer(out, c, t);
      if (ch.form == Form::small) line += " small.out.";
      else if (ch.form == Form::ppo) line += " ppo.out.";
      else line += std::string(" gemm.out.") + shape_name(ch.shape) + ".";
      line += ch.fused ? " fused" : " unfused";
    }
    std::printf("%s\n", line.c_str());
  }
  return 0;
}
