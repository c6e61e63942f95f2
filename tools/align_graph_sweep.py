"""Alignment graphs (fdnn_align_graph.hip): the kernels alone beside the chain kernel, and the whole call against today's way.

Kernel alone -- one segment of T rows of scores (64 columns, the states repeat them), at the table shapes of
tools/align_sweep.py (T in 100, 1000, 10 000, S in 40, 400, 1000, 4000, T >= S, and 64 segments of 100 x 40 in one launch) and at
1000 x 64, 128 and 256, the wave form's 1, 2 and 4 states a lane up to its limit:
  chain graph     api.chain_graph of S states                       -> fdnn_align_graph_rows_device, wave and workgroup form
  silence graph   api.optional_silence_graph, words of 5 states, about S states in all   -> the same two forms
  chain kernel    fdnn_align_rows_device (the rule's form) on the same chain: the ratio graph / chain is what LDS costs
End to end on the 8000-node net, host frames in, path and total out, optional-silence transcripts:
  (a) today   fdnn_calculate_lazy_sets + the host logarithm (api.loglik_entries_ref) + fdnn_debug_align_graph_ref (plain C++)
  (b) device  fdnn_calculate_align_graph
at 64 utterances x 100 frames x 43 states in one call, and 1 utterance x 3000 frames x 995 states.

Alternated in one process: warm-up, then ROUNDS blocks per path, the paths taking turns; the figure is the median block's time
per call, the spread its (max - min) / median.  Before timing every path's bytes are compared with the host restatement.

  python tools/align_graph_sweep.py [--skip-model] [--log FILE]

Prints one JSON line per shape and the tables, and writes both to the log (default profiles/align_graph_sweep.log)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api, formats as F  # noqa: E402

ROUNDS = 5
LD = 64
LOG = []


def say(line=""):
    print(line, flush=True)
    LOG.append(line)


def median_spread(v):
    m = float(np.median(v))
    return round(m, 2), round((max(v) - min(v)) / m, 3)


def silence_graph(S, rng, n_cols):
    """About S states: words of 5 states and a silence (column 0) around each; arc scores ln U(0.05, 0.95)."""
    n_words = max(1, (S - 1) // 6)
    g = api.optional_silence_graph([rng.integers(1, n_cols, 5).tolist() for _ in range(n_words)], 0)
    g["arc_lp"] = np.log(rng.uniform(0.05, 0.95, g["arc_lp"].size)).astype(np.float32)
    return g


def timed_blocks(torch, runs, reps):
    """runs: name -> callable that enqueues one call -> name -> [us per call of each round], the paths taking turns."""
    us = {name: [] for name in runs}
    for _ in range(ROUNDS):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            e1.synchronize()
            us[name].append(1000.0 * e0.elapsed_time(e1) / reps)
    return us


def kernel_alone(torch, results):
    s = torch.cuda.current_stream().cuda_stream
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
    ptr = lambda d: d.data_ptr() if d is not None and d.numel() else 0
    shapes = [(T, S, 1) for T in (100, 1000, 10000) for S in (40, 400, 1000, 4000) if T >= S] + [(100, 40, 64)] + [(1000, S, 1) for S in (64, 128, 256)]
    for T, S, n_segs in shapes:
        rng = np.random.default_rng(T + S)
        rows = (3 * rng.standard_normal((n_segs * T, LD)) - 5).astype(np.float32)
        d_rows = dev(rows, np.float32)
        seg_T, off, ld = [T] * n_segs, [i * T * LD for i in range(n_segs)], [LD] * n_segs
        u = rng.uniform(0.05, 0.95, n_segs * S)
        sl, nl = np.log(u).astype(np.float32), np.log(1 - u).astype(np.float32)
        chain_col = rng.integers(0, LD, n_segs * S).astype(np.int32)
        kinds = {
            "chain": [api.chain_graph(chain_col[i * S:(i + 1) * S], sl[i * S:(i + 1) * S], nl[i * S:(i + 1) * S]) for i in range(n_segs)],
            "silence": [silence_graph(S, rng, LD) for _ in range(n_segs)],
        }
        rec = {"frames": T, "states": S, "segments": n_segs}
        runs, keep = {}, []
        d_path = torch.empty(n_segs * T, dtype=torch.int32, device="cuda")
        d_total = torch.empty(n_segs, dtype=torch.float32, device="cuda")
        for kind, graphs in kinds.items():
            g = api.pack_graphs(graphs)
            col = g["states"]  # the states' nodes are their columns here
            rec[kind + "_states"], rec[kind + "_arcs"] = int(g["statePtr"][1]), int(g["arcPtr"][g["statePtr"][1]])
            want = api.align_graph_ref(rows, seg_T, off, ld, g, col)
            assert np.isfinite(want[1]).all(), "a shape without a path measures nothing"
            bufs = [dev(col, np.int32), dev(g["arcPtr"], np.int32), dev(g["arcSrc"], np.int32), dev(g["arcLp"], np.float32),
                    dev(g["startLp"], np.float32) if g["startLp"] is not None else None, dev(g["finalLp"], np.float32) if g["finalLp"] is not None else None]
            keep.append(bufs)
            for name, mode in (("wave", 1), ("workgroup", 2)):
                if mode == 1 and rec[kind + "_states"] > api.align_graph_limits()["wave_states"]:
                    continue
                api.set_align_graph_kernel(mode)
                words = api.align_graph_scratch_words(seg_T, g["statePtr"])
                d_scr = torch.empty(max(words, 2), dtype=torch.int32, device="cuda")
                keep.append(d_scr)

                def run(mode=mode, g=g, bufs=bufs, d_scr=d_scr, words=words):
                    api.set_align_graph_kernel(mode)
                    api.align_graph_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, g["statePtr"], g["arcPtr"], bufs[0].data_ptr(), 0, bufs[1].data_ptr(),
                                                ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), ptr(bufs[5]), d_scr.data_ptr() if words else 0, words,
                                                d_path.data_ptr(), d_total.data_ptr(), s)

                d_path.fill_(-9)
                for _ in range(3):
                    run()
                torch.cuda.synchronize()
                assert np.array_equal(d_path.cpu().numpy(), want[0]) and np.array_equal(d_total.cpu().numpy().view(np.uint32), want[1].view(np.uint32)), \
                    f"{kind} {name}: bytes differ from the host restatement"
                runs[f"{kind}_{name}"] = run
        api.set_align_graph_kernel(0)
        # the chain kernel on the same chain
        sp = [i * S for i in range(n_segs + 1)]
        want = api.align_ref(rows, seg_T, off, ld, sp, chain_col, selfLp=sl, nextLp=nl)
        c_col, c_sl, c_nl = dev(chain_col, np.int32), dev(sl, np.float32), dev(nl, np.float32)
        c_words = api.align_scratch_words(seg_T, sp)
        c_scr = torch.empty(max(c_words, 2), dtype=torch.int32, device="cuda")

        def chain_kernel():
            api.align_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, sp, c_col.data_ptr(), 0, c_sl.data_ptr(), c_nl.data_ptr(),
                                  c_scr.data_ptr() if c_words else 0, c_words, d_path.data_ptr(), d_total.data_ptr(), s)

        for _ in range(3):
            chain_kernel()
        torch.cuda.synchronize()
        assert np.array_equal(d_path.cpu().numpy(), want[0]) and np.array_equal(d_total.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
        runs["chain_kernel"] = chain_kernel
        reps = 20 if T * max(S, 64) <= 1_000_000 else 3
        for name, v in timed_blocks(torch, runs, reps).items():
            rec[name + "_us"], rec[name + "_spread"] = median_spread(v)
            rec[name + "_ns_per_frame"] = round(1000.0 * rec[name + "_us"] / T, 1)
        best = min(rec[k + "_us"] for k in ("chain_wave", "chain_workgroup") if k + "_us" in rec)
        rec["chain_graph_over_chain_kernel"] = round(best / rec["chain_kernel_us"], 2)
        results.append(rec)
        say(json.dumps(rec))


def end_to_end(results):
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "fdnn_net_seed1_gauss.bin")
    F.ensure_model_file(path, F.NET_TOPOLOGY, seed=1, mode="gauss")
    dnn = api.QuantizedDnn.loadFromFile(path)
    O = dnn.outputDimension()
    rng = np.random.default_rng(7)
    z = rng.standard_normal(O) * 1.5
    lp = np.log(np.exp(z - z.max()) / np.exp(z - z.max()).sum()).astype(np.float32)
    handle = (-30.0, api.LOGLIK_F32)
    ll = api.Loglik(lp, *handle)
    for n_utt, T, n_words in ((64, 100, 6), (1, 3000, 142)):
        n = n_utt * T
        x = F.synth_features(n, dnn.inputDimension(), seed=n)
        seg_rows = np.arange(n_utt + 1, dtype=np.int32) * T
        graphs = []
        for _ in range(n_utt):
            g = api.optional_silence_graph([rng.integers(1, O, 6).tolist() for _ in range(n_words)], 0)
            g["arc_lp"] = np.log(rng.uniform(0.05, 0.95, g["arc_lp"].size)).astype(np.float32)
            graphs.append(g)
        packed = api.pack_graphs(graphs)
        ptr, states = packed["statePtr"], packed["states"]

        def today():
            set_ptr, nodes, col = api.align_sets(ptr, states)
            probs = dnn.calculateLazySets(x, seg_rows, set_ptr, nodes)[0]
            ln = np.diff(set_ptr)
            off = np.concatenate([[0], np.cumsum(np.full(n_utt, T, np.int64) * ln)[:-1]])
            entry_nodes = np.concatenate([np.tile(nodes[set_ptr[i]:set_ptr[i + 1]], T) for i in range(n_utt)])
            e = api.loglik_entries_ref(entry_nodes, probs, lp, *handle)
            return api.align_graph_ref(e, [T] * n_utt, off, ln, packed, col), probs.nbytes

        def device():
            return dnn.calculateAlignGraph(x, ll, seg_rows, packed)

        (want, fetched), got = today(), device()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "bytes differ from today's way"
        assert np.isfinite(want[1]).all()
        ms = {"today": [], "device": []}
        reps = 5 if n_utt > 1 else 2
        for _ in range(ROUNDS):
            for name, f in (("today", today), ("device", device)):
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                ms[name].append(1000.0 * (time.perf_counter() - t0) / reps)
        rec = {"utterances": n_utt, "frames": T, "states": int(ptr[1]), "bytes_back_today": int(fetched), "bytes_back_device": int(4 * n + 4 * n_utt)}
        for name, v in ms.items():
            rec[name + "_ms"], rec[name + "_spread"] = median_spread(v)
        rec["device_over_today"] = round(rec["device_ms"] / rec["today_ms"], 3)
        results.append(rec)
        say(json.dumps(rec))
    ll.delete()
    dnn.delete()


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "align_graph_sweep.log"))
    args = ap.parse_args()
    kernels, calls = [], []
    kernel_alone(torch, kernels)
    if not args.skip_model:
        end_to_end(calls)
    cell = lambda r, k: f"{r[k + '_us']} ({r[k + '_ns_per_frame']}, {r[k + '_spread']})" if k + "_us" in r else "-"
    say("\nus per call (ns per frame, spread)")
    say("| frames | states | segments | chain graph wave | workgroup | silence graph (states, arcs) wave | workgroup | chain kernel | chain graph / chain kernel |")
    say("|---|---|---|---|---|---|---|---|---|")
    for r in kernels:
        say(f"| {r['frames']} | {r['states']} | {r['segments']} | {cell(r, 'chain_wave')} | {cell(r, 'chain_workgroup')} | "
            f"({r['silence_states']}, {r['silence_arcs']}) {cell(r, 'silence_wave')} | {cell(r, 'silence_workgroup')} | {cell(r, 'chain_kernel')} | "
            f"{r['chain_graph_over_chain_kernel']} |")
    if calls:
        say("\n| utterances | frames | states | (a) today ms | (b) device ms | (b) / (a) | bytes back (a) | (b) | spread (a) / (b) |")
        say("|---|---|---|---|---|---|---|---|---|")
        for r in calls:
            say(f"| {r['utterances']} | {r['frames']} | {r['states']} | {r['today_ms']} | {r['device_ms']} | {r['device_over_today']} | "
                f"{r['bytes_back_today']} | {r['bytes_back_device']} | {r['today_spread']} / {r['device_spread']} |")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as fh:
        fh.write("\n".join(LOG) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
