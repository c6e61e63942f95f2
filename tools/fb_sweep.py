"""Forward-backward over alignment graphs (fdnn_fb.hip): the kernels alone beside the best-path kernel on the same graphs, the
crossover of the two forms, and the whole call against today's way.

Kernel alone -- one segment of T rows of scores (64 columns, the states repeat them), optional-silence graphs of about S
states (words of 5 states), at the shapes of tools/align_graph_sweep.py (T in 100, 1000, 10 000, S in 40, 400, 1000, 4000,
T >= S, and 64 segments of 100 x 40 in one launch) and, for the FORM CROSSOVER that sets the rule, at 1000 x 32, 64, 96, 128,
192 and 256 states and at 64 segments of 100 x 64 and 300 x 128 in both forms:
  forward         fdnn_fb_rows_device without gamma: the log-add recursion and the total
  forward + back  the same with gamma: plus the lattice written, read back, and the backward sweep
  best path       fdnn_align_graph_rows_device (the rule's form) on the same graph: compare and select instead of a log-add
forward / best path is what the log-add costs; (forward + back) / (2 forward) what the lattice traffic and gamma add.
End to end on the 8000-node net, host frames in, total and gamma out, optional-silence transcripts:
  (a) today   fdnn_calculate_lazy_sets + the host logarithm (api.loglik_entries_ref) + fdnn_debug_fb_ref (plain C++)
  (b) device  fdnn_calculate_fb
at 64 utterances x 100 frames x 43 states in one call, and 1 utterance x 3000 frames x 995 states.

Alternated in one process: warm-up, then ROUNDS blocks per path, the paths taking turns; the figure is the median block's time
per call, the spread its (max - min) / median.  Before timing every path's bytes are compared with the host restatement.

  python tools/fb_sweep.py [--skip-model] [--skip-kernels] [--log FILE]

Prints one JSON line per shape and the tables, and writes both to the log (default profiles/fb_sweep.log)."""
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
    shapes = [(T, S, 1) for T in (100, 1000, 10000) for S in (40, 400, 1000, 4000) if T >= S] + [(100, 40, 64)]
    shapes += [(1000, S, 1) for S in (32, 64, 96, 128, 192, 256)] + [(100, 64, 64), (300, 128, 64)]  # (a graph of S states needs about S frames)
    wave_states = api.fb_limits()["wave_states"]
    for T, S, n_segs in shapes:
        rng = np.random.default_rng(T + S)
        rows = (0.5 * (3 * rng.standard_normal((n_segs * T, LD)) - 5)).astype(np.float32)
        d_rows = dev(rows, np.float32)
        seg_T, off, ld = [T] * n_segs, [i * T * LD for i in range(n_segs)], [LD] * n_segs
        g = api.pack_graphs([silence_graph(S, rng, LD) for _ in range(n_segs)])
        t = api.fb_transpose(g)
        col = g["states"]  # the states' nodes are their columns here
        n_states = int(g["statePtr"][1])
        rec = {"frames": T, "states": n_states, "arcs": int(g["arcPtr"][n_states]), "segments": n_segs}
        want = api.fb_ref(rows, seg_T, off, ld, g, col, transposed=t)
        assert np.isfinite(want[0]).all(), "a shape without a path measures nothing"
        bufs = [dev(col, np.int32), dev(g["arcPtr"], np.int32), dev(g["arcSrc"], np.int32), dev(g["arcLp"], np.float32), dev(g["startLp"], np.float32),
                dev(g["finalLp"], np.float32), dev(t["tPtr"], np.int32), dev(t["tSrc"], np.int32), dev(t["tLp"], np.float32)]
        cells = int(want[1].size)
        d_scr = torch.empty(max(cells, 2), dtype=torch.float32, device="cuda")
        d_gamma = torch.empty(max(cells, 2), dtype=torch.float32, device="cuda")
        d_total = torch.empty(n_segs, dtype=torch.float32, device="cuda")
        d_path = torch.empty(n_segs * T, dtype=torch.int32, device="cuda")
        runs = {}
        for name, mode in (("wave", 1), ("workgroup", 2)):
            if mode == 1 and n_states > wave_states:
                continue
            for what, gamma in (("fwd", False), ("fb", True)):

                def run(mode=mode, gamma=gamma):
                    api.set_fb_kernel(mode)
                    api.fb_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, g["statePtr"], g["arcPtr"], t["tPtr"] if gamma else None, bufs[0].data_ptr(), 0,
                                       bufs[1].data_ptr(), ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), ptr(bufs[5]), bufs[6].data_ptr() if gamma else 0,
                                       ptr(bufs[7]) if gamma else 0, ptr(bufs[8]) if gamma else 0, d_scr.data_ptr() if gamma else 0, cells if gamma else 0,
                                       d_total.data_ptr(), d_gamma.data_ptr() if gamma else 0, s)

                d_gamma.fill_(-9)
                for _ in range(3):
                    run()
                torch.cuda.synchronize()
                assert np.array_equal(d_total.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), f"{name} {what}: the total differs from the host restatement"
                if gamma:
                    assert np.array_equal(d_gamma.cpu().numpy()[:cells].view(np.uint32), want[1].view(np.uint32)), f"{name}: gamma differs from the host restatement"
                runs[f"{what}_{name}"] = run
        api.set_fb_kernel(0)
        words = api.align_graph_scratch_words(seg_T, g["statePtr"])
        b_scr = torch.empty(max(words, 2), dtype=torch.int32, device="cuda")

        def best_path():
            api.align_graph_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, g["statePtr"], g["arcPtr"], bufs[0].data_ptr(), 0, bufs[1].data_ptr(),
                                        ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), ptr(bufs[5]), b_scr.data_ptr() if words else 0, words, d_path.data_ptr(),
                                        d_total.data_ptr(), s)

        for _ in range(3):
            best_path()
        torch.cuda.synchronize()
        runs["best_path"] = best_path
        reps = 20 if n_segs * T * max(n_states, 64) <= 1_000_000 else 3
        for name, v in timed_blocks(torch, runs, reps).items():
            rec[name + "_us"], rec[name + "_spread"] = median_spread(v)
            rec[name + "_ns_per_frame"] = round(1000.0 * rec[name + "_us"] / T, 1)
        fwd = min(rec[k + "_us"] for k in ("fwd_wave", "fwd_workgroup") if k + "_us" in rec)
        fb = min(rec[k + "_us"] for k in ("fb_wave", "fb_workgroup") if k + "_us" in rec)
        rec["forward_over_best_path"] = round(fwd / rec["best_path_us"], 2)
        rec["fb_over_two_forwards"] = round(fb / (2 * fwd), 2)
        if "fb_wave_us" in rec:
            rec["wave_over_workgroup_fwd"] = round(rec["fwd_wave_us"] / rec["fwd_workgroup_us"], 2)
            rec["wave_over_workgroup_fb"] = round(rec["fb_wave_us"] / rec["fb_workgroup_us"], 2)
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
        for want_gamma in (True, False):

            def today():
                set_ptr, nodes, col = api.align_sets(ptr, states)
                probs = dnn.calculateLazySets(x, seg_rows, set_ptr, nodes)[0]
                ln = np.diff(set_ptr)
                off = np.concatenate([[0], np.cumsum(np.full(n_utt, T, np.int64) * ln)[:-1]])
                entry_nodes = np.concatenate([np.tile(nodes[set_ptr[i]:set_ptr[i + 1]], T) for i in range(n_utt)])
                e = api.loglik_entries_ref(entry_nodes, probs, lp, *handle)
                return api.fb_ref(e, [T] * n_utt, off, ln, packed, col, want_gamma=want_gamma), probs.nbytes

            def device():
                return dnn.calculateForwardBackward(x, ll, seg_rows, packed, want_gamma=want_gamma)

            (want, fetched), got = today(), device()
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "the total differs from today's way"
            assert not want_gamma or np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "gamma differs from today's way"
            assert np.isfinite(want[0]).all()
            ms = {"today": [], "device": []}
            reps = 5 if n_utt > 1 else 2
            for _ in range(ROUNDS):
                for name, f in (("today", today), ("device", device)):
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        f()
                    ms[name].append(1000.0 * (time.perf_counter() - t0) / reps)
            back = 4 * n_utt + (4 * got[1].size if want_gamma else 0)
            rec = {"utterances": n_utt, "frames": T, "states": int(ptr[1]), "gamma": want_gamma, "bytes_back_today": int(fetched), "bytes_back_device": int(back)}
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
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "fb_sweep.log"))
    args = ap.parse_args()
    kernels, calls = [], []
    if not args.skip_kernels:
        kernel_alone(torch, kernels)
    if not args.skip_model:
        end_to_end(calls)
    cell = lambda r, k: f"{r[k + '_us']} ({r[k + '_ns_per_frame']}, {r[k + '_spread']})" if k + "_us" in r else "-"
    if kernels:
        say("\nus per call (ns per frame, spread)")
        say("| frames | states | arcs | segments | forward wave | workgroup | forward + backward wave | workgroup | best path | forward / best path | fb / 2 forward |")
        say("|---|---|---|---|---|---|---|---|---|---|---|")
        for r in kernels:
            say(f"| {r['frames']} | {r['states']} | {r['arcs']} | {r['segments']} | {cell(r, 'fwd_wave')} | {cell(r, 'fwd_workgroup')} | {cell(r, 'fb_wave')} | "
                f"{cell(r, 'fb_workgroup')} | {cell(r, 'best_path')} | {r['forward_over_best_path']} | {r['fb_over_two_forwards']} |")
    if calls:
        say("\n| utterances | frames | states | gamma | (a) today ms | (b) device ms | (b) / (a) | bytes back (a) | (b) | spread (a) / (b) |")
        say("|---|---|---|---|---|---|---|---|---|---|")
        for r in calls:
            say(f"| {r['utterances']} | {r['frames']} | {r['states']} | {r['gamma']} | {r['today_ms']} | {r['device_ms']} | {r['device_over_today']} | "
                f"{r['bytes_back_today']} | {r['bytes_back_device']} | {r['today_spread']} / {r['device_spread']} |")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as fh:
        fh.write("\n".join(LOG) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
