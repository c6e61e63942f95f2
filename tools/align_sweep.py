"""Forced alignment (fdnn_align.hip): the kernels alone, and the whole call against today's way of aligning.

Kernel alone -- one segment of T rows of scores (64 columns, the states repeat them) and a transcript of S states, both forms
  wave       fdnn_align_rows_device under fdnn_debug_set_align_kernel(1)   (S <= 1024)
  workgroup  fdnn_align_rows_device under fdnn_debug_set_align_kernel(2)
over T in 100, 1000, 10 000 and S in 40, 400, 1000, 4000 (T >= S: a shorter segment has no path), and the flagship's 64
segments of 100 x 40 in one launch.
End to end on the 8000-node net, host frames in, path and total out:
  (a) today   fdnn_calculate_lazy_sets + the host logarithm (api.loglik_entries_ref) + fdnn_debug_align_ref (plain C++)
  (b) device  fdnn_calculate_align
at 64 utterances x 100 frames x 40 states in one call, and 1 utterance x 3000 frames x 1000 states.

Alternated in one process: warm-up, then ROUNDS blocks per path; the figure is the median block's time per call, the spread its
(max - min) / median.  Before timing every path's bytes are compared with the host restatement (api.align_ref).

  python tools/align_sweep.py [--skip-model] [--out FILE.json]

Prints one JSON line per shape and the tables."""
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


def median_spread(v):
    m = float(np.median(v))
    return round(m, 2), round((max(v) - min(v)) / m, 3)


def kernel_alone(torch, results):
    s = torch.cuda.current_stream().cuda_stream
    shapes = [(T, S, 1) for T in (100, 1000, 10000) for S in (40, 400, 1000, 4000) if T >= S] + [(100, 40, 64)]
    for T, S, n_segs in shapes:
        rng = np.random.default_rng(T + S)
        rows = (3 * rng.standard_normal((n_segs * T, LD)) - 5).astype(np.float32)
        col = rng.integers(0, LD, n_segs * S).astype(np.int32)
        u = rng.uniform(0.05, 0.95, n_segs * S)
        sl, nl = np.log(u).astype(np.float32), np.log(1 - u).astype(np.float32)
        seg_T, off, ld, sp = [T] * n_segs, [i * T * LD for i in range(n_segs)], [LD] * n_segs, [i * S for i in range(n_segs + 1)]
        want = api.align_ref(rows, seg_T, off, ld, sp, col, selfLp=sl, nextLp=nl)
        dev = lambda a: torch.from_numpy(a).cuda()
        d_rows, d_col, d_sl, d_nl = dev(rows), dev(col), dev(sl), dev(nl)
        d_path = torch.empty(n_segs * T, dtype=torch.int32, device="cuda")
        d_total = torch.empty(n_segs, dtype=torch.float32, device="cuda")
        rec = {"frames": T, "states": S, "segments": n_segs}
        us = {}
        for name, mode in (("wave", 1), ("workgroup", 2)):
            if mode == 1 and S > api.align_limits()["wave_states"]:
                continue
            api.set_align_kernel(mode)
            words = api.align_scratch_words(seg_T, sp)
            d_scr = torch.empty(max(words, 2), dtype=torch.int32, device="cuda")

            def run():
                api.align_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, sp, d_col.data_ptr(), 0, d_sl.data_ptr(), d_nl.data_ptr(),
                                      d_scr.data_ptr() if words else 0, words, d_path.data_ptr(), d_total.data_ptr(), s)

            d_path.fill_(-9)
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            assert np.array_equal(d_path.cpu().numpy(), want[0]) and np.array_equal(d_total.cpu().numpy().view(np.uint32), want[1].view(np.uint32)), \
                f"{name}: bytes differ from the host restatement"
            reps = 20 if T * max(S, 64) <= 1_000_000 else 3
            us[name] = []
            for _ in range(ROUNDS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run()
                e1.record()
                e1.synchronize()
                us[name].append(1000.0 * e0.elapsed_time(e1) / reps)
            rec["scratch_words_" + name] = words
        api.set_align_kernel(0)
        for name, v in us.items():
            rec[name + "_us"], rec[name + "_spread"] = median_spread(v)
            rec[name + "_ns_per_frame"] = round(1000.0 * rec[name + "_us"] / T, 1)
        results.append(rec)
        print(json.dumps(rec), flush=True)


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
    for n_utt, T, S in ((64, 100, 40), (1, 3000, 1000)):
        n = n_utt * T
        x = F.synth_features(n, dnn.inputDimension(), seed=n)
        seg_rows = np.arange(n_utt + 1, dtype=np.int32) * T
        ptr = np.arange(n_utt + 1, dtype=np.int32) * S
        states = rng.integers(0, O, n_utt * S).astype(np.int32)
        u = rng.uniform(0.05, 0.95, n_utt * S)
        sl, nl = np.log(u).astype(np.float32), np.log(1 - u).astype(np.float32)

        def today():
            set_ptr, nodes, col = api.align_sets(ptr, states)
            probs = dnn.calculateLazySets(x, seg_rows, set_ptr, nodes)[0]
            ln = np.diff(set_ptr)
            off = np.concatenate([[0], np.cumsum(np.full(n_utt, T, np.int64) * ln)[:-1]])
            entry_nodes = np.concatenate([np.tile(nodes[set_ptr[i]:set_ptr[i + 1]], T) for i in range(n_utt)])
            e = api.loglik_entries_ref(entry_nodes, probs, lp, *handle)
            return api.align_ref(e, [T] * n_utt, off, ln, ptr, col, selfLp=sl, nextLp=nl), probs.nbytes

        def device():
            return dnn.calculateAlign(x, ll, seg_rows, ptr, states, sl, nl)

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
        rec = {"utterances": n_utt, "frames": T, "states": S, "bytes_back_today": int(fetched), "bytes_back_device": int(4 * n + 4 * n_utt)}
        for name, v in ms.items():
            rec[name + "_ms"], rec[name + "_spread"] = median_spread(v)
        rec["device_over_today"] = round(rec["device_ms"] / rec["today_ms"], 3)
        results.append(rec)
        print(json.dumps(rec), flush=True)
    ll.delete()
    dnn.delete()


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    kernels, calls = [], []
    kernel_alone(torch, kernels)
    if not args.skip_model:
        end_to_end(calls)
    print("\n| frames | states | segments | wave us | ns / frame | workgroup us | ns / frame | spread wave / workgroup |")
    print("|---|---|---|---|---|---|---|---|")
    for r in kernels:
        print(f"| {r['frames']} | {r['states']} | {r['segments']} | {r.get('wave_us', '-')} | {r.get('wave_ns_per_frame', '-')} | {r['workgroup_us']} | "
              f"{r['workgroup_ns_per_frame']} | {r.get('wave_spread', '-')} / {r['workgroup_spread']} |")
    if calls:
        print("\n| utterances | frames | states | (a) today ms | (b) device ms | (b) / (a) | bytes back (a) | (b) | spread (a) / (b) |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in calls:
            print(f"| {r['utterances']} | {r['frames']} | {r['states']} | {r['today_ms']} | {r['device_ms']} | {r['device_over_today']} | "
                  f"{r['bytes_back_today']} | {r['bytes_back_device']} | {r['today_spread']} / {r['device_spread']} |")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"kernels": kernels, "calls": calls}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
