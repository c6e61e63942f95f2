"""The frames form of the best path over alignment graphs (fdnn_align_frames.hip) beside its two siblings on the same graphs,
and one push-by-push shape.

Kernel alone -- the shapes and graphs of tools/fb_frames_sweep.py (one segment of T rows of scores, 64 columns,
optional-silence graphs of about S states; T in 100, 1000, 10 000, S in 40, 400, 1000, 4000, T >= S; 64 segments of 100 x 40):
  free, anchored  fdnn_align_frames_rows_device: one launch, 12 bytes a frame written, no back-pointers, no scratch
  graph           fdnn_align_graph_rows_device: the best-path sibling, which stores T x S back-pointers and traces back
  fb_frames       fdnn_fb_frames_rows_device, free start: the summed sibling's sweep, lattice and row totals
free / graph is the aim (<= 1 within the larger spread); free / fb_frames is reported and not bounded.  All under the
rule's forms.
Push by push -- a 37-state graph scored in pushes of 10 frames with a free start, each call taking the call before's carry
in place: us per push.

Alternated in one process: three warm-up calls, then ROUNDS blocks per path, the paths taking turns; the figure is the median
block's time per call, the spread its (max - min) / median.  Before timing the frames path's bytes are compared with the host
restatement.

  python tools/align_frames_sweep.py [--log FILE]

Prints one JSON line per shape and the table, and writes both to the log (default profiles/align_frames_sweep.log)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api  # noqa: E402
from fb_frames_sweep import buffers  # noqa: E402
from fb_sweep import LD, LOG, median_spread, say, silence_graph, timed_blocks  # noqa: E402


def same(d_results, d_carry, want):
    got = [d.cpu().numpy() for d in d_results + d_carry]
    flat = (want[0].view(np.uint32), want[1], want[2], want[3][0].view(np.uint32), want[3][1])
    return all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, flat))


def kernel_alone(torch, results):
    s = torch.cuda.current_stream().cuda_stream
    shapes = [(T, S, 1) for T in (100, 1000, 10000) for S in (40, 400, 1000, 4000) if T >= S] + [(100, 40, 64)]
    for T, S, n_segs in shapes:
        rng = np.random.default_rng(T + S)
        rows = (0.5 * (3 * rng.standard_normal((n_segs * T, LD)) - 5)).astype(np.float32)
        d_rows = torch.from_numpy(rows).cuda()
        seg_T, off, ld = [T] * n_segs, [i * T * LD for i in range(n_segs)], [LD] * n_segs
        g = api.pack_graphs([silence_graph(S, rng, LD) for _ in range(n_segs)])
        n_states, all_states = int(g["statePtr"][1]), int(g["statePtr"][-1])
        p, keep = buffers(torch, g)
        rows_n, cells = n_segs * T, n_segs * T * n_states
        empty = lambda n, ty: torch.empty(max(n, 1), dtype=ty, device="cuda")
        d_res = [empty(rows_n, torch.float32), empty(rows_n, torch.int32), empty(rows_n, torch.int32)]
        d_carry = [empty(all_states, torch.float32), empty(all_states, torch.int32)]
        bp_words = api.align_graph_scratch_words(seg_T, g["statePtr"])
        d_bp, d_path, d_total = empty(bp_words, torch.int32), empty(rows_n, torch.int32), empty(n_segs, torch.float32)
        d_lat, d_tot, d_alpha = empty(cells, torch.float32), empty(rows_n, torch.float32), empty(all_states, torch.float32)
        base = list(range(0, 1000 * n_segs, 1000))

        def frames(free=True):
            api.align_frames_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, g["statePtr"], g["arcPtr"], p["col"], 0, p["ap"], p["src"], p["lp"], p["start"],
                                         p["final"], free, base, 0, 0, d_carry[0].data_ptr(), d_carry[1].data_ptr(), d_res[0].data_ptr(), d_res[1].data_ptr(),
                                         d_res[2].data_ptr(), s)

        def graph():
            api.align_graph_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, g["statePtr"], g["arcPtr"], p["col"], 0, p["ap"], p["src"], p["lp"], p["start"],
                                        p["final"], d_bp.data_ptr() if bp_words else 0, bp_words, d_path.data_ptr(), d_total.data_ptr(), s)

        def fb_frames():
            api.fb_frames_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, g["statePtr"], g["arcPtr"], p["col"], 0, p["ap"], p["src"], p["lp"], p["start"],
                                      p["final"], True, 0, d_alpha.data_ptr(), d_lat.data_ptr(), cells, d_tot.data_ptr(), s)

        runs = {"free": frames, "anchored": lambda: frames(False), "graph": graph, "fb_frames": fb_frames}
        for run in runs.values():
            for _ in range(3):
                run()
        for free in (False, True):
            frames(free)
            torch.cuda.synchronize()
            want = api.align_frames_ref(rows, seg_T, off, ld, g, g["states"], free_start=free, frame_base=base)
            assert np.isfinite(want[0][-1]), "a shape without a path measures nothing"
            assert same(d_res, d_carry, want), "the frames form differs from the host restatement"
        rec = {"frames": T, "states": n_states, "arcs": int(g["arcPtr"][n_states]), "segments": n_segs}
        reps = 20 if n_segs * T * max(n_states, 64) <= 1_000_000 else 3
        for name, v in timed_blocks(torch, runs, reps).items():
            rec[name + "_us"], rec[name + "_spread"] = median_spread(v)
        rec["free_over_graph"] = round(rec["free_us"] / rec["graph_us"], 3)
        rec["free_over_fb_frames"] = round(rec["free_us"] / rec["fb_frames_us"], 3)
        rec["margin"] = max(rec["free_spread"], rec["graph_spread"])
        rec["aim_met"] = bool(rec["free_over_graph"] <= 1 + rec["margin"] and rec["anchored_us"] / rec["graph_us"] <= 1 + max(rec["anchored_spread"], rec["graph_spread"]))
        results.append(rec)
        say(json.dumps(rec))
        del keep


def push_by_push(torch):
    s = torch.cuda.current_stream().cuda_stream
    T, pushes = 10, 100
    rng = np.random.default_rng(77)
    g = api.pack_graphs([silence_graph(40, rng, LD)])
    n_states = int(g["statePtr"][1])
    rows = (0.5 * (3 * rng.standard_normal((T * pushes, LD)) - 5)).astype(np.float32)
    d_rows = torch.from_numpy(rows).cuda()
    p, keep = buffers(torch, g)
    d_res = [torch.empty(T * pushes, dtype=ty, device="cuda") for ty in (torch.float32, torch.int32, torch.int32)]
    d_carry = [torch.empty(n_states, dtype=ty, device="cuda") for ty in (torch.float32, torch.int32)]

    def stream_once():
        for i in range(pushes):  # push i reads the carry push i - 1 wrote, in place
            cin = [d.data_ptr() if i else 0 for d in d_carry]
            api.align_frames_rows_device(None, d_rows.data_ptr() + 4 * i * T * LD, [T], [0], [LD], g["statePtr"], g["arcPtr"], p["col"], 0, p["ap"], p["src"],
                                         p["lp"], p["start"], p["final"], True, [i * T], cin[0], cin[1], d_carry[0].data_ptr(), d_carry[1].data_ptr(),
                                         d_res[0].data_ptr() + 4 * i * T, d_res[1].data_ptr() + 4 * i * T, d_res[2].data_ptr() + 4 * i * T, s)

    stream_once()
    torch.cuda.synchronize()
    want = api.align_frames_ref(rows, [T * pushes], [0], [LD], g, g["states"], free_start=True)
    assert same(d_res, d_carry, want), "the pushes differ from the one call's restatement"
    us, spread = median_spread([v / pushes for v in timed_blocks(torch, {"push": stream_once}, 3)["push"]])
    rec = {"push_frames": T, "states": n_states, "pushes": pushes, "us_per_push": us, "spread": spread, "bytes_written_per_push": 12 * T + 8 * n_states}
    say(json.dumps(rec))
    del keep
    return rec


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "align_frames_sweep.log"))
    args = ap.parse_args()
    results = []
    kernel_alone(torch, results)
    push = push_by_push(torch)
    say("\nus per call (spread)")
    say("| frames | states | arcs | segments | free | anchored | graph sibling | fb_frames | free / graph | margin | aim met | free / fb_frames |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        say(f"| {r['frames']} | {r['states']} | {r['arcs']} | {r['segments']} | {r['free_us']} ({r['free_spread']}) | {r['anchored_us']} ({r['anchored_spread']}) | "
            f"{r['graph_us']} ({r['graph_spread']}) | {r['fb_frames_us']} ({r['fb_frames_spread']}) | {r['free_over_graph']} | {r['margin']} | "
            f"{'yes' if r['aim_met'] else 'NO'} | {r['free_over_fb_frames']} |")
    say(f"\npush by push: {push['states']} states, pushes of {push['push_frames']} frames with carry in place: {push['us_per_push']} us per push "
        f"(spread {push['spread']}), {push['bytes_written_per_push']} bytes written per push")
    say("not measured: the entry points through a model, more than one device, the forced forms")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as fh:
        fh.write("\n".join(LOG) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
