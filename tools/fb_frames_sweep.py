"""The frames form of the summed alignment graphs (fdnn_fb_frames.hip): the sweep and its row totals beside two yardsticks on
the same graphs, and one push-by-push shape.

Kernel alone -- the shapes and graphs of tools/fb_sweep.py (one segment of T rows of scores, 64 columns, optional-silence
graphs of about S states; T in 100, 1000, 10 000, S in 40, 400, 1000, 4000, T >= S; and 64 segments of 100 x 40):
  frames          fdnn_fb_frames_rows_device, free start: the sweep that leaves the lattice, then the row totals
  forward         fdnn_fb_rows_device without gamma: no lattice, one total
  forward + back  the same with gamma: the lattice written, then read in a second SERIAL sweep
frames / (forward + back) is the aim (<= 1 within the larger spread); frames / forward is what the lattice stores and the row
totals cost, reported and not bounded.  All under the rule's forms.
Push by push -- a 37-state graph scored in pushes of 10 frames, each call taking the call before's alpha_out: us per push.

Alternated in one process: warm-up, then ROUNDS blocks per path, the paths taking turns; the figure is the median block's time
per call, the spread its (max - min) / median.  Before timing the frames path's bytes are compared with the host restatement.

  python tools/fb_frames_sweep.py [--log FILE]

Prints one JSON line per shape and the table, and writes both to the log (default profiles/fb_frames_sweep.log)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api  # noqa: E402
from fb_sweep import LD, LOG, median_spread, say, silence_graph, timed_blocks  # noqa: E402


def buffers(torch, g, t=None):
    dev = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, ty)).cuda()
    b = dict(col=dev(g["states"], np.int32), ap=dev(g["arcPtr"], np.int32), src=dev(g["arcSrc"], np.int32), lp=dev(g["arcLp"], np.float32),
             start=dev(g["startLp"], np.float32), final=dev(g["finalLp"], np.float32))
    if t is not None:
        b.update(tp=dev(t["tPtr"], np.int32), ts=dev(t["tSrc"], np.int32), tl=dev(t["tLp"], np.float32))
    return {k: v.data_ptr() for k, v in b.items()}, b  # (the tensors are kept alive by the caller)


def kernel_alone(torch, results):
    s = torch.cuda.current_stream().cuda_stream
    shapes = [(T, S, 1) for T in (100, 1000, 10000) for S in (40, 400, 1000, 4000) if T >= S] + [(100, 40, 64)]
    for T, S, n_segs in shapes:
        rng = np.random.default_rng(T + S)
        rows = (0.5 * (3 * rng.standard_normal((n_segs * T, LD)) - 5)).astype(np.float32)
        d_rows = torch.from_numpy(rows).cuda()
        seg_T, off, ld = [T] * n_segs, [i * T * LD for i in range(n_segs)], [LD] * n_segs
        g = api.pack_graphs([silence_graph(S, rng, LD) for _ in range(n_segs)])
        t = api.fb_transpose(g)
        n_states, all_states = int(g["statePtr"][1]), int(g["statePtr"][-1])
        p, keep = buffers(torch, g, t)
        cells = n_segs * T * n_states
        d_scr = torch.empty(cells, dtype=torch.float32, device="cuda")
        d_gamma = torch.empty(cells, dtype=torch.float32, device="cuda")
        d_total = torch.empty(n_segs, dtype=torch.float32, device="cuda")
        d_frames = torch.empty(n_segs * T, dtype=torch.float32, device="cuda")
        d_out = torch.empty(all_states, dtype=torch.float32, device="cuda")

        def frames():
            api.fb_frames_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, g["statePtr"], g["arcPtr"], p["col"], 0, p["ap"], p["src"], p["lp"], p["start"],
                                      p["final"], True, 0, d_out.data_ptr(), d_scr.data_ptr(), cells, d_frames.data_ptr(), s)

        def forward(gamma=False):
            api.fb_rows_device(None, d_rows.data_ptr(), seg_T, off, ld, g["statePtr"], g["arcPtr"], t["tPtr"] if gamma else None, p["col"], 0, p["ap"], p["src"],
                               p["lp"], p["start"], p["final"], p["tp"] if gamma else 0, p["ts"] if gamma else 0, p["tl"] if gamma else 0,
                               d_scr.data_ptr() if gamma else 0, cells if gamma else 0, d_total.data_ptr(), d_gamma.data_ptr() if gamma else 0, s)

        runs = {"frames": frames, "fwd": forward, "fb": lambda: forward(True)}
        for run in runs.values():
            for _ in range(3):
                run()
        frames()
        torch.cuda.synchronize()
        want = api.fb_frames_ref(rows, seg_T, off, ld, g, g["states"], free_start=True)
        assert np.isfinite(want[0][-1]), "a shape without a path measures nothing"
        assert np.array_equal(d_frames.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), "frame_total differs from the host restatement"
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want[1].view(np.uint32)), "alpha_out differs from the host restatement"
        rec = {"frames": T, "states": n_states, "arcs": int(g["arcPtr"][n_states]), "segments": n_segs}
        reps = 20 if n_segs * T * max(n_states, 64) <= 1_000_000 else 3
        for name, v in timed_blocks(torch, runs, reps).items():
            rec[name + "_us"], rec[name + "_spread"] = median_spread(v)
        rec["frames_over_fb"] = round(rec["frames_us"] / rec["fb_us"], 3)
        rec["frames_over_fwd"] = round(rec["frames_us"] / rec["fwd_us"], 3)
        rec["margin"] = max(rec["frames_spread"], rec["fb_spread"])
        rec["aim_met"] = bool(rec["frames_over_fb"] <= 1 + rec["margin"])
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
    d_scr = torch.empty(T * n_states, dtype=torch.float32, device="cuda")
    d_frames = torch.empty(T * pushes, dtype=torch.float32, device="cuda")
    d_carry = [torch.empty(n_states, dtype=torch.float32, device="cuda") for _ in range(2)]

    def stream_once():
        for i in range(pushes):  # push i reads the carry push i - 1 wrote
            api.fb_frames_rows_device(None, d_rows.data_ptr() + 4 * i * T * LD, [T], [0], [LD], g["statePtr"], g["arcPtr"], p["col"], 0, p["ap"], p["src"],
                                      p["lp"], p["start"], p["final"], True, d_carry[(i + 1) % 2].data_ptr() if i else 0, d_carry[i % 2].data_ptr(),
                                      d_scr.data_ptr(), T * n_states, d_frames.data_ptr() + 4 * i * T, s)

    stream_once()
    torch.cuda.synchronize()
    want = api.fb_frames_ref(rows, [T * pushes], [0], [LD], g, g["states"], free_start=True)
    assert np.array_equal(d_frames.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), "the pushes differ from the one call's restatement"
    us, spread = median_spread([v / pushes for v in timed_blocks(torch, {"push": stream_once}, 3)["push"]])
    rec = {"push_frames": T, "states": n_states, "pushes": pushes, "us_per_push": us, "spread": spread}
    say(json.dumps(rec))
    del keep
    return rec


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "fb_frames_sweep.log"))
    args = ap.parse_args()
    results = []
    kernel_alone(torch, results)
    push = push_by_push(torch)
    say("\nus per call (spread)")
    say("| frames | states | arcs | segments | frames form | forward only | forward + backward | frames / (forward + backward) | margin | frames / forward |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        say(f"| {r['frames']} | {r['states']} | {r['arcs']} | {r['segments']} | {r['frames_us']} ({r['frames_spread']}) | {r['fwd_us']} ({r['fwd_spread']}) | "
            f"{r['fb_us']} ({r['fb_spread']}) | {r['frames_over_fb']} | {r['margin']} | {r['frames_over_fwd']} |")
    say(f"\npush by push: {push['states']} states, pushes of {push['push_frames']} frames with carry: {push['us_per_push']} us per push (spread {push['spread']})")
    say("not measured: the entry points through a model, more than one device, the forced forms")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as fh:
        fh.write("\n".join(LOG) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
