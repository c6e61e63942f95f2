"""The decoder-score kernel (fdnn_loglik.hip) against two yardsticks on the same device rows: a device-to-device copy of the
rows (n x W x 4 bytes read and as many written, where the fp16 form writes half) and the same scores by torch
(log(rows) - log_prior, followed by .half() for the fp16 case -- torch's logarithm is another one: close, not the same bytes).

Device-resident soft-max rows [n][8000]; per (n, type) the kernel is timed in both forms,
  vector   fdnn_loglik_rows_device under fdnn_debug_set_loglik_kernel(1)   (16-byte loads and stores, priors in registers)
  scalar   fdnn_loglik_rows_device under fdnn_debug_set_loglik_kernel(2)   (element by element)
  copy     torch's device-to-device copy of the rows
  torch    torch.log(rows) - lp [, .half()]
alternated in one process: warm-up, then ROUNDS blocks per path of `reps` calls between two device events; the figure is the
median block's time per call, the spread its (max - min) / median.  Before timing, both forms' bytes are compared with each
other and with the host restatement (api.loglik_ref) on the first rows; the largest relative difference to torch's scores is
reported.

  python tools/loglik_sweep.py [--width 8000] [--batches 100,1000,10000] [--out FILE.json]

Prints one JSON line per (n, type) and the table."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api  # noqa: E402

ROUNDS = 5


def reps_for(n, width):
    return 200 if n * width <= 1_000_000 else 50 if n * width <= 10_000_000 else 10


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=8000)
    ap.add_argument("--batches", default="100,1000,10000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    s = torch.cuda.current_stream().cuda_stream
    width = args.width
    results = []
    rng = np.random.default_rng(5)
    z = rng.standard_normal(width) * 1.5
    lp = np.log(np.exp(z - z.max()) / np.exp(z - z.max()).sum()).astype(np.float32)
    d_lp = torch.from_numpy(lp).cuda()
    for n in [int(v) for v in args.batches.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(width + n)
        rows = torch.softmax(torch.randn((n, width), generator=g, device="cuda") * 3.0, dim=1).contiguous()
        dst = torch.empty_like(rows)
        head = rows[:4].cpu().numpy()
        for t, name in ((api.LOGLIK_F32, "f32"), (api.LOGLIK_F16, "f16")):
            ll = api.Loglik(lp, -30.0, t)
            tdt = torch.float16 if t == api.LOGLIK_F16 else torch.float32
            dq = [torch.empty((n, width), dtype=tdt, device="cuda") for _ in range(2)]
            keep = {}

            def run_kernel(mode, slot):
                api.set_loglik_kernel(mode)
                ll.rows_device(rows.data_ptr(), n, dq[slot].data_ptr(), s)

            def by_torch():
                v = torch.log(rows) - d_lp
                keep["torch"] = v.half() if t == api.LOGLIK_F16 else v

            runs = {"vector": lambda: run_kernel(1, 0), "scalar": lambda: run_kernel(2, 1), "copy": lambda: dst.copy_(rows), "torch": by_torch}
            before = api.loglik_launches()
            for _ in range(3):
                for f in runs.values():
                    f()
            torch.cuda.synchronize()
            after = api.loglik_launches()
            assert (after[0] - before[0], after[1] - before[1]) == (3, 3), "the modes did not select the two forms"
            it = torch.int16 if t == api.LOGLIK_F16 else torch.int32
            assert torch.equal(dq[0].view(it), dq[1].view(it)), "the two forms' bytes differ"
            want = api.loglik_ref(head, lp, -30.0, t)
            assert np.array_equal(dq[0][:4].cpu().numpy().view(want.dtype).view(np.uint16 if t else np.uint32), want.view(np.uint16 if t else np.uint32)), "bytes differ from the host restatement"
            ours, theirs = dq[0].double(), keep["torch"].double().clamp_min(-30.0)
            rel = float(((ours - theirs).abs() / theirs.abs().clamp_min(1e-3)).max())  # (reported, not asserted: another logarithm)
            reps = reps_for(n, width)
            us = {k: [] for k in runs}
            for _ in range(ROUNDS):
                for k, f in runs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        f()
                    e1.record()
                    e1.synchronize()
                    us[k].append(1000.0 * e0.elapsed_time(e1) / reps)
            out_mb = n * width * (2 if t == api.LOGLIK_F16 else 4) / 1e6
            rec = {"width": width, "frames": n, "type": name, "reps": reps, "in_mb": round(n * width * 4 / 1e6, 2), "out_mb": round(out_mb, 2)}
            for k, v in us.items():
                rec[k + "_us"] = round(float(np.median(v)), 2)
                rec[k + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 3)
            rec["vector_gb_s"] = round((rec["in_mb"] + out_mb) / rec["vector_us"] * 1000.0, 1)  # (MB / us = TB/s)
            rec["torch_max_rel_diff"] = float(f"{rel:.3g}")
            results.append(rec)
            print(json.dumps(rec), flush=True)
            ll.delete()
            keep.clear()
        rows = dst = None
    api.set_loglik_kernel(0)
    print("\n| frames | type | vector us | scalar us | copy us | torch us | vector / copy | vector GB/s | spread vec / sca / copy / torch |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in results:
        print(f"| {r['frames']} | {r['type']} | {r['vector_us']} | {r['scalar_us']} | {r['copy_us']} | {r['torch_us']} | {r['vector_us'] / r['copy_us']:.2f} | "
              f"{r['vector_gb_s']} | {r['vector_spread']} / {r['scalar_spread']} / {r['copy_spread']} / {r['torch_spread']} |")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
