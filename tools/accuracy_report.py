#!/usr/bin/env python3
"""Quantization error of the scorer against the fp32 net (the reference's FuncTest.diff notion:
per output node, |quantized - float| summed over the frames; nodes above 0.1 get printed there).

    python tools/accuracy_report.py model.bin [features.bin] [--frames N] [--cutoffs 2,3,4] [--device | --host]

--device (the default where a GPU is present): the float forward (api.FloatDnn), the quantized forward and the report
(api.AccuracyReport) all run on the device, chunk by chunk over the WHOLE feature file (or --frames synthetic frames);
nothing but the figures comes back.  --cutoffs a,b,c prints one report line per weight cut-off from ONE float pass.
--host is the numpy path (convert.float_forward, convert.quantization_report): a few thousand frames per second, so it
looks at the first --frames frames only (default 1000).  The quantized forward needs the GPU either way.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from fast_dnn_amd import api, convert as CV, formats as F  # noqa: E402

CHUNK = 4096  # frames per device pass: x, the float rows and the quantized rows of a chunk live on the device


def host_report(a, net, x):
    for cutoff in a.cutoffs:
        dnn = api.QuantizedDnn.loadFromFile(a.model, cutoff)
        q = dnn.calculate(x)
        dnn.delete()
        rep = CV.quantization_report(CV.float_forward(net, x[:, :net.layers[0].in_dim]), q)  # (x is padded to x4 for the scorer)
        print(json.dumps({"cutoff": cutoff, "path": "host", **rep}))


def device_report(a, x):
    import torch

    fdnn = api.FloatDnn.loadFromFile(a.model)
    O = fdnn.outputDimension()
    if x.shape[1] != fdnn.inputDimension():  # (fit_width's rule restated by the library that reads the rows)
        sys.exit(f"accuracy_report: Input vector size {x.shape[1]} must be equal with network input size {fdnn.inputDimension()}")
    qdnns = [api.QuantizedDnn.loadFromFile(a.model, c) for c in a.cutoffs]
    reps = [api.AccuracyReport(O) for _ in a.cutoffs]
    s = torch.cuda.current_stream().cuda_stream
    d_ref = torch.empty((min(CHUNK, len(x)), O), dtype=torch.float32, device="cuda")
    d_q = torch.empty_like(d_ref)
    for first in range(0, len(x), CHUNK):
        d_x = torch.from_numpy(x[first:first + CHUNK]).cuda()
        m = d_x.shape[0]
        fdnn.calculateDevice(d_x.data_ptr(), m, d_ref.data_ptr(), s)  # one float pass serves every cut-off
        for dnn, rep in zip(qdnns, reps):
            dnn.calculate_device(d_x.data_ptr(), m, d_q.data_ptr(), s)
            rep.addDevice(d_ref.data_ptr(), d_q.data_ptr(), m, s)
        torch.cuda.synchronize()  # d_x is released below
    for cutoff, dnn, rep in zip(a.cutoffs, qdnns, reps):
        out = rep.read(0.1)
        print(json.dumps({"cutoff": cutoff, "path": "device", **out}))
        rep.delete()
        dnn.delete()
    fdnn.delete()


def fit_width(x, in_dim_file, dim):
    """The frames at the width both nets read, `dim` = the model's input width padded to x4 (float_dnn.cc:32-33): rows of the
    file's own width are zero-padded as the loader pads the weights; any other width is not this model's feature file.  The
    device entry points take raw pointers and check nothing, so this is the one place that can."""
    if x.ndim != 2 or x.shape[1] not in (in_dim_file, dim):
        sys.exit(f"accuracy_report: Input vector size {x.shape[-1]} must be equal with network input size {dim}"
                 + (f" (or the model file's {in_dim_file})" if in_dim_file != dim else ""))
    if x.shape[1] < dim:
        x = np.concatenate((x, np.zeros((x.shape[0], dim - x.shape[1]), np.float32)), axis=1)
    return np.ascontiguousarray(x, dtype=np.float32)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("model")
    ap.add_argument("features", nargs="?")
    ap.add_argument("--frames", type=int, default=None, help="synthetic frames when no feature file is given; with --host, the frames looked at (default 1000)")
    ap.add_argument("--cutoffs", default="3", help="weight cut-offs of fdnn_model_load, comma separated (default 3)")
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--device", action="store_true", help="everything on the device (default where a GPU is present)")
    mode.add_argument("--host", action="store_true", help="the float forward and the report in numpy")
    a = ap.parse_args()
    a.cutoffs = [float(v) for v in a.cutoffs.split(",")]
    net = F.read_model_bin(a.model)
    dim = -(-net.layers[0].in_dim // 4) * 4
    frames = a.frames if a.frames is not None else 1000
    x = F.read_feature_bin(a.features) if a.features else F.synth_features(frames, dim, seed=3)
    x = fit_width(x, net.layers[0].in_dim, dim)
    if api.device_count() < 1:
        sys.exit("accuracy_report: the quantized scorer needs a HIP device (no CPU path)")
    if a.host:
        host_report(a, net, x[:frames])
    else:
        device_report(a, x if a.frames is None or not a.features else x[:frames])


if __name__ == "__main__":
    main()
