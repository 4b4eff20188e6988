#!/usr/bin/env python3
"""Interleaved A/B of the two noise modes (include/ldpc_amd.h, ldpc_hip_set_noise): the reference's mt19937_64 stream
against the NON-PARITY counter-based mode, on the BASELINE configurations' parameters (libldpc_amd/workloads.py, read only).

    python tools/noise_ab.py [--configs 2,3,4,5,5bec] [--rounds 5] [--steps 20] [--warmup 5] [--out profiles/noise_modes.jsonl]

A round runs every mode once: stream_begin (seed 0), `warmup` steps, a synchronise, then `steps` timed steps of one batch
each (stream_decode into device buffers + the batch counters, as bench.py's step), timed by HIP events on the launch stream.
Per configuration and mode one JSON line: ms_per_step median and range over the rounds, frames/s at the median, FER and mean
iterations over every frame of the timed steps."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libldpc_amd import workloads  # noqa: E402

MODES = ("reference", "counter")


def run(cfg, rounds, steps, warmup):
    import torch
    import libldpc_amd
    w = workloads.get(cfg)
    dec = libldpc_amd.HipDecoder(workloads.code_path(w))
    dec.set_bec_compat(w.get("bec_compat", False))
    B, early, iters = w["batch"], w["early_term"], w["iterations"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"iters": torch.zeros(B, dtype=torch.int32, device=dev), "bit_errors": torch.zeros(B, dtype=torch.int32, device=dev)}
    c = torch.zeros(5, dtype=torch.int64, device=dev)
    res = {m: {"ms": [], "tot": torch.zeros(5, dtype=torch.int64, device=dev)} for m in MODES}

    def step(tot):
        dec.stream_decode(B, early_term=early, iterations=iters, decoding=w["decoding"], want=(), out=out, stream=stream)
        dec.batch_counters(out["iters"].data_ptr(), out["bit_errors"].data_ptr(), B, iters, early, c.data_ptr(), stream)
        if tot is not None:
            tot.add_(c)

    for _ in range(rounds):
        for m in MODES:
            dec.set_noise(m)
            dec.stream_begin(w["channel"], 0, w["x"])
            for _ in range(warmup):
                step(None)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(res[m]["tot"])
            e1.record()
            torch.cuda.synchronize()
            res[m]["ms"].append(e0.elapsed_time(e1) / steps)
    lines = []
    for m in MODES:
        ms, t = res[m]["ms"], res[m]["tot"].cpu().tolist()
        med = statistics.median(ms)
        lines.append({"config": cfg, "noise": m, "parity": m == "reference", "workload": w["name"], "batch": B,
                      "rounds": rounds, "steps": steps, "warmup": warmup, "ms_per_step_median": round(med, 4),
                      "ms_per_step_min": round(min(ms), 4), "ms_per_step_max": round(max(ms), 4),
                      "ms_per_step_rounds": [round(v, 4) for v in ms], "frames_per_s": round(B / med * 1e3),
                      "frames": t[0], "fer": t[1] / t[0], "avg_iter": t[3] / t[0]})
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="2,3,4,5,5bec")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_modes.jsonl"))
    args = ap.parse_args()
    lines = []
    for cfg in args.configs.split(","):
        for ln in run(cfg, args.rounds, args.steps, args.warmup):
            print(json.dumps(ln), flush=True)
            lines.append(ln)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
