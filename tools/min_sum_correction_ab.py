#!/usr/bin/env python3
"""Corrected min-sum (include/ldpc_amd.h, ldpc_hip_set_min_sum_correction): interleaved A/B of plain BP_MS against the
normalized form, and a frame-error / mean-iteration table of BP, BP_MS, NMS and OMS.

    python tools/min_sum_correction_ab.py ab  [--rounds 5] [--steps 20] [--warmup 5] [--out profiles/min_sum_correction_ab.jsonl]
    python tools/min_sum_correction_ab.py fer [--frames 65536] [--out profiles/min_sum_correction_fer.jsonl]

ab: config 3's workload (h.txt, AWGN -4 dB, BP_MS, 50 iterations, no early termination, 65 536 frames per step;
libldpc_amd/workloads.py) and the 8k code at 2.0 dB with early termination (config 4's point, BP_MS), each plain and with
scale 0.75, interleaved: a round runs both once (stream_begin seed 0, `warmup` steps, a synchronise, `steps` timed steps of
stream_decode into device buffers plus the batch counters, as bench.py's step, timed by HIP events).  One JSON line per
workload and rule: ms per step median and range over the rounds, FER and mean iterations over the timed frames.

fer: counter-based noise (seed 1), three channel points per code, `frames` frames per point and rule."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libldpc_amd import workloads  # noqa: E402

AB = [("3", dict()), ("4", dict(decoding="BP_MS"))]
RULES_AB = [("BP_MS", 1.0, 0.0), ("NMS 0.75", 0.75, 0.0)]
RULES_FER = [("BP", None, None), ("BP_MS", 1.0, 0.0), ("NMS 0.75", 0.75, 0.0), ("NMS 0.8125", 0.8125, 0.0),
             ("OMS 0.25", 1.0, 0.25), ("OMS 0.5", 1.0, 0.5)]
POINTS = {"h": [-5.0, -4.5, -4.0], "8k": [1.4, 1.6, 1.8]}


def _steps(dec, w, B, n_steps, stream, out, c, tot):
    for _ in range(n_steps):
        dec.stream_decode(B, early_term=w["early_term"], iterations=w["iterations"], decoding=w["decoding"], want=(), out=out,
                          stream=stream)
        dec.batch_counters(out["iters"].data_ptr(), out["bit_errors"].data_ptr(), B, w["iterations"], w["early_term"],
                           c.data_ptr(), stream)
        if tot is not None:
            tot.add_(c)


def ab(cfg, over, rounds, steps, warmup):
    import torch
    import libldpc_amd
    w = dict(workloads.get(cfg), **over)
    dec = libldpc_amd.HipDecoder(workloads.code_path(w))
    B = w["batch"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"iters": torch.zeros(B, dtype=torch.int32, device=dev), "bit_errors": torch.zeros(B, dtype=torch.int32, device=dev)}
    c = torch.zeros(5, dtype=torch.int64, device=dev)
    res = {r[0]: {"ms": [], "tot": torch.zeros(5, dtype=torch.int64, device=dev)} for r in RULES_AB}
    for _ in range(rounds):
        for name, s, o in RULES_AB:
            dec.set_min_sum_correction(s, o)
            dec.stream_begin(w["channel"], 0, w["x"])
            _steps(dec, w, B, warmup, stream, out, c, None)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _steps(dec, w, B, steps, stream, out, c, res[name]["tot"])
            e1.record()
            torch.cuda.synchronize()
            res[name]["ms"].append(e0.elapsed_time(e1) / steps)
    lines = []
    for name, s, o in RULES_AB:
        ms, t = res[name]["ms"], res[name]["tot"].cpu().tolist()
        med = statistics.median(ms)
        lines.append({"config": cfg, "rule": name, "scale": s, "offset": o, "code": w["code"], "x": w["x"],
                      "early_term": w["early_term"], "batch": B, "rounds": rounds, "steps": steps, "warmup": warmup,
                      "ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms), 4),
                      "ms_per_step_max": round(max(ms), 4), "ms_per_step_rounds": [round(v, 4) for v in ms],
                      "frames": t[0], "fer": t[1] / t[0], "avg_iter": t[3] / t[0]})
    base = lines[0]["ms_per_step_median"]
    for ln in lines:
        ln["ratio_to_plain"] = round(ln["ms_per_step_median"] / base, 4)
    return lines


def fer(frames):
    import numpy as np
    import libldpc_amd
    lines = []
    for code, cfg in (("h", "3"), ("8k", "4")):
        w = workloads.get(cfg)
        dec = libldpc_amd.HipDecoder(workloads.code_path(w))
        dec.set_noise("counter")
        B = min(frames, 65536 if code == "h" else 8192)
        for x in POINTS[code]:
            for name, s, o in RULES_FER:
                dec.set_min_sum_correction(s or 1.0, o or 0.0)
                dec.stream_begin("AWGN", 1, x)
                it, be = [], []
                for _ in range(frames // B):
                    r = dec.stream_decode(B, early_term=True, iterations=50, decoding="BP" if s is None else "BP_MS")
                    it.append(r["iters"]), be.append(r["bit_errors"])
                it, be = np.concatenate(it).astype(np.float64), np.concatenate(be)
                p = float((be > 0).mean())
                lines.append({"code": code, "x": x, "rule": name, "scale": s, "offset": o, "frames": int(be.size),
                              "fer": p, "fer_se": float(np.sqrt(p * (1 - p) / be.size)), "avg_iter": float(it.mean()),
                              "early_term": True, "iterations": 50, "noise": "counter", "seed": 1})
                print(json.dumps(lines[-1]), flush=True)
        dec.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("what", choices=("ab", "fer"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    if args.what == "ab":
        for cfg, over in AB:
            for ln in ab(cfg, over, args.rounds, args.steps, args.warmup):
                print(json.dumps(ln), flush=True)
                lines.append(ln)
    else:
        lines = fer(args.frames)
    out = args.out or os.path.join(ROOT, "profiles", f"min_sum_correction_{args.what}.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
