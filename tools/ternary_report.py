#!/usr/bin/env python3
"""Ternary min-sum (include/ldpc_amd.h, ldpc_hip_set_min_sum_ternary) against flooding binary64 min-sum and 2-bit quantized
min-sum on the same frames, and the bit-sliced erasure kernel's frames/s on the same box: what a bit-sliced ternary kernel
costs or buys in frames/s, kernel time, iterations and error rate.

    python tools/ternary_report.py [--rounds 3] [--steps 20] [--warmup 3] [--out profiles/ternary.jsonl]

Two BSC workloads, both BP_MS, 50 iterations, early termination, counter-based noise (seed 0), so that every decoder decodes
the same frames, 65 536 frames per step: the (3,6)-regular code of 2048 columns (tools/gen_regular_code.generate(2048, 3, 6,
1)) at eps = 0.03 with channel weight 1, and the (4,8)-regular code of 1024 columns (generate(1024, 4, 8, 2)) at eps = 0.03
with weight 2.  Three decoders per workload — ternary, binary64 flooding min-sum, quantized min-sum with 2 bits at step 2.0
— interleaved: a round runs every decoder once (stream_begin, `warmup` steps, a synchronise, `steps` timed steps of
stream_decode into device buffers plus the batch counters, as bench.py's step, timed by HIP events; the decode launches'
own time from ldpc_hip_last_ms).  A third workload is the erasure decoder on h.txt at eps = 0.7 (configuration 5bec), the
one other bit-sliced kernel.  One JSON line per workload and decoder: ms per step (median and range over the rounds),
kernel ms, frames/s, mean iterations, FER, and the device's name.

Each workload runs in a child process of its own under a time limit; a workload that fails or runs out of time ends the
report there, and nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libldpc_amd import workloads  # noqa: E402

# key -> (nc, dv, dc, code seed, channel weight, eps)
WORKLOADS = {"r36_2048": (2048, 3, 6, 1, 1, 0.03), "r48_1024": (1024, 4, 8, 2, 2, 0.03), "bec": None}
DECODERS = ("ternary", "binary64", "quantized2")
BATCH, ITERATIONS = 65536, 50


def _code_file(nc, dv, dc, seed):
    import gen_regular_code
    path = os.path.join(tempfile.gettempdir(), f"ldpc_amd_r{nc}_{dv}_{dc}_{seed}_{os.getuid()}.txt")
    if not os.path.exists(path):
        tmp = f"{path}.{os.getpid()}"
        with open(tmp, "w") as f:
            f.write(gen_regular_code.generate(nc, dv, dc, seed))
        os.replace(tmp, path)
    return path


def _switch(dec, which, weight):
    dec.set_min_sum_ternary(0)
    dec.set_min_sum_quantization(0)
    if which == "ternary":
        dec.set_min_sum_ternary(weight)
    elif which == "quantized2":
        dec.set_min_sum_quantization(2, 2.0)


def _steps(dec, B, channel_args, n_steps, stream, out, c, tot):
    for _ in range(n_steps):
        dec.stream_decode(B, want=(), out=out, stream=stream, **channel_args)
        dec.batch_counters(out["iters"].data_ptr(), out["bit_errors"].data_ptr(), B, ITERATIONS, True, c.data_ptr(), stream)
        if tot is not None:
            tot.add_(c)


def report(key, rounds, steps, warmup):
    import torch
    import libldpc_amd
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    stream = torch.cuda.current_stream().cuda_stream
    if WORKLOADS[key] is None:
        w = workloads.get("5bec")
        dec = libldpc_amd.HipDecoder(workloads.code_path(w))
        dec.set_bec_compat(True)
        variants, weight, channel, x, code = ("bec",), 0, "BEC", w["x"], "h.txt"
        dargs = dict(early_term=True, iterations=ITERATIONS, decoding="BP")
    else:
        nc, dv, dc, cseed, weight, x = WORKLOADS[key]
        dec = libldpc_amd.HipDecoder(_code_file(nc, dv, dc, cseed))
        variants, channel, code = DECODERS, "BSC", f"({dv},{dc})-regular nc={nc} (tools/gen_regular_code.py seed {cseed})"
        dargs = dict(early_term=True, iterations=ITERATIONS, decoding="BP_MS")
    dec.set_noise("counter")
    dec.set_profiling(True)
    B = BATCH
    out = {"iters": torch.zeros(B, dtype=torch.int32, device=dev), "bit_errors": torch.zeros(B, dtype=torch.int32, device=dev)}
    c = torch.zeros(5, dtype=torch.int64, device=dev)
    res = {v: {"ms": [], "kernel_ms": [], "tot": torch.zeros(5, dtype=torch.int64, device=dev)} for v in variants}
    for _ in range(rounds):
        for v in variants:
            if v != "bec":
                _switch(dec, v, weight)
            dec.stream_begin(channel, 0, x)
            _steps(dec, B, dargs, warmup, stream, out, c, None)
            torch.cuda.synchronize()
            dec.last_ms(0)  # (the warm-up's launches are not in the mean)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _steps(dec, B, dargs, steps, stream, out, c, res[v]["tot"])
            e1.record()
            torch.cuda.synchronize()
            res[v]["ms"].append(e0.elapsed_time(e1) / steps)
            res[v]["kernel_ms"].append(dec.last_ms(0))
    lines = []
    for v in variants:
        ms, t = res[v]["ms"], res[v]["tot"].cpu().tolist()
        med = statistics.median(ms)
        lines.append({"workload": key, "code": code, "channel": channel, "x": x, "decoder": v,
                      "weight": weight if v == "ternary" else None, "early_term": True, "iterations": ITERATIONS,
                      "noise": "counter", "seed": 0, "batch": B, "rounds": rounds, "steps": steps, "warmup": warmup,
                      "ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms), 4),
                      "ms_per_step_max": round(max(ms), 4), "ms_per_step_rounds": [round(m, 4) for m in ms],
                      "kernel_ms_median": round(statistics.median(res[v]["kernel_ms"]), 4),
                      "frames_per_s": round(B / med * 1e3, 1), "frames": t[0], "fer": t[1] / t[0], "avg_iter": t[3] / t[0],
                      "ternary_lds_bytes_per_group": dec.ternary_lds_bytes() if v == "ternary" else None, "box": box})
    by = {ln["decoder"]: ln["frames_per_s"] for ln in lines}
    if "binary64" in by:
        for ln in lines:
            ln["frames_per_s_over_binary64"] = round(ln["frames_per_s"] / by["binary64"], 4)
    dec.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds one workload's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ternary.jsonl"))
    ap.add_argument("--workload", choices=sorted(WORKLOADS), help="(internal) run this workload here and print its lines")
    args = ap.parse_args()
    if args.workload:
        for ln in report(args.workload, args.rounds, args.steps, args.warmup):
            print(json.dumps(ln), flush=True)
        return 0
    lines = []
    for key in WORKLOADS:
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", key, "--rounds", str(args.rounds), "--steps", str(args.steps),
               "--warmup", str(args.warmup)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"workload {key}: no result within {args.limit} s; stopping here", file=sys.stderr)
            return 124
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"workload {key}: exit status {p.returncode}; stopping here", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        lines += [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    bec = [ln["frames_per_s"] for ln in lines if ln["decoder"] == "bec"]
    for ln in lines:
        ln["frames_per_s_over_bec_sliced"] = round(ln["frames_per_s"] / bec[0], 4) if bec else None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
