#!/usr/bin/env python3
"""Fixed-point layered min-sum (include/ldpc_amd.h, ldpc_hip_set_min_sum_layered_fixed) against the other min-sum decoders on
the same frames: what int16 totals and 32-bit check-node records cost or buy in frames/s, sweeps and error rate.

    python tools/layered_fixed_min_sum_report.py [--rounds 3] [--steps 10] [--warmup 2] [--out profiles/layered_fixed_min_sum.jsonl]

Two workloads, both BP_MS, 50 iterations, early termination, counter-based noise (seed 0), so that every variant decodes the
same frames: h.txt at AWGN -4 dB, 65 536 frames per step (config 3's code), and the 8k (3,6) code at 2.0 dB, 8 192 frames per
step (config 4's point).  Five variants per workload — flooding binary64 min-sum (plain), layered binary64 at scale 0.8125,
flooding 6-bit at step 0.25 and scale 0.8125, layered fixed (6, 8, 0.25) and (5, 7, 0.5) at scale 0.8125 — interleaved: a
round runs every variant once (stream_begin, `warmup` steps, a synchronise, `steps` timed steps of stream_decode into device
buffers plus the batch counters, as bench.py's step, timed by HIP events).  One JSON line per workload and variant: ms per
step (median and range over the rounds), frames/s, mean sweeps (iterations), FER, LDS bytes per frame and frames per CU.
The yardsticks are the other variants of the same run.

Each workload runs in a child process of its own under a time limit; a workload that fails or runs out of time ends the
report there, and nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libldpc_amd import workloads  # noqa: E402

WORKLOADS = {"3": dict(early_term=True), "4": dict(decoding="BP_MS")}
# name, scale, then what is switched on: schedule / (bits, step) / (msg_bits, app_bits, step)
VARIANTS = [
    dict(decoder="flooding-binary64", scale=1.0),
    dict(decoder="layered-binary64", scale=0.8125, schedule="layered"),
    dict(decoder="flooding-quantized", scale=0.8125, quantization=(6, 0.25)),
    dict(decoder="layered-fixed", scale=0.8125, layered_fixed=(6, 8, 0.25)),
    dict(decoder="layered-fixed", scale=0.8125, layered_fixed=(5, 7, 0.5)),
]
LDS_PER_CU = 160 * 1024


def _switch(dec, v):
    """Everything off, then the variant's own switch (the setters refuse one another)."""
    dec.set_min_sum_schedule("flooding")
    dec.set_min_sum_quantization(0)
    dec.set_min_sum_layered_fixed(0)
    dec.set_min_sum_correction(v["scale"], 0.0)
    if "schedule" in v:
        dec.set_min_sum_schedule(v["schedule"])
    if "quantization" in v:
        dec.set_min_sum_quantization(*v["quantization"])
    if "layered_fixed" in v:
        dec.set_min_sum_layered_fixed(*v["layered_fixed"])


def _lds(dec, v):
    if "schedule" in v:
        return dec.layered_min_sum_lds_bytes()
    if "quantization" in v:
        return dec.quantized_min_sum_lds_bytes()
    if "layered_fixed" in v:
        return dec.layered_fixed_lds_bytes()
    return int(dec.lds_bytes)  # the resident decoder's own figure (registers, not LDS, bound the register-resident one)


def _steps(dec, w, B, n_steps, stream, out, c, tot):
    for _ in range(n_steps):
        dec.stream_decode(B, early_term=w["early_term"], iterations=w["iterations"], decoding=w["decoding"], want=(), out=out,
                          stream=stream)
        dec.batch_counters(out["iters"].data_ptr(), out["bit_errors"].data_ptr(), B, w["iterations"], w["early_term"],
                           c.data_ptr(), stream)
        if tot is not None:
            tot.add_(c)


def report(cfg, rounds, steps, warmup):
    import torch
    import libldpc_amd
    w = dict(workloads.get(cfg), **WORKLOADS[cfg])
    assert w["decoding"] == "BP_MS" and w["early_term"]
    dec = libldpc_amd.HipDecoder(workloads.code_path(w))
    dec.set_noise("counter")
    B = w["batch"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"iters": torch.zeros(B, dtype=torch.int32, device=dev), "bit_errors": torch.zeros(B, dtype=torch.int32, device=dev)}
    c = torch.zeros(5, dtype=torch.int64, device=dev)
    res = [{"ms": [], "tot": torch.zeros(5, dtype=torch.int64, device=dev)} for _ in VARIANTS]
    for _ in range(rounds):
        for v, r in zip(VARIANTS, res):
            _switch(dec, v)
            dec.stream_begin(w["channel"], 0, w["x"])
            _steps(dec, w, B, warmup, stream, out, c, None)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _steps(dec, w, B, steps, stream, out, c, r["tot"])
            e1.record()
            torch.cuda.synchronize()
            r["ms"].append(e0.elapsed_time(e1) / steps)
    lines = []
    for v, r in zip(VARIANTS, res):
        ms, t = r["ms"], r["tot"].cpu().tolist()
        med = statistics.median(ms)
        _switch(dec, v)
        lds = _lds(dec, v)
        lf = v.get("layered_fixed")
        lines.append({"config": cfg, "code": w["code"], "x": w["x"], "decoder": v["decoder"],
                      "decoder_choice": dec.decoder_choice(True, w["iterations"], "BP_MS"),
                      "msg_bits": lf[0] if lf else v.get("quantization", (None,))[0], "app_bits": lf[1] if lf else None,
                      "step": lf[2] if lf else v.get("quantization", (None, None))[1], "scale": v["scale"], "offset": 0.0,
                      "early_term": True, "iterations": w["iterations"], "noise": "counter", "seed": 0, "batch": B,
                      "rounds": rounds, "steps": steps, "warmup": warmup,
                      "ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms), 4),
                      "ms_per_step_max": round(max(ms), 4), "ms_per_step_rounds": [round(x, 4) for x in ms],
                      "frames_per_s": round(B / med * 1e3, 1), "frames": t[0], "fer": t[1] / t[0], "avg_sweeps": t[3] / t[0],
                      "lds_bytes_per_frame": lds,
                      "frames_per_cu_by_lds": LDS_PER_CU // lds if v["decoder"] != "flooding-binary64" else None,
                      "binary64_residency": dec.residency})
    by = {ln["decoder"]: ln["frames_per_s"] for ln in lines[:3]}
    for ln in lines:
        ln["frames_per_s_over_flooding_binary64"] = round(ln["frames_per_s"] / by["flooding-binary64"], 4)
        ln["frames_per_s_over_layered_binary64"] = round(ln["frames_per_s"] / by["layered-binary64"], 4)
        ln["frames_per_s_over_flooding_quantized"] = round(ln["frames_per_s"] / by["flooding-quantized"], 4)
    dec.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds one workload's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layered_fixed_min_sum.jsonl"))
    ap.add_argument("--workload", choices=sorted(WORKLOADS), help="(internal) run this workload here and print its lines")
    args = ap.parse_args()
    if args.workload:
        for ln in report(args.workload, args.rounds, args.steps, args.warmup):
            print(json.dumps(ln), flush=True)
        return 0
    lines = []
    for cfg in WORKLOADS:
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", cfg, "--rounds", str(args.rounds), "--steps", str(args.steps),
               "--warmup", str(args.warmup)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"workload {cfg}: no result within {args.limit} s; stopping here", file=sys.stderr)
            return 124
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"workload {cfg}: exit status {p.returncode}; stopping here", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        lines += [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
