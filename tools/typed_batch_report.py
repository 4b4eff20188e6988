#!/usr/bin/env python3
"""decode_batch on binary64 device LLRs against decode_batch_typed on int8 and float32 device LLRs of the same frames
(include/ldpc_amd.h, ldpc_hip_decode_batch_typed): what the direct form of fixed-point layered min-sum — no binary64 staging
area in LDS, 25 instead of 17 frames of h.txt per CU, four instead of two of the 8k code — buys or costs.

    python tools/typed_batch_report.py [--rounds 5] [--steps 10] [--warmup 2] [--out profiles/typed_batch.jsonl]

Settings: BP_MS, fixed-point layered (6, 8, 0.25) at scale 0.8125, 50 sweeps with early termination.  Two workloads: h.txt at
AWGN -4 dB, 65 536 frames, and the 8k (3,6) code at 2.0 dB, 8 192 frames.  The frames are dumped once (counter-based noise,
seed 0) as a binary64 device tensor; the float32 tensor is its cast and the int8 tensor clamp(rint(llr / 0.25), -128, 127), so
the three inputs describe the same frames (they do not decode to the same bits: each is decoded as what it widens to).
Interleaved: a round runs every variant once — `warmup` calls, a synchronise, `steps` timed calls into device buffers.  One
JSON line per workload and variant: kernel ms (last_ms(0): the launches between the engine's marks, the packing launch
included, the conversion launch too where there is one) and end-to-end ms per call (HIP events around the calls), median and
range over the rounds, frames/s, mean sweeps, LDS bytes per frame and frames per CU.

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

WORKLOADS = ("3", "4")  # the codes and channel points of these configurations; decoding and early termination as below
SETTING = (6, 8, 0.25)
SCALE = 0.8125
VARIANTS = [dict(call="decode_batch", input="float64"), dict(call="decode_batch_typed", input="float32"),
            dict(call="decode_batch_typed", input="int8"), dict(call="decode_batch_typed", input="int8", hard_bits=True)]
LDS_PER_CU = 160 * 1024


def report(cfg, rounds, steps, warmup):
    import torch
    import libldpc_amd
    w = workloads.get(cfg)
    iterations = w["iterations"]
    dec = libldpc_amd.HipDecoder(workloads.code_path(w))
    B, nc = w["batch"], dec.nc
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    llr = torch.zeros((B, nc), dtype=torch.float64, device=dev)
    dec.set_noise("counter")
    dec.stream_begin(w["channel"], 0, w["x"])
    dec.stream_decode(B, iterations=1, decoding="BP_MS", want=(), out={"llr_in": llr}, stream=stream)
    torch.cuda.synchronize()
    inputs = {"float64": llr, "float32": llr.to(torch.float32),
              "int8": torch.clamp(torch.round(llr / SETTING[2]), -128, 127).to(torch.int8)}
    dec.set_min_sum_layered_fixed(*SETTING)
    dec.set_min_sum_correction(SCALE, 0.0)
    dec.set_profiling(True)
    out = {"iters": torch.zeros(B, dtype=torch.int32, device=dev), "bit_errors": torch.zeros(B, dtype=torch.int32, device=dev)}
    bits = torch.zeros((B, (nc + 31) // 32), dtype=torch.int32, device=dev)

    def calls(v, n):
        o = dict(out, hard_bits=bits) if v.get("hard_bits") else out
        for _ in range(n):
            if v["call"] == "decode_batch":
                dec.decode_batch(inputs[v["input"]], early_term=True, iterations=iterations, decoding="BP_MS", want=(), out=o, stream=stream)
            else:
                dec.decode_batch_typed(inputs[v["input"]], early_term=True, iterations=iterations, decoding="BP_MS", want=(), out=o,
                                       stream=stream)

    res = [{"e2e": [], "kernel": [], "sweeps": None, "fer": None} for _ in VARIANTS]
    for _ in range(rounds):
        for v, r in zip(VARIANTS, res):
            calls(v, warmup)
            torch.cuda.synchronize()
            dec.last_ms(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            calls(v, steps)
            e1.record()
            torch.cuda.synchronize()
            r["e2e"].append(e0.elapsed_time(e1) / steps)
            r["kernel"].append(dec.last_ms(0))
            r["sweeps"] = float(out["iters"].double().mean())
            r["fer"] = float((out["bit_errors"] != 0).double().mean())
    staged, direct = dec.layered_fixed_lds_bytes(), dec.layered_fixed_direct_lds_bytes()
    lines = []
    for v, r in zip(VARIANTS, res):
        lds = staged if v["input"] == "float64" else direct
        e2e, k = statistics.median(r["e2e"]), statistics.median(r["kernel"])
        lines.append({"config": cfg, "code": w["code"], "channel": w["channel"], "x": w["x"], "call": v["call"], "input": v["input"],
                      "hard_bits": bool(v.get("hard_bits")), "decoder_choice": dec.decoder_choice(True, iterations, "BP_MS"),
                      "msg_bits": SETTING[0], "app_bits": SETTING[1], "step": SETTING[2], "scale": SCALE, "early_term": True,
                      "iterations": iterations, "noise": "counter", "seed": 0, "batch": B, "rounds": rounds, "steps": steps,
                      "warmup": warmup, "input_bytes": int(inputs[v["input"]].numel() * inputs[v["input"]].element_size()),
                      "kernel_ms_median": round(k, 4), "kernel_ms_min": round(min(r["kernel"]), 4),
                      "kernel_ms_max": round(max(r["kernel"]), 4), "kernel_ms_rounds": [round(x, 4) for x in r["kernel"]],
                      "e2e_ms_median": round(e2e, 4), "e2e_ms_min": round(min(r["e2e"]), 4), "e2e_ms_max": round(max(r["e2e"]), 4),
                      "e2e_ms_rounds": [round(x, 4) for x in r["e2e"]], "frames_per_s": round(B / e2e * 1e3, 1),
                      "avg_sweeps": r["sweeps"], "fer": r["fer"], "lds_bytes_per_frame": lds, "frames_per_cu_by_lds": LDS_PER_CU // lds})
    base = lines[0]
    for ln in lines:
        ln["kernel_ms_over_float64"] = round(ln["kernel_ms_median"] / base["kernel_ms_median"], 4)
        ln["e2e_ms_over_float64"] = round(ln["e2e_ms_median"] / base["e2e_ms_median"], 4)
    dec.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds one workload's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "typed_batch.jsonl"))
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
