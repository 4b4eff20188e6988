#!/usr/bin/env python3
"""Time per call of syndrome_decode_layered_batch on device tensors (include/ldpc_amd.h,
ldpc_hip_syndrome_decode_layered_batch; libldpc_amd/csrc/kernels_syndrome_decode_layered.hip) at (6, 8, 0.25, 0.8125) next to
syndrome_decode_batch at (6, 0.25, 0.8125) on the same frames toward the same syndromes, on int8 and on float64 LLRs.

    python tools/syndrome_decode_layered_report.py [--rounds 5] [--window-ms 250] [--out profiles/syndrome_decode_layered.jsonl]

The two workloads of tools/syndrome_decode_report.py: tests/golden/h.txt, 65 536 frames at BSC 0.12, and a (3,6)-regular code of
8 192 columns, 8 192 frames at 0.05.  Every buffer is a device tensor.  The frames: random words x (not codewords),
s = syndrome_batch(x) packed, the LLRs of x through channel_batch (BSC) as int8 with (6, 0.25) and as float64.  All settings are
warmed first; a round then times each of them once, in turn (interleaved), over a window of about --window-ms of back-to-back
calls between two device events; the figure of a round is window / calls.  One JSON line per workload: median and range over
the rounds per setting, mean iterations, the share of frames that reach s, the frames a CU holds by the LDS query, and the
ratio flooding / layered of the medians.  No time is gated.  Any failure ends the report; nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from syndrome_decode_report import ITERATIONS, Q_BITS, SCALE, SEED, STEP, WORKLOADS, _time  # noqa: E402  (the same workloads and clock)

APP_BITS = 8
CU_LDS = 160 * 1024


def report(w, rounds, window_ms, directory):
    import torch
    import libldpc_amd
    import gen_regular_code
    dev = torch.device("cuda", 0)
    if w["code"] == "h":
        path = os.path.join(ROOT, "tests", "golden", "h.txt")
    else:
        path = os.path.join(directory, "r8192.h.txt")
        open(path, "w").write(gen_regular_code.generate(8192, 3, 6, 1))
    dec = libldpc_amd.HipDecoder(path, "")
    n, nc, mc = w["frames"], dec.nc, dec.mc
    words, swords = (nc + 31) // 32, (mc + 31) // 32

    def u32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev).view(torch.uint32)

    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randint(0, 2, (n, nc), dtype=torch.uint8, device=dev, generator=gen)
    s_bits = u32(n, swords)
    dec.syndrome_batch(x, want=(), out={"syndrome_bits": s_bits})
    llr8 = torch.zeros((n, nc), dtype=torch.int8, device=dev)
    llr64 = torch.zeros((n, nc), dtype=torch.float64, device=dev)
    dec.channel_batch(x, "BSC", w["eps"], seed=SEED, llr="int8", q_bits=Q_BITS, step=STEP, want=(), out={"llr": llr8})
    dec.channel_batch(x, "BSC", w["eps"], seed=SEED, want=(), out={"llr": llr64})

    keys = ("layered_int8", "layered_float64", "flooding_int8", "flooding_float64")
    res = {k: {"hard_bits": u32(n, words), "iters": u32(n), "weight": u32(n)} for k in keys}
    layered = dict(iterations=ITERATIONS, early_term=True, msg_bits=Q_BITS, app_bits=APP_BITS, step=STEP, scale=SCALE, offset=0.0, want=())
    flooding = dict(iterations=ITERATIONS, early_term=True, q_bits=Q_BITS, step=STEP, scale=SCALE, offset=0.0, want=())
    timed = {"layered_int8": lambda: dec.syndrome_decode_layered_batch(llr8, s_bits, out=res["layered_int8"], **layered),
             "layered_float64": lambda: dec.syndrome_decode_layered_batch(llr64, s_bits, out=res["layered_float64"], **layered),
             "flooding_int8": lambda: dec.syndrome_decode_batch(llr8, s_bits, out=res["flooding_int8"], **flooding),
             "flooding_float64": lambda: dec.syndrome_decode_batch(llr64, s_bits, out=res["flooding_float64"], **flooding)}
    calls = {}
    for k, fn in timed.items():  # warm, and size the windows
        fn()
        torch.cuda.synchronize()
        calls[k] = max(3, min(5000, int(window_ms / max(_time(fn, 3), 1e-3))))
    samples = {k: [] for k in timed}
    for _ in range(rounds):
        for k, fn in timed.items():
            samples[k].append(_time(fn, calls[k]))
    torch.cuda.synchronize()
    stat = lambda v: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}  # noqa: E731
    i32 = lambda t: t.view(torch.int32)  # noqa: E731
    errors = {k: u32(n) for k in ("layered_int8", "flooding_int8")}
    for k, e in errors.items():
        dec.bit_errors_batch(res[k]["hard_bits"], x, out=e)
    torch.cuda.synchronize()
    lds = dict(layered=dec.syndrome_decode_layered_lds_bytes(), flooding=dec.syndrome_decode_lds_bytes())
    same = lambda a, b: bool(all((i32(res[a][k]) == i32(res[b][k])).all() for k in ("hard_bits", "iters", "weight")))  # noqa: E731
    median = {k: statistics.median(samples[k]) for k in timed}
    line = dict(code=w["code"], nc=nc, mc=mc, frames=n, bsc_eps=w["eps"], msg_bits=Q_BITS, app_bits=APP_BITS, step=STEP, scale=SCALE,
                iterations=ITERATIONS, early_term=True, rounds=rounds, calls_per_window=calls, lds_bytes_per_frame=lds,
                frames_per_cu_by_lds={k: CU_LDS // v for k, v in lds.items()},
                reach_s_share={k: round(float((i32(res[k + "_int8"]["weight"]) == 0).float().mean()), 5) for k in ("layered", "flooding")},
                come_back_as_x_share={k: round(float((i32(errors[k + "_int8"]) == 0).float().mean()), 5) for k in ("layered", "flooding")},
                mean_iters={k: round(float(i32(res[k + "_int8"]["iters"]).float().mean()), 3) for k in ("layered", "flooding")},
                int8_equals_float64=dict(layered=same("layered_int8", "layered_float64"), flooding=same("flooding_int8", "flooding_float64")),
                flooding_over_layered=dict(int8=round(median["flooding_int8"] / median["layered_int8"], 3),
                                           float64=round(median["flooding_float64"] / median["layered_float64"], 3)))
    for k in timed:
        line[k] = dict(ms_per_call=stat(samples[k]), ms_rounds=[round(v, 5) for v in samples[k]])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syndrome_decode_layered.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("syndrome_decode_layered_report: no GPU (there is no CPU fallback)")
    lines = []
    with tempfile.TemporaryDirectory() as directory:
        for w in WORKLOADS:
            lines.append(report(w, args.rounds, args.window_ms, directory))
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
