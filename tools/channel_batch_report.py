#!/usr/bin/env python3
"""Time per call of channel_batch on device tensors (include/ldpc_amd.h, ldpc_hip_channel_batch;
libldpc_amd/csrc/kernels_channel.hip), next to two yardsticks from the same run: a device-to-device copy of as many bytes as
the call writes, and the decode launch those frames feed.

    python tools/channel_batch_report.py [--rounds 5] [--window-ms 250] [--out profiles/channel_batch.jsonl]

Two workloads: tests/golden/h.txt at 65 536 frames (codewords of g.txt, packed, as encode_batch leaves them) and the
(3,6)-regular n = 8192 code of benchmark config 4 at 8 192 frames (no generator: the all-zero codeword).  Variants: binary
signalling (m = 1) with float64, float32 and int8 LLRs, and 16-ASK (m = 4) with int8; int8 is (6 bits, step 0.25).  Codewords
and LLRs are device tensors.  Every variant and every copy is warmed first; a round then times each of them once, in turn
(interleaved), over a window of about --window-ms of back-to-back calls between two device events; the figure of a round is
window / calls.  The decode yardstick is ldpc_hip_last_ms(0) of decode_batch_typed ("BP_MS", 50 iterations, early
termination) on the variant's own LLRs, once per round: plain min-sum for the floating-point types, for int8 the fixed-point
mode the JSON line names.  One JSON line per workload and variant: median and range over the rounds.  Any failure ends the
report; nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# x: Es / sigma^2 in dB per dimension; 16-ASK needs about 11.5 dB more than binary signalling for the same decoder load
WORKLOADS = (dict(code="h", frames=65536, x={1: 3.0, 4: 14.5}), dict(code="8k", frames=8192, x={1: 2.0, 4: 13.5}))
VARIANTS = ((1, "float64"), (1, "float32"), (1, "int8"), (4, "int8"))
ITERATIONS, Q_BITS, APP_BITS, STEP = 50, 6, 8, 0.25


def _time(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def report(w, rounds, window_ms):
    import torch
    import libldpc_amd
    from libldpc_amd import workloads
    dev = torch.device("cuda", 0)
    golden = os.path.join(ROOT, "tests", "golden")
    dec = libldpc_amd.HipDecoder(workloads.code_path(w), os.path.join(golden, "g.txt") if w["code"] == "h" else "")
    n, nc = w["frames"], dec.nc
    dtypes = {"float64": torch.float64, "float32": torch.float32, "int8": torch.int8}
    codeword = None
    if w["code"] == "h":
        gen = torch.Generator(device=dev).manual_seed(1)
        info = torch.randint(0, 2, (n, dec.kc), dtype=torch.uint8, device=dev, generator=gen)
        codeword = torch.zeros((n, (nc + 31) // 32), dtype=torch.int32, device=dev).view(torch.uint32)
        dec.encode_batch(info, want=(), out={"codeword_bits": codeword})
    try:
        dec.set_min_sum_layered_fixed(Q_BITS, APP_BITS, STEP)
        fixed = f"layered_fixed({Q_BITS}, {APP_BITS}, {STEP})"
        dec.set_min_sum_layered_fixed(0)
    except RuntimeError:
        fixed = f"quantization({Q_BITS}, {STEP})"
    iters = torch.zeros(n, dtype=torch.int32, device=dev)
    dec.set_profiling(True)
    variants, copies, llrs = {}, {}, {}
    for m, kind in VARIANTS:
        llr = torch.zeros((n, nc), dtype=dtypes[kind], device=dev)
        llrs[(m, kind)] = llr
        variants[(m, kind)] = (lambda m=m, kind=kind, llr=llr: dec.channel_batch(
            codeword, "AWGN", w["x"][m], seed=1, bits_per_symbol=m, llr=kind, q_bits=Q_BITS, step=STEP, frames=n, want=(), out={"llr": llr}))
        src, dst = torch.zeros_like(llr), torch.zeros_like(llr)
        copies[(m, kind)] = (lambda s=src, d=dst: d.copy_(s))

    def decode(key):
        if key[1] == "int8":
            if fixed.startswith("layered"):
                dec.set_min_sum_layered_fixed(Q_BITS, APP_BITS, STEP)
            else:
                dec.set_min_sum_quantization(Q_BITS, STEP)
        dec.last_ms(0)
        dec.decode_batch_typed(llrs[key], early_term=True, iterations=ITERATIONS, decoding="BP_MS", want=(), out={"iters": iters})
        torch.cuda.synchronize()
        ms = dec.last_ms(0)
        dec.set_min_sum_layered_fixed(0)
        dec.set_min_sum_quantization(0)
        return ms, float(iters.float().mean())

    # warm every shape and size the windows
    calls = {}
    for key in variants:
        for timed in (variants[key], copies[key]):
            timed()
            torch.cuda.synchronize()
            calls[(key, timed is copies[key])] = max(10, min(5000, int(window_ms / max(_time(timed, 10), 1e-3))))
        decode(key)
    samples = {key: ([], [], []) for key in variants}
    mean_iters = {}
    for _ in range(rounds):
        for key in variants:
            samples[key][0].append(_time(variants[key], calls[(key, False)]))
            samples[key][1].append(_time(copies[key], calls[(key, True)]))
        for key in variants:
            ms, mean_iters[key] = decode(key)
            samples[key][2].append(ms)
    stat = lambda v: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}  # noqa: E731
    lines = []
    for (m, kind), (mine, copy, dms) in samples.items():
        out_bytes = n * nc * llrs[(m, kind)].element_size()
        lines.append(dict(code=w["code"], nc=nc, nct=dec.nct, frames=n, call="channel_batch", channel="AWGN", x=w["x"][m], bits_per_symbol=m,
                          llr=kind, codeword="packed" if codeword is not None else "none (all zero)", output_bytes=out_bytes, rounds=rounds,
                          calls_per_window=calls[((m, kind), False)], ms_per_call=stat(mine), ms_rounds=[round(v, 5) for v in mine],
                          copy_same_bytes_ms=stat(copy), decode_launch_ms=stat(dms),
                          decode=dict(decoding="BP_MS", mode=fixed if kind == "int8" else "plain", iterations=ITERATIONS, early_term=True,
                                      mean_iters=round(mean_iters[(m, kind)], 3))))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_batch.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("channel_batch_report: no GPU (there is no CPU fallback)")
    lines = []
    for w in WORKLOADS:
        lines += report(w, args.rounds, args.window_ms)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
