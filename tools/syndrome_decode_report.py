#!/usr/bin/env python3
"""Time per call of syndrome_decode_batch on device tensors (include/ldpc_amd.h, ldpc_hip_syndrome_decode_batch;
libldpc_amd/csrc/kernels_syndrome_decode.hip) on int8 and on float64 LLRs, next to the two things it can be compared with on
the same frames: the route it replaces — decode_batch_typed under set_min_sum_quantization with the same (q, D, scale) on the
augmented code [H | I] with +-99999.9 on the extra columns — and the same decoder toward zero on the unaugmented code.

    python tools/syndrome_decode_report.py [--rounds 5] [--window-ms 250] [--out profiles/syndrome_decode.jsonl]

Two workloads: tests/golden/h.txt, 65 536 frames, and a (3,6)-regular code of 8 192 columns, 8 192 frames.  Every buffer is a
device tensor.  The frames: random words x (not codewords), s = syndrome_batch(x) packed, the LLRs of x through channel_batch
(BSC) as int8 with (6, 0.25) and as float64.  All settings are warmed first; a round then times each of them once, in turn
(interleaved), over a window of about --window-ms of back-to-back calls between two device events; the figure of a round is
window / calls.  One JSON line per workload: median and range over the rounds per setting, the share of frames that reach s,
and whether the native call and the augmented route returned the same iteration counts and decisions.  No time is gated.  Any
failure ends the report; nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = (dict(code="h", eps=0.12, frames=65536), dict(code="r8192", eps=0.05, frames=8192))
ITERATIONS, SEED, Q_BITS, STEP, SCALE = 50, 9, 6, 0.25, 0.8125
SHORTEN = 99999.9


def _time(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _augmented(path, out):
    """[H | I] as a file in (row, column) order: column nc + r in row r alone (header lines dropped)."""
    entries = [tuple(int(v) for v in line.split()[:2]) for line in open(path) if ":" not in line and len(line.split()) >= 2]
    nc, mc = max(c for _, c in entries) + 1, max(r for r, _ in entries) + 1
    entries += [(r, nc + r) for r in range(mc)]
    open(out, "w").write("\n".join(f"{r} {c}" for r, c in sorted(entries)))
    return out


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
    aug = libldpc_amd.HipDecoder(_augmented(path, os.path.join(directory, w["code"] + "_aug.txt")), "")
    for d in (dec, aug):  # (the native call reads none of this)
        d.set_min_sum_quantization(Q_BITS, STEP)
        d.set_min_sum_correction(SCALE, 0.0)
    n, nc, mc = w["frames"], dec.nc, dec.mc
    words, swords, awords = (nc + 31) // 32, (mc + 31) // 32, (aug.nc + 31) // 32
    assert (aug.nc, aug.mc) == (nc + mc, mc) and nc % 32 == 0

    def u32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev).view(torch.uint32)

    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randint(0, 2, (n, nc), dtype=torch.uint8, device=dev, generator=gen)
    s_bits, s_bytes = u32(n, swords), torch.zeros((n, mc), dtype=torch.uint8, device=dev)
    dec.syndrome_batch(x, want=(), out={"syndrome_bits": s_bits, "syndrome": s_bytes})
    llr8 = torch.zeros((n, nc), dtype=torch.int8, device=dev)
    llr64 = torch.zeros((n, nc), dtype=torch.float64, device=dev)
    dec.channel_batch(x, "BSC", w["eps"], seed=SEED, llr="int8", q_bits=Q_BITS, step=STEP, want=(), out={"llr": llr8})
    dec.channel_batch(x, "BSC", w["eps"], seed=SEED, want=(), out={"llr": llr64})
    wide = torch.cat((llr64, SHORTEN * (1.0 - 2.0 * s_bytes.to(torch.float64))), dim=1).contiguous()
    del s_bytes

    def outs(width):
        return {"hard_bits": u32(n, width), "iters": u32(n)}

    res = {"native_int8": dict(outs(words), weight=u32(n)), "native_float64": dict(outs(words), weight=u32(n)),
           "augmented_float64": outs(awords), "toward_zero_float64": outs(words), "toward_zero_int8": outs(words)}
    for k in ("augmented_float64", "toward_zero_float64", "toward_zero_int8"):
        res[k]["iters"] = torch.zeros(n, dtype=torch.int32, device=dev)  # (the decode calls count in int32)
    native = dict(iterations=ITERATIONS, early_term=True, q_bits=Q_BITS, step=STEP, scale=SCALE, offset=0.0, want=())
    typed = dict(early_term=True, iterations=ITERATIONS, decoding="BP_MS", want=())
    timed = {"native_int8": lambda: dec.syndrome_decode_batch(llr8, s_bits, out=res["native_int8"], **native),
             "native_float64": lambda: dec.syndrome_decode_batch(llr64, s_bits, out=res["native_float64"], **native),
             "augmented_float64": lambda: aug.decode_batch_typed(wide, out=res["augmented_float64"], **typed),
             "toward_zero_float64": lambda: dec.decode_batch_typed(llr64, out=res["toward_zero_float64"], **typed),
             "toward_zero_int8": lambda: dec.decode_batch_typed(llr8, out=res["toward_zero_int8"], **typed)}
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
    a, b, c = res["native_int8"], res["native_float64"], res["augmented_float64"]
    errors = u32(n)
    dec.bit_errors_batch(a["hard_bits"], x, out=errors)
    torch.cuda.synchronize()
    line = dict(code=w["code"], nc=nc, mc=mc, frames=n, bsc_eps=w["eps"], q_bits=Q_BITS, step=STEP, scale=SCALE, iterations=ITERATIONS,
                early_term=True, rounds=rounds, calls_per_window=calls,
                lds_bytes_per_frame=dict(native=dec.syndrome_decode_lds_bytes(), augmented=aug.quantized_min_sum_lds_bytes(),
                                         toward_zero=dec.quantized_min_sum_lds_bytes()),
                reach_s_share=round(float((i32(a["weight"]) == 0).float().mean()), 5),
                come_back_as_x_share=round(float((i32(errors) == 0).float().mean()), 5),
                mean_iters=dict(native=round(float(i32(a["iters"]).float().mean()), 3), augmented=round(float(c["iters"].float().mean()), 3),
                                toward_zero=round(float(res["toward_zero_float64"]["iters"].float().mean()), 3)),
                int8_equals_float64=bool((i32(a["hard_bits"]) == i32(b["hard_bits"])).all() and (i32(a["iters"]) == i32(b["iters"])).all()),
                native_equals_augmented=bool((i32(b["hard_bits"]) == i32(c["hard_bits"])[:, :words]).all() and (i32(b["iters"]) == c["iters"]).all()))
    for k in timed:
        line[k] = dict(ms_per_call=stat(samples[k]), ms_rounds=[round(v, 5) for v in samples[k]])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syndrome_decode.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("syndrome_decode_report: no GPU (there is no CPU fallback)")
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
