#!/usr/bin/env python3
"""Time per call of erasure_channel_batch and erasure_decode_batch on device tensors (include/ldpc_amd.h,
ldpc_hip_erasure_channel_batch / ldpc_hip_erasure_decode_batch; libldpc_amd/csrc/kernels_erasure.hip), next to two yardsticks
from the same run: the stream's BEC launch (channel and genie decoder fused, LDPC_HIP_NOISE_COUNTER, ldpc_hip_last_ms) on
the same frames, and a device-to-device copy of as many bytes as each call writes.

    python tools/erasure_batch_report.py [--rounds 5] [--window-ms 250] [--out profiles/erasure_batch.jsonl]

Two workloads at the erasure probability of benchmark config 5bec: tests/golden/h.txt at 65 536 frames (codewords of g.txt,
packed, as encode_batch leaves them) and the (3,6)-regular n = 8192 code of benchmark config 4 at 8 192 frames (no generator:
the all-zero codeword).  Every buffer is a device tensor.  The decoder runs 50 iterations with early termination, as the
stream does, and once more with the stalled stop on top.  Every call and every copy is warmed first; a round then times each
of them once, in turn (interleaved), over a window of about --window-ms of back-to-back calls between two device events; the
figure of a round is window / calls.  The stream yardstick is one launch per round on the same seed and frames, with
ldpc_hip_set_bec_compat(0): the frames and results of the two decoders are then the same.  One JSON line per workload and
call: median and range over the rounds.  Any failure ends the report; nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (dict(code="h", frames=65536), dict(code="8k", frames=8192))
ITERATIONS, SEED = 50, 1


def _time(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def report(w, eps, rounds, window_ms):
    import torch
    import libldpc_amd
    from libldpc_amd import workloads
    dev = torch.device("cuda", 0)
    golden = os.path.join(ROOT, "tests", "golden")
    dec = libldpc_amd.HipDecoder(workloads.code_path(w), os.path.join(golden, "g.txt") if w["code"] == "h" else "")
    n, nc, words = w["frames"], dec.nc, (dec.nc + 31) // 32

    def u32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev).view(torch.uint32)

    codeword = None
    if w["code"] == "h":
        gen = torch.Generator(device=dev).manual_seed(1)
        info = torch.randint(0, 2, (n, dec.kc), dtype=torch.uint8, device=dev, generator=gen)
        codeword = u32(n, words)
        dec.encode_batch(info, want=(), out={"codeword_bits": codeword})
    word, erased = u32(n, words), u32(n, words)
    outs = {"word": u32(n, words), "erased": u32(n, words), "iters": u32(n), "unresolved": u32(n)}
    stream_iters = torch.zeros(n, dtype=torch.int32, device=dev)
    channel = lambda: dec.erasure_channel_batch(codeword, eps, seed=SEED, frames=n, want=(), out={"word": word, "erased": erased})  # noqa: E731
    channel()
    timed = {
        "erasure_channel_batch": (channel, 8 * n * words),
        "erasure_decode_batch": (lambda: dec.erasure_decode_batch(word, erased, iterations=ITERATIONS, want=(), out=outs), 8 * n * words + 8 * n),
        "erasure_decode_batch stop_stalled": (lambda: dec.erasure_decode_batch(word, erased, iterations=ITERATIONS, stop_stalled=True,
                                                                             want=(), out=outs), 8 * n * words + 8 * n),
    }
    copies = {}
    for name, (_, out_bytes) in timed.items():
        src, dst = torch.zeros(out_bytes, dtype=torch.uint8, device=dev), torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
        copies[name] = (lambda s=src, d=dst: d.copy_(s))
    dec.set_profiling(True)
    dec.set_noise("counter")
    dec.set_bec_compat(False)

    def stream():
        dec.stream_begin("BEC", SEED, eps)
        dec.last_ms(0)
        dec.stream_decode(n, early_term=True, iterations=ITERATIONS, decoding="BP", want=(), out={"iters": stream_iters})
        torch.cuda.synchronize()
        return dec.last_ms(0)

    # warm every shape and size the windows
    calls = {}
    for name, (fn, _) in timed.items():
        for what in (fn, copies[name]):
            what()
            torch.cuda.synchronize()
            calls[(name, what is copies[name])] = max(10, min(5000, int(window_ms / max(_time(what, 10), 1e-3))))
    stream()
    samples = {name: ([], []) for name in timed}
    stream_ms = []
    for _ in range(rounds):
        for name, (fn, _) in timed.items():
            samples[name][0].append(_time(fn, calls[(name, False)]))
            samples[name][1].append(_time(copies[name], calls[(name, True)]))
        stream_ms.append(stream())
    torch.cuda.synchronize()
    mean = lambda t: round(float(t.view(torch.int32).float().mean()), 3)  # noqa: E731
    mean_stalled = mean(outs["iters"])  # (the last call timed: with the stalled stop)
    timed["erasure_decode_batch"][0]()
    torch.cuda.synchronize()
    same = bool((outs["iters"].view(torch.int32) == stream_iters).all())
    stat = lambda v: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}  # noqa: E731
    left = outs["unresolved"].view(torch.int32)
    lines = []
    for name, (mine, copy) in samples.items():
        lines.append(dict(code=w["code"], nc=nc, mc=dec.mc, nct=dec.nct, frames=n, call=name, eps=eps, iterations=ITERATIONS, early_term=True,
                          codeword="packed" if codeword is not None else "none (all zero)", lds_bytes_per_group=dec.erasure_lds_bytes(),
                          output_bytes=timed[name][1], rounds=rounds, calls_per_window=calls[(name, False)], ms_per_call=stat(mine),
                          ms_rounds=[round(v, 5) for v in mine], copy_same_bytes_ms=stat(copy),
                          stream_bec_launch_ms=stat(stream_ms), stream=dict(noise="counter", bec_compat=False, fused="channel + genie decoder"),
                          frames_resolved=int((left == 0).sum()), mean_iters=mean(outs["iters"]), mean_iters_stop_stalled=mean_stalled,
                          mean_iters_stream=mean(stream_iters), iters_equal_stream=same))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "erasure_batch.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("erasure_batch_report: no GPU (there is no CPU fallback)")
    from libldpc_amd import workloads
    eps = workloads.get("5bec")["x"]
    lines = []
    for w in WORKLOADS:
        lines += report(w, eps, args.rounds, args.window_ms)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
