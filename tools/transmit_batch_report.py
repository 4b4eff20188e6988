#!/usr/bin/env python3
"""Time per call of encode_batch and syndrome_batch on device tensors (include/ldpc_amd.h, ldpc_hip_encode_batch /
ldpc_hip_syndrome_batch; libldpc_amd/csrc/kernels_gf2.hip), next to two yardsticks from the same run: a device-to-device copy
of as many bytes as the call writes, and the decode launch those frames feed.

    python tools/transmit_batch_report.py [--rounds 5] [--window-ms 250] [--out profiles/transmit_batch.jsonl]

Two workloads: tests/golden/h.txt with g.txt at 65 536 frames, and the largest generator pair of tests/generator_codes.py
(s6000x3600: nc = 9600, kc = 6000) at 8 192 frames.  Information, words and outputs are device tensors.  Variants: encode_batch
bytes -> bytes and packed -> packed, syndrome_batch bytes -> syndrome bytes + weight and packed -> syndrome words + weight.
Every variant and every copy is warmed first; a round then times each of them once, in turn (interleaved), over a window of
about --window-ms of back-to-back calls between two device events; the figure of a round is window / calls.  The decode
yardstick is ldpc_hip_last_ms(0) of decode_batch ("BP_MS", 50 iterations, early termination) on the LLRs the library's own
counter-noise stream made of encoded frames at the workload's channel point, once per round.  One JSON line per workload and
variant: median and range over the rounds.  Any failure ends the report; nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = (dict(code="h", frames=65536, x=3.0), dict(code="s6000x3600", frames=8192, x=5.5))
ITERATIONS = 50


def _files(code, directory):
    if code == "h":
        golden = os.path.join(ROOT, "tests", "golden")
        return os.path.join(golden, "h.txt"), os.path.join(golden, "g.txt")
    import generator_codes
    return generator_codes.write_pair(directory, code)


def _time(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def report(w, rounds, window_ms, directory):
    import torch
    import libldpc_amd
    dev = torch.device("cuda", 0)
    dec = libldpc_amd.HipDecoder(*_files(w["code"], directory))
    n, nc, mc, kc = w["frames"], dec.nc, dec.mc, dec.kc
    words = lambda bits: (bits + 31) // 32  # noqa: E731
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)  # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731  (packed words: passed on as views of uint32)
    u = lambda t: t.view(torch.uint32)  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(1)
    info = torch.randint(0, 2, (n, kc), dtype=torch.uint8, device=dev, generator=gen)
    cw, cw_bits = u8(n, nc), i32(n, words(nc))
    synd, synd_bits, weight = u8(n, mc), i32(n, words(mc)), i32(n)
    # codewords with a few bits flipped, so that the syndrome has work in it; the packed operands are made by torch, so that
    # the checks below hold the library's two formats against each other
    dec.encode_batch(info, want=(), out={"codeword": cw, "codeword_bits": u(cw_bits)})
    word = cw ^ (torch.rand((n, nc), device=dev, generator=gen) < 0.01).to(torch.uint8)
    shifts = torch.arange(32, device=dev, dtype=torch.int64)

    def pack(rows, length):
        padded = torch.nn.functional.pad(rows.to(torch.int64), (0, words(length) * 32 - length)).view(rows.shape[0], -1, 32)
        return (padded << shifts).sum(2).to(torch.int32).contiguous()

    info_bits, word_bits = pack(info, kc), pack(word, nc)
    variants = {
        ("encode_batch", "bytes"): (lambda: dec.encode_batch(info, want=(), out={"codeword": cw}), n * nc),
        ("encode_batch", "packed"): (lambda: dec.encode_batch(u(info_bits), want=(), out={"codeword_bits": u(cw_bits)}), 4 * n * words(nc)),
        ("syndrome_batch", "bytes"): (lambda: dec.syndrome_batch(word, want=(), out={"syndrome": synd, "weight": u(weight)}), n * mc + 4 * n),
        ("syndrome_batch", "packed"): (lambda: dec.syndrome_batch(u(word_bits), want=(), out={"syndrome_bits": u(synd_bits), "weight": u(weight)}),
                                       4 * n * words(mc) + 4 * n),
    }
    copies = {}
    for key, (_, out_bytes) in variants.items():
        src, dst = u8(out_bytes), u8(out_bytes)
        copies[key] = (lambda s=src, d=dst: d.copy_(s))
    # the decode launch these frames feed: LLRs of encoded frames from the library's counter-noise stream
    llr = torch.zeros((n, nc), dtype=torch.float64, device=dev)
    dec.set_noise("counter")
    dec.stream_begin("AWGN", 0, w["x"])
    dec.stream_decode(n, iterations=1, decoding="BP_MS", want=(), out={"llr_in": llr})
    iters = torch.zeros(n, dtype=torch.int32, device=dev)
    dec.set_profiling(True)

    def decode():
        dec.decode_batch(llr, early_term=True, iterations=ITERATIONS, decoding="BP_MS", want=(), out={"iters": iters})
        torch.cuda.synchronize()
        return dec.last_ms(0)

    # warm every shape, check the two paths against each other, and size the windows
    calls = {}
    for key, (fn, _) in variants.items():
        for timed in (variants[key][0], copies[key]):
            timed()
            torch.cuda.synchronize()
            calls[(key, timed is copies[key])] = max(10, min(5000, int(window_ms / max(_time(timed, 10), 1e-3))))
    packed_first = synd_bits.clone()
    variants[("syndrome_batch", "bytes")][0]()
    torch.cuda.synchronize()
    assert torch.equal(pack(synd, mc), packed_first) and torch.equal(pack(cw, nc), cw_bits) and int(weight.sum()) > 0
    decode()
    samples = {key: ([], []) for key in variants}
    decode_ms = []
    for _ in range(rounds):
        for key, (fn, _) in variants.items():
            samples[key][0].append(_time(fn, calls[(key, False)]))
            samples[key][1].append(_time(copies[key], calls[(key, True)]))
        decode_ms.append(decode())
    stat = lambda v: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}  # noqa: E731
    lines = []
    for (call, fmt), (_, out_bytes) in variants.items():
        mine, copy = samples[(call, fmt)]
        lines.append(dict(code=w["code"], nc=nc, mc=mc, kc=kc, frames=n, call=call, format=fmt, output_bytes=out_bytes,
                          rounds=rounds, calls_per_window=calls[((call, fmt), False)], ms_per_call=stat(mine), ms_rounds=[round(v, 5) for v in mine],
                          copy_same_bytes_ms=stat(copy), decode_launch_ms=stat(decode_ms), decode=dict(channel="AWGN", x=w["x"], decoding="BP_MS",
                          iterations=ITERATIONS, early_term=True, mean_iters=round(float(iters.float().mean()), 3))))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transmit_batch.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("transmit_batch_report: no GPU (there is no CPU fallback)")
    lines = []
    with tempfile.TemporaryDirectory() as d:
        for w in WORKLOADS:
            lines += report(w, args.rounds, args.window_ms, d)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
