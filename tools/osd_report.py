#!/usr/bin/env python3
"""Time per call of osd_batch on device tensors (include/ldpc_amd.h, ldpc_hip_osd_batch; libldpc_amd/csrc/kernels_osd.hip)
on the frames that min-sum leaves with a non-zero syndrome, next to the decode launch that produced them, and the share of
those frames that OSD turns into the transmitted codeword.

    python tools/osd_report.py [--rounds 5] [--window-ms 250] [--out profiles/osd.jsonl]

Two workloads: a (3,6)-regular code of 240 columns at 3.0 dB (no generator: the all-zero codeword) and tests/golden/h.txt at
-3.6 dB (codewords of g.txt, packed, as encode_batch leaves them), 65 536 frames each.  Every buffer is a device tensor.  The
chain: channel_batch (AWGN, binary64 LLRs), decode_batch_typed with "BP_MS", 50 iterations and early termination — its
launch time is ldpc_hip_last_ms(0) —, syndrome_batch of its decisions; the frames with a non-zero syndrome are gathered and
osd_batch runs on their llr_out with 0 and with 64 candidates.  Both settings are warmed first; a round then times each of
them once, in turn (interleaved), over a window of about --window-ms of back-to-back calls between two device events; the
figure of a round is window / calls.  One JSON line per workload: median and range over the rounds, the decode launch, and
per setting the share of the failing frames that come back as the transmitted codeword.  No time is gated.  Any failure
ends the report; nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = (dict(code="r240", x=3.0, frames=65536), dict(code="h", x=-3.6, frames=65536))
ITERATIONS, SEED, CANDIDATES = 50, 1, (0, 64)


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
    import gen_regular_code
    dev = torch.device("cuda", 0)
    golden = os.path.join(ROOT, "tests", "golden")
    if w["code"] == "h":
        dec = libldpc_amd.HipDecoder(os.path.join(golden, "h.txt"), os.path.join(golden, "g.txt"))
    else:
        path = os.path.join(directory, "r240.h.txt")
        open(path, "w").write(gen_regular_code.generate(240, 3, 6, 1))
        dec = libldpc_amd.HipDecoder(path, "")
    n, words = w["frames"], (dec.nc + 31) // 32

    def u32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev).view(torch.uint32)

    codeword = u32(n, words)
    if w["code"] == "h":
        gen = torch.Generator(device=dev).manual_seed(1)
        info = torch.randint(0, 2, (n, dec.kc), dtype=torch.uint8, device=dev, generator=gen)
        dec.encode_batch(info, want=(), out={"codeword_bits": codeword})
    llr = torch.zeros((n, dec.nc), dtype=torch.float64, device=dev)
    dec.channel_batch(codeword, "AWGN", w["x"], seed=SEED, want=(), out={"llr": llr})
    out = {"iters": torch.zeros(n, dtype=torch.int32, device=dev), "llr_out": torch.zeros((n, dec.nc), dtype=torch.float64, device=dev),
           "hard_bits": u32(n, words)}
    dec.set_profiling(True)
    decode_ms = []
    for _ in range(3):  # (the first launch warms)
        dec.last_ms(0)
        dec.decode_batch_typed(llr, early_term=True, iterations=ITERATIONS, decoding="BP_MS", want=(), out=out)
        torch.cuda.synchronize()
        decode_ms.append(dec.last_ms(0))
    dec.set_profiling(False)
    weight = u32(n)
    dec.syndrome_batch(out["hard_bits"], want=(), out={"weight": weight})
    torch.cuda.synchronize()
    failing = torch.nonzero(weight.view(torch.int32) != 0).flatten()
    f = int(failing.numel())
    if f == 0:
        raise SystemExit(f"osd_report: min-sum left no frame of {w['code']} at {w['x']} dB")
    soft = out["llr_out"][failing].contiguous()
    sent = codeword.view(torch.int32)[failing].contiguous()
    res = {c: {"word": u32(f, words), "flips": u32(f), "status": u32(f), "flipped_column": u32(f),
               "metric": torch.zeros(f, dtype=torch.int64, device=dev).view(torch.uint64)} for c in CANDIDATES}
    timed = {c: (lambda c=c: dec.osd_batch(soft, candidates=c, want=(), out=res[c])) for c in CANDIDATES}
    calls = {}
    for c, fn in timed.items():  # warm, and size the windows
        fn()
        torch.cuda.synchronize()
        calls[c] = max(3, min(5000, int(window_ms / max(_time(fn, 3), 1e-3))))
    samples = {c: [] for c in timed}
    for _ in range(rounds):
        for c, fn in timed.items():
            samples[c].append(_time(fn, calls[c]))
    torch.cuda.synchronize()
    stat = lambda v: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}  # noqa: E731
    line = dict(code=w["code"], nc=dec.nc, mc=dec.mc, frames=n, es_over_sigma2_db=w["x"], codeword="packed" if w["code"] == "h" else "none (all zero)",
                decode=dict(decoding="BP_MS", iterations=ITERATIONS, early_term=True, launch_ms=[round(v, 5) for v in decode_ms[1:]],
                            mean_iters=round(float(out["iters"].float().mean()), 3)),
                failing_frames=f, failing_share=round(f / n, 5), osd_lds_bytes_per_frame=dec.osd_lds_bytes(), rounds=rounds,
                calls_per_window={str(c): calls[c] for c in CANDIDATES})
    for c in CANDIDATES:
        check = u32(f)
        dec.syndrome_batch(res[c]["word"], want=(), out={"weight": check})
        torch.cuda.synchronize()
        right = (res[c]["word"].view(torch.int32) == sent).all(1)
        status = res[c]["status"].view(torch.int32)
        line[f"osd{c}"] = dict(ms_per_call=stat(samples[c]), ms_rounds=[round(v, 5) for v in samples[c]],
                               transmitted_codeword_share=round(float(right.float().mean()), 5), transmitted_codeword_frames=int(right.sum()),
                               status_counts=[int((status == k).sum()) for k in range(3)],
                               every_word_has_zero_syndrome=bool((check.view(torch.int32) == 0).all()))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "osd.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("osd_report: no GPU (there is no CPU fallback)")
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
