#!/usr/bin/env python3
"""Time per call of osd_syndrome_batch on device tensors (include/ldpc_amd.h, ldpc_hip_osd_syndrome_batch;
libldpc_amd/csrc/kernels_osd_syndrome.hip) on the frames that syndrome_decode_batch leaves short of their syndrome, next to
that launch, and the share of those frames that come back as the transmitted word at each pair depth.

    python tools/osd_syndrome_report.py [--rounds 5] [--window-ms 250] [--out profiles/osd_syndrome.jsonl]

Two workloads, 65 536 frames each: tests/golden/h.txt at a crossover probability of 0.12 and a (3,6)-regular code of 240
columns at 0.05.  Every buffer is a device tensor.  The chain: random words x (not codewords) of a device generator,
s = syndrome_batch(x) packed, the LLRs of x through channel_batch (BSC, binary64), syndrome_decode_batch (6 bits, step 0.25,
scale 0.8125, 50 iterations, early termination) — timed between two device events —; the frames with weight > 0 are gathered
and the settings below run on their llr_out and their s:
  (a) osd_batch with 64 candidates against osd_syndrome_batch with 64 candidates, no syndrome and pair_depth 0, on the same
      LLRs: the two do the same work (the decisions miss H x = 0 on about every such frame), so their ratio is recorded;
  (b) osd_syndrome_batch toward s with 64 candidates and pair_depth 0, 16, 64 and 256;
  (c) the same at pair_depth 0 and 256 on the first min(256, failing) frames alone: at most one frame per CU, so the
      difference is one frame's pair stage at the cap.
All settings are warmed first; a round then times each of them once, in turn (interleaved), over a window of about
--window-ms of back-to-back calls between two device events; the figure of a round is window / calls.  One JSON line per
workload: median and range over the rounds, and per depth the share of the failing frames that come back as x.  No time is
gated.  Any failure ends the report; nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = (dict(code="r240", eps=0.05, frames=65536), dict(code="h", eps=0.12, frames=65536))
MIN_SUM = dict(iterations=50, early_term=True, q_bits=6, step=0.25, scale=0.8125, offset=0.0)
SEED, CANDIDATES, DEPTHS = 9, 64, (0, 16, 64, 256)


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
    import numpy as np
    import torch
    import libldpc_amd
    import gen_regular_code
    dev = torch.device("cuda", 0)
    if w["code"] == "h":
        dec = libldpc_amd.HipDecoder(os.path.join(ROOT, "tests", "golden", "h.txt"), "")
    else:
        path = os.path.join(directory, "r240.h.txt")
        open(path, "w").write(gen_regular_code.generate(240, 3, 6, 1))
        dec = libldpc_amd.HipDecoder(path, "")
    n, words, syn_words = w["frames"], (dec.nc + 31) // 32, (dec.mc + 31) // 32

    def u32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev).view(torch.uint32)

    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randint(0, 2, (n, dec.nc), dtype=torch.uint8, device=dev, generator=gen)
    s = u32(n, syn_words)
    dec.syndrome_batch(x, want=(), out={"syndrome_bits": s})
    llr = torch.zeros((n, dec.nc), dtype=torch.float64, device=dev)
    dec.channel_batch(x, "BSC", w["eps"], seed=SEED, want=(), out={"llr": llr})
    out = {"iters": u32(n), "weight": u32(n), "llr_out": torch.zeros((n, dec.nc), dtype=torch.float64, device=dev), "hard_bits": u32(n, words)}
    decode = lambda: dec.syndrome_decode_batch(llr, s, want=(), out=out, **MIN_SUM)  # noqa: E731
    decode()
    torch.cuda.synchronize()
    decode_ms = [_time(decode, 1) for _ in range(2)]
    failing = torch.nonzero(out["weight"].view(torch.int32) != 0).flatten()
    f = int(failing.numel())
    if f == 0:
        raise SystemExit(f"osd_syndrome_report: min-sum left no frame of {w['code']} at {w['eps']}")
    soft = out["llr_out"][failing].contiguous()
    toward = s.view(torch.int32)[failing].contiguous().view(torch.uint32)
    bits = np.zeros((f, 32 * words), np.uint8)  # x as packed words, to compare the words returned with
    bits[:, :dec.nc] = x[failing].cpu().numpy()
    sent = torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view(np.int32).reshape(f, words)).to(dev)

    def bufs(count, columns):
        return {"word": u32(count, words), "flips": u32(count), "status": u32(count), columns: u32(count, 2) if columns == "flipped_columns" else u32(count),
                "metric": torch.zeros(count, dtype=torch.int64, device=dev).view(torch.uint64)}

    one = min(f, 256)
    res = {"osd_batch": bufs(f, "flipped_column"), "null_depth0": bufs(f, "flipped_columns")}
    timed = {"osd_batch": lambda: dec.osd_batch(soft, candidates=CANDIDATES, want=(), out=res["osd_batch"]),
             "null_depth0": lambda: dec.osd_syndrome_batch(soft, None, candidates=CANDIDATES, pair_depth=0, want=(), out=res["null_depth0"])}
    for d in DEPTHS:
        res[f"depth{d}"] = bufs(f, "flipped_columns")
        timed[f"depth{d}"] = lambda d=d: dec.osd_syndrome_batch(soft, toward, candidates=CANDIDATES, pair_depth=d, want=(), out=res[f"depth{d}"])
    for d in (0, 256):
        res[f"one_per_cu_depth{d}"] = bufs(one, "flipped_columns")
        timed[f"one_per_cu_depth{d}"] = lambda d=d: dec.osd_syndrome_batch(soft[:one], toward[:one], candidates=CANDIDATES, pair_depth=d, want=(),
                                                                           out=res[f"one_per_cu_depth{d}"])
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
    line = dict(code=w["code"], nc=dec.nc, mc=dec.mc, frames=n, crossover=w["eps"], candidates=CANDIDATES,
                decode=dict(MIN_SUM, ms_per_call=[round(v, 5) for v in decode_ms], mean_iters=round(float(out["iters"].view(torch.int32).float().mean()), 3)),
                failing_frames=f, failing_share=round(f / n, 5), frames_one_per_cu=one, lds_bytes_per_frame=dec.osd_syndrome_lds_bytes(),
                osd_lds_bytes_per_frame=dec.osd_lds_bytes(), rounds=rounds, calls_per_window=calls)
    for k in timed:
        line[k] = dict(ms_per_call=stat(samples[k]), ms_rounds=[round(v, 5) for v in samples[k]])
    a, b = line["null_depth0"]["ms_per_call"], line["osd_batch"]["ms_per_call"]
    line["null_depth0_over_osd_batch"] = dict(median=round(a["median"] / b["median"], 4),
                                              rounds=[round(p / q, 4) for p, q in zip(samples["null_depth0"], samples["osd_batch"])])
    line["null_depth0_equals_osd_batch"] = bool(all(torch.equal(res["null_depth0"][k].view(torch.int32), res["osd_batch"][k].view(torch.int32))
                                                    for k in ("word", "flips", "status")) and
                                                torch.equal(res["null_depth0"]["metric"].view(torch.int64), res["osd_batch"]["metric"].view(torch.int64)))
    line["pair_stage_ms_per_frame_at_cap"] = round(line["one_per_cu_depth256"]["ms_per_call"]["median"] - line["one_per_cu_depth0"]["ms_per_call"]["median"], 5)
    for d in DEPTHS:
        r = res[f"depth{d}"]
        check = u32(f, syn_words)
        dec.syndrome_batch(r["word"], want=(), out={"syndrome_bits": check})
        torch.cuda.synchronize()
        right = (r["word"].view(torch.int32) == sent).all(1)
        status = r["status"].view(torch.int32)
        line[f"depth{d}"].update(transmitted_word_share=round(float(right.float().mean()), 5), transmitted_word_frames=int(right.sum()),
                                 status_counts=[int((status == k).sum()) for k in range(5)],
                                 every_word_has_the_syndrome=bool(torch.equal(check.view(torch.int32), toward.view(torch.int32))))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "osd_syndrome.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("osd_syndrome_report: no GPU (there is no CPU fallback)")
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
