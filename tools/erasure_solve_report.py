#!/usr/bin/env python3
"""Time per call of erasure_solve_batch on device tensors (include/ldpc_amd.h, ldpc_hip_erasure_solve_batch;
libldpc_amd/csrc/kernels_erasure_solve.hip) next to the peeling call in front of it, and what each leaves unresolved.

    python tools/erasure_solve_report.py [--rounds 5] [--window-ms 250] [--out profiles/erasure_solve.jsonl]

Three workloads: tests/golden/h.txt at erasure probability 0.82 and 0.85 (codewords of g.txt, packed, as encode_batch leaves
them; max_unknowns = 1024) and a (3,6)-regular code of 240 columns at 0.45 (no generator: the all-zero codeword; max_unknowns
= 240).  Every buffer is a device tensor.  The chain is the advised one: erasure_channel_batch once, then
erasure_decode_batch with 50 iterations, early termination and the stalled stop, then erasure_solve_batch on its output.
Both calls are warmed first; a round then times each of them once, in turn (interleaved), over a window of about --window-ms
of back-to-back calls between two device events; the figure of a round is window / calls.  One JSON line per workload:
median and range over the rounds of both calls, the share of frames each leaves unresolved, and the sizes of the systems the
solver met.  Any failure ends the report; nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = (dict(code="h", eps=0.82, frames=4096, max_unknowns=1024), dict(code="h", eps=0.85, frames=4096, max_unknowns=1024),
             dict(code="r240", eps=0.45, frames=65536, max_unknowns=240))
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
    n, words, cap = w["frames"], (dec.nc + 31) // 32, w["max_unknowns"]

    def u32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev).view(torch.uint32)

    codeword = None
    if w["code"] == "h":
        gen = torch.Generator(device=dev).manual_seed(1)
        info = torch.randint(0, 2, (n, dec.kc), dtype=torch.uint8, device=dev, generator=gen)
        codeword = u32(n, words)
        dec.encode_batch(info, want=(), out={"codeword_bits": codeword})
    word, erased = u32(n, words), u32(n, words)
    dec.erasure_channel_batch(codeword, w["eps"], seed=SEED, frames=n, want=(), out={"word": word, "erased": erased})
    mid = {"word": u32(n, words), "erased": u32(n, words), "iters": u32(n), "unresolved": u32(n)}
    out = {"word": u32(n, words), "erased": u32(n, words), "unresolved": u32(n), "rank": u32(n), "status": u32(n)}
    timed = {
        "peeling": lambda: dec.erasure_decode_batch(word, erased, iterations=ITERATIONS, stop_stalled=True, want=(), out=mid),
        "solve": lambda: dec.erasure_solve_batch(mid["word"], mid["erased"], max_unknowns=cap, want=(), out=out),
    }
    calls = {}
    for name, fn in timed.items():  # warm, and size the windows
        fn()
        torch.cuda.synchronize()
        calls[name] = max(3, min(5000, int(window_ms / max(_time(fn, 3), 1e-3))))
    samples = {name: [] for name in timed}
    for _ in range(rounds):
        for name, fn in timed.items():
            samples[name].append(_time(fn, calls[name]))
    torch.cuda.synchronize()
    stat = lambda v: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}  # noqa: E731
    left_peel, left_solve = mid["unresolved"].view(torch.int32), out["unresolved"].view(torch.int32)
    status = out["status"].view(torch.int32)
    met = left_peel[left_peel > 0].float()
    weight = u32(n)
    dec.syndrome_batch(out["word"], want=(), out={"weight": weight})
    torch.cuda.synchronize()
    clean = bool((weight.view(torch.int32)[status == 0] == 0).all())
    return dict(code=w["code"], nc=dec.nc, mc=dec.mc, frames=n, eps=w["eps"], codeword="packed" if codeword is not None else "none (all zero)",
                peeling=dict(iterations=ITERATIONS, early_term=True, stop_stalled=True, lds_bytes_per_group=dec.erasure_lds_bytes()),
                max_unknowns=cap, solve_lds_bytes_per_frame=dec.erasure_solve_lds_bytes(cap), rounds=rounds, calls_per_window=calls,
                peeling_ms_per_call=stat(samples["peeling"]), solve_ms_per_call=stat(samples["solve"]),
                peeling_ms_rounds=[round(v, 5) for v in samples["peeling"]], solve_ms_rounds=[round(v, 5) for v in samples["solve"]],
                unresolved_share_after_peeling=round(float((left_peel > 0).float().mean()), 5),
                unresolved_share_after_solve=round(float((left_solve > 0).float().mean()), 5),
                status_counts=[int((status == k).sum()) for k in range(4)],
                unknowns_met=dict(frames=int(met.numel()), mean=round(float(met.mean()), 1) if met.numel() else 0.0,
                                  max=int(met.max()) if met.numel() else 0),
                solved_frames_have_zero_syndrome=clean)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "erasure_solve.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("erasure_solve_report: no GPU (there is no CPU fallback)")
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
