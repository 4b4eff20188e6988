#!/usr/bin/env python3
"""Time per call of bit_flip_batch on device tensors (include/ldpc_amd.h, ldpc_hip_bit_flip_batch;
libldpc_amd/csrc/kernels_bit_flip.hip) on int8 hard decisions, deterministic (GDBF) and at flip_prob 0.7 (PGDBF), next to
syndrome_decode_batch on the same frames and syndromes: at 2 bits on the same +-1, and at (6, 0.25, 0.8125) on the BSC's LLRs.

    python tools/bit_flip_report.py [--rounds 5] [--window-ms 250] [--out profiles/bit_flip.jsonl]

Two workloads: a (3,6)-regular code of 2 048 columns at BSC 0.03, 65 536 frames, and the (3,6)-regular code of 8 192 columns
at 0.02, 8 192 frames; 100 rounds (iterations) at most.  Every buffer is a device tensor.  The frames: random words x (not
codewords), s = syndrome_batch(x) packed, the LLRs of x through channel_batch (BSC) as int8 with (6, 0.25), and their signs.
The method is that of tools/syndrome_decode_report.py: all rows are warmed first; a round then times each of them once, in
turn (interleaved), over a window of about --window-ms of back-to-back calls between two device events; the figure of a
round is window / calls.  One JSON line per workload; per row the median and range over the rounds, the mean rounds or
iterations, the share of frames that reach s, the share that return x, the time per frame and round, the LDS bytes of a frame
and the frames a CU holds.  No time is gated.  Any failure ends the report; nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = (dict(code="r2048", nc=2048, eps=0.03, frames=65536), dict(code="r8192", nc=8192, eps=0.02, frames=8192))
ROUNDS_MOST, SEED, DRAW_SEED, Q_BITS, STEP, SCALE = 100, 9, 77, 6, 0.25, 0.8125
CU_LDS, CU_WAVES = 160 * 1024, 32


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
    path = os.path.join(directory, w["code"] + ".h.txt")
    open(path, "w").write(gen_regular_code.generate(w["nc"], 3, 6, 1))
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
    dec.channel_batch(x, "BSC", w["eps"], seed=SEED, llr="int8", q_bits=Q_BITS, step=STEP, want=(), out={"llr": llr8})
    hard8 = torch.sign(llr8).to(torch.int8).contiguous()
    assert bool((hard8 != 0).all())

    names = ("bit_flip", "bit_flip_p07", "min_sum_2bit", "min_sum_6bit")
    res = {k: {"hard_bits": u32(n, words), "iters": u32(n), "weight": u32(n)} for k in names}
    flip = dict(iterations=ROUNDS_MOST, q_bits=2, step=1.0, check_weight=2, margin=0, seed=DRAW_SEED, want=())
    soft = dict(iterations=ROUNDS_MOST, early_term=True, offset=0.0, want=())
    timed = {"bit_flip": lambda: dec.bit_flip_batch(hard8, s_bits, flip_prob=1.0, out=res["bit_flip"], **flip),
             "bit_flip_p07": lambda: dec.bit_flip_batch(hard8, s_bits, flip_prob=0.7, out=res["bit_flip_p07"], **flip),
             "min_sum_2bit": lambda: dec.syndrome_decode_batch(hard8, s_bits, q_bits=2, step=1.0, scale=1.0, out=res["min_sum_2bit"], **soft),
             "min_sum_6bit": lambda: dec.syndrome_decode_batch(llr8, s_bits, q_bits=Q_BITS, step=STEP, scale=SCALE, out=res["min_sum_6bit"], **soft)}
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
    bf_lds, ms_lds = dec.bit_flip_lds_bytes(), dec.syndrome_decode_lds_bytes()
    group = max(1, min(4, (CU_LDS // 4) // bf_lds))  # kernels.hpp, bit_flip_group_frames
    lds = {"bit_flip": bf_lds, "bit_flip_p07": bf_lds, "min_sum_2bit": ms_lds, "min_sum_6bit": ms_lds}
    # a wave per frame in groups of `group`; four waves per frame
    per_cu = {"bit_flip": min(CU_WAVES, CU_LDS // (group * bf_lds) * group), "min_sum_2bit": min(CU_WAVES // 4, CU_LDS // ms_lds)}
    per_cu["bit_flip_p07"], per_cu["min_sum_6bit"] = per_cu["bit_flip"], per_cu["min_sum_2bit"]
    line = dict(code=w["code"], nc=nc, mc=mc, frames=n, bsc_eps=w["eps"], rounds_at_most=ROUNDS_MOST, rounds=rounds, calls_per_window=calls)
    errors = u32(n)
    for k in names:
        dec.bit_errors_batch(res[k]["hard_bits"], x, out=errors)
        torch.cuda.synchronize()
        total = float(i32(res[k]["iters"]).double().sum())
        # (min-sum counts the index of the iteration that met s: one more ran)
        ran = total + (float((i32(res[k]["weight"]) == 0).sum()) if k.startswith("min_sum") else 0.0)
        med = statistics.median(samples[k])
        line[k] = dict(ms_per_call=stat(samples[k]), ms_rounds=[round(v, 5) for v in samples[k]],
                       mean_rounds=round(total / n, 3), reach_s_share=round(float((i32(res[k]["weight"]) == 0).float().mean()), 5),
                       return_x_share=round(float((i32(errors) == 0).float().mean()), 5),
                       ns_per_frame_round=round(med * 1e6 / max(ran, 1.0), 3), lds_bytes_per_frame=lds[k], frames_per_cu=per_cu[k])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bit_flip.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bit_flip_report: no GPU (there is no CPU fallback)")
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
