#!/usr/bin/env python3
"""Time per call of relay_decode_batch on device tensors (include/ldpc_amd.h, ldpc_hip_relay_decode_batch;
libldpc_amd/csrc/kernels_relay_decode.hip) in form 1 (a workgroup per frame) and form 2 (a wave per frame), next to the two
things the library offered for the same frames before: syndrome_decode_batch alone, and syndrome_decode_batch followed by
osd_syndrome_batch (64 candidates, no pairs) on the frames it leaves short of their syndrome.

    python tools/relay_decode_report.py [--rounds 5] [--window-ms 250] [--out profiles/relay_decode.jsonl]

Five workloads.  The X-checks of the 6 x 6 and of the 12 x 12 toric code (72 and 288 columns), 65 536 shots each: errors
Bernoulli(0.09) drawn on the device, s = syndrome_batch(errors), ONE shared prior row log(0.91 / 0.09) in float64; the same
on the 16 x 16 and 20 x 20 codes (512 and 800 columns), which are there to place the rule that chooses between the forms.  And
tests/golden/h.txt with the frames of tools/syndrome_decode_report.py: 65 536 random words, s their syndromes, their LLRs
through channel_batch (BSC 0.12) as int8.  Everything at (6 bits, step 0.25, scale 0.8125); the relay is 12 legs of 50 / 30
iterations, stop_after 1, the gamma of relay_gammas(12, -16, 42, seed 3, first 8); min-sum alone takes 50 iterations.
Every buffer is a device tensor.  The method is that of tools/syndrome_decode_report.py: all rows are warmed first; a round
then times each of them once, in turn (interleaved), over a window of about --window-ms of back-to-back calls between two
device events; the figure of a round is window / calls.  The min-sum + OSD row includes what it takes to find and gather the
frames left (a torch nonzero and two index_selects: a host round trip).  One JSON line per workload; per row the median and
range over the rounds, the share of frames that reach s and the mean iters.  No time is gated.  Any failure ends the report;
nothing more is started on the GPU."""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = (dict(code="toric6", size=6, p=0.09, frames=65536), dict(code="toric12", size=12, p=0.09, frames=65536),
             dict(code="toric16", size=16, p=0.09, frames=65536), dict(code="toric20", size=20, p=0.09, frames=65536),
             dict(code="h", eps=0.12, frames=65536))
SEED, Q_BITS, STEP, SCALE, ITERATIONS = 9, 6, 0.25, 0.8125, 50
RELAY = dict(legs=12, first_iterations=50, leg_iterations=30, stop_after=1)
GAMMA = dict(lo=-16, hi=42, seed=3, first=8)
CANDIDATES, OSD_INFEASIBLE = 64, 4


def _time(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _toric(path, size):
    """The X-checks of the size x size toric code: vertex (i, j) touches h(i, j), h(i, j - 1), v(i, j), v(i - 1, j)."""
    lines = []
    for i in range(size):
        for j in range(size):
            cols = (i * size + j, i * size + (j - 1) % size, size * size + i * size + j, size * size + ((i - 1) % size) * size + j)
            lines += [f"{i * size + j} {c}" for c in sorted(cols)]
    open(path, "w").write("\n".join(lines))
    return path


def report(w, rounds, window_ms, directory):
    import torch
    import libldpc_amd
    dev = torch.device("cuda", 0)
    toric = "size" in w
    path = _toric(os.path.join(directory, w["code"] + ".txt"), w["size"]) if toric else os.path.join(ROOT, "tests", "golden", "h.txt")
    dec = libldpc_amd.HipDecoder(path, "")
    n, nc, mc = w["frames"], dec.nc, dec.mc
    words, swords = (nc + 31) // 32, (mc + 31) // 32

    def u32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev).view(torch.uint32)

    i32 = lambda t: t.view(torch.int32)  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(5)
    s_bits = u32(n, swords)
    if toric:
        x = (torch.rand((n, nc), device=dev, generator=gen) < w["p"]).to(torch.uint8)
        llr = torch.full((nc,), math.log((1.0 - w["p"]) / w["p"]), dtype=torch.float64, device=dev)
    else:
        x = torch.randint(0, 2, (n, nc), dtype=torch.uint8, device=dev, generator=gen)
        llr = torch.zeros((n, nc), dtype=torch.int8, device=dev)
        dec.channel_batch(x, "BSC", w["eps"], seed=SEED, llr="int8", q_bits=Q_BITS, step=STEP, want=(), out={"llr": llr})
    dec.syndrome_batch(x, want=(), out={"syndrome_bits": s_bits})
    gamma = torch.from_numpy(dec.relay_gammas(RELAY["legs"], GAMMA["lo"], GAMMA["hi"], GAMMA["seed"], GAMMA["first"])).to(dev)

    res = {k: {key: u32(n, words) if key == "hard_bits" else u32(n) for key in dec.RELAY_OUTPUTS} for k in ("relay_form1", "relay_form2")}
    res["min_sum"] = {"hard_bits": u32(n, words), "iters": u32(n), "weight": u32(n)}
    res["min_sum_osd"] = dict(res["min_sum"], llr_out=torch.zeros((n, nc), dtype=torch.float64, device=dev))
    common = dict(q_bits=Q_BITS, step=STEP, scale=SCALE, offset=0.0, shared_llr=toric, want=())
    osd = {"left": 0}

    def min_sum_osd():
        out = res["min_sum_osd"]
        dec.syndrome_decode_batch(llr, s_bits, iterations=ITERATIONS, early_term=True, out=out, **common)
        left = torch.nonzero(i32(out["weight"]) != 0).reshape(-1)
        osd["left"] = int(left.numel())
        if left.numel():
            soft = out["llr_out"].index_select(0, left)
            toward = i32(s_bits).index_select(0, left).view(torch.uint32)
            r = {"word": u32(left.numel(), words), "status": u32(left.numel())}
            dec.osd_syndrome_batch(soft, toward, candidates=CANDIDATES, pair_depth=0, want=(), out=r)
            osd["status"] = r["status"]

    timed = {"relay_form1": lambda: dec.relay_decode_batch(llr, s_bits, gamma, form=1, out=res["relay_form1"], **RELAY, **common),
             "relay_form2": lambda: dec.relay_decode_batch(llr, s_bits, gamma, form=2, out=res["relay_form2"], **RELAY, **common),
             "min_sum": lambda: dec.syndrome_decode_batch(llr, s_bits, iterations=ITERATIONS, early_term=True, out=res["min_sum"], **common),
             "min_sum_osd": min_sum_osd}
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
    share = lambda t: round(float((i32(t) == 0).float().mean()), 5)  # noqa: E731
    a, b = res["relay_form1"], res["relay_form2"]
    solved = int((i32(osd["status"]) != OSD_INFEASIBLE).sum()) if osd["left"] else 0
    line = dict(code=w["code"], nc=nc, mc=mc, frames=n, q_bits=Q_BITS, step=STEP, scale=SCALE, relay=RELAY, gamma=GAMMA,
                min_sum_iterations=ITERATIONS, osd_candidates=CANDIDATES, rounds=rounds, calls_per_window=calls,
                lds_bytes_per_frame=dict(relay=dec.relay_decode_lds_bytes(), min_sum=dec.syndrome_decode_lds_bytes(), osd=dec.osd_syndrome_lds_bytes()),
                forms_agree=bool(all((i32(a[k]) == i32(b[k])).all() for k in dec.RELAY_OUTPUTS)),
                reach_s_share=dict(relay=share(a["weight"]), min_sum=share(res["min_sum"]["weight"]),
                                   min_sum_osd=round((n - osd["left"] + solved) / n, 5)),
                mean_iters=dict(relay=round(float(i32(a["iters"]).float().mean()), 3), min_sum=round(float(i32(res["min_sum"]["iters"]).float().mean()), 3)),
                relay_mean_solutions=round(float(i32(a["solutions"]).float().mean()), 4),
                relay_best_leg_histogram=torch.bincount(i32(a["best_leg"])[i32(a["weight"]) == 0].to(torch.int64), minlength=RELAY["legs"]).tolist(),
                frames_left_to_osd=osd["left"])
    if toric:
        line["error_probability"] = w["p"]
    else:
        line["bsc_eps"] = w["eps"]
    for k in timed:
        line[k] = dict(ms_per_call=stat(samples[k]), ms_rounds=[round(v, 5) for v in samples[k]])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relay_decode.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("relay_decode_report: no GPU (there is no CPU fallback)")
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
