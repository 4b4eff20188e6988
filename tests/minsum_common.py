"""What the tests of the min-sum variants (correction, layered, quantized, ternary, fixed-point layered: test_*min_sum*.py,
test_*ternary*.py) and of the decoder choice share: one descriptor per variant (VARIANTS), comparing results bit for bit,
dumping a stream's LLRs, the split-batch and the no-iteration checks, writing a small parity-check file, the launch stages
while a variant is on, and the bodies of the tests every variant has — the paths that must not move, the simulation loop and
the CLI, the fused channel.  A plain module, like orc.py."""
import os
import subprocess
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable

import numpy as np

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = ("iters", "hard", "llr_out", "bit_errors")


@dataclass(frozen=True)
class Variant:
    """What the shared test bodies need to know about one variant of BP_MS decoding."""
    on: Callable                     # switches it on (the setting of test_nothing_else_moves and of the host tests)
    off: Callable
    sim_on: Callable = None          # the setting of test_simulation_and_cli (default: on) ...
    flags: tuple = ()                # ... and the same on ldpcsim's command line
    banner: tuple = ()               # what ldpcsim's banner then holds
    counter: bool = True             # the simulation runs on counter-based noise
    channel: str = "AWGN"
    xr: tuple = (-4.5, -3.5, 0.5)    # the simulation's range and, in the order of its rows, the points it visits
    points: tuple = (-4.5, -4.0)
    plain: tuple = None              # the run without the flags: (text its banner lacks, its result file differs); None: no such run
    refused: tuple = ()              # refused command lines: (with the default BP decoding?, flags, texts of the message)
    changes: str = None              # the output of BP_MS it certainly changes
    afterwards: tuple = ()           # the other variants BP_MS is checked under once this one is off again
    setter: str = None               # one of the four that exclude each other: its setter's C name ...
    choice: str = None               # ... the decoder it selects (HipDecoder.DECODERS) ...
    state: Callable = None           # ... and its getter


VARIANTS = {
    "correction": Variant(
        on=lambda d: d.set_min_sum_correction(0.75, 0.25), off=lambda d: d.set_min_sum_correction(1.0, 0.0),
        sim_on=lambda d: d.set_min_sum_correction(0.8125, 0.25), flags=("--ms-scale", "0.8125", "--ms-offset", "0.25"),
        banner=("NON-PARITY", "Min-Sum Correction"), counter=False, plain=("NON-PARITY", True)),
    "layered": Variant(
        on=lambda d: d.set_min_sum_schedule("layered"), off=lambda d: d.set_min_sum_schedule("flooding"),
        sim_on=lambda d: (d.set_min_sum_schedule("layered"), d.set_min_sum_correction(0.8125, 0.0)),
        flags=("--ms-schedule", "layered", "--ms-scale", "0.8125"), banner=("NON-PARITY", "Min-Sum Schedule: layered"), counter=False,
        plain=("NON-PARITY", False), refused=((True, ("--ms-schedule", "layered"), ("--ms-schedule",)),), changes="iters",
        setter="ldpc_hip_set_min_sum_schedule", choice="layered-min-sum", state=lambda d: d.min_sum_schedule == "layered"),
    "quantized": Variant(
        on=lambda d: d.set_min_sum_quantization(6, 0.25), off=lambda d: d.set_min_sum_quantization(0),
        flags=("--ms-bits", "6", "--ms-step", "0.25"), banner=("Min-Sum Quantization: 6 bits, step 0.25", "NON-PARITY"),
        plain=("Min-Sum Quantization", True),
        refused=((True, ("--ms-bits", "6", "--ms-step", "0.25"), ("--ms-bits",)),
                 (False, ("--ms-bits", "6", "--ms-step", "0.25", "--ms-schedule", "layered"), ("--ms-bits", "layered")),
                 (False, ("--ms-bits", "9"), ("--ms-bits",))),
        changes="llr_out", afterwards=("layered",),
        setter="ldpc_hip_set_min_sum_quantization", choice="quantized-min-sum", state=lambda d: d.min_sum_quantization[0] == 6),
    "ternary": Variant(
        on=lambda d: d.set_min_sum_ternary(2), off=lambda d: d.set_min_sum_ternary(0), sim_on=lambda d: d.set_min_sum_ternary(1),
        flags=("--ms-ternary", "1"), banner=("Min-Sum Ternary: weight 1", "NON-PARITY"), channel="BSC", xr=(0.03, 0.045, 0.01),
        points=(0.03 + 0.01, 0.03),  # (the loop walks an eps axis from its far end, adding the step up from MIN)
        refused=tuple((False, ("--ms-ternary", "1") + extra, ("--ms-ternary",)) for extra in
                      (("--ms-bits", "6"), ("--ms-schedule", "layered"), ("--ms-scale", "0.75"), ("--ms-offset", "0.5"))) +
                ((True, ("--ms-ternary", "1"), ("--ms-ternary",)), (False, ("--ms-ternary", "8"), ("--ms-ternary",))),
        changes="llr_out", afterwards=("layered", "quantized"),
        setter="ldpc_hip_set_min_sum_ternary", choice="ternary", state=lambda d: d.min_sum_ternary == 2),
    "layered-fixed": Variant(
        on=lambda d: d.set_min_sum_layered_fixed(6, 8, 0.25), off=lambda d: d.set_min_sum_layered_fixed(0),
        flags=("--ms-layered-fixed", "6,8,0.25"),
        banner=(" Min-Sum Layered Fixed-Point: 6-bit messages, 8-bit totals, step 0.25, NON-PARITY",),
        plain=("Min-Sum Layered Fixed-Point", True),
        refused=((True, ("--ms-layered-fixed", "6,8,0.25"), ("--ms-layered-fixed",)),) +
                tuple((False, ("--ms-layered-fixed", "6,8,0.25") + extra, ("--ms-layered-fixed", extra[0])) for extra in
                      (("--ms-bits", "6"), ("--ms-schedule", "layered"), ("--ms-ternary", "2"))) +
                ((False, ("--ms-layered-fixed", "6,5,0.25"), ("--ms-layered-fixed",)),),
        changes="llr_out", afterwards=("layered", "quantized"),
        setter="ldpc_hip_set_min_sum_layered_fixed", choice="layered-fixed-min-sum", state=lambda d: d.min_sum_layered_fixed == (6, 8, 0.25)),
}
EXCLUSIVE = [k for k, v in VARIANTS.items() if v.setter]  # the four of which at most one is in force


def same(r, m, what, rows=slice(None)):
    """Results r equal rows `rows` of the results m: iters, hard, bit_errors, and llr_out as uint64."""
    for k in WANT:
        a, b = r[k], np.asarray(m[k])[rows].astype(r[k].dtype)
        if k == "llr_out":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (what, k)


def dumped(d, switch_off, ch, x, n, seed=3):
    """llr_in of n frames of the reference stream, dumped with the variant switched off (switch_off(d)) and plain min-sum."""
    switch_off(d)
    d.set_min_sum_correction()
    d.stream_begin(ch, seed, x)
    return d.stream_decode(n, decoding="BP_MS", want=("llr_in",))["llr_in"]


def against_mirror(settings, runs, decode, mirror):
    """decode(setting, early, iterations) against mirror(setting, early, iterations) for every setting (a tuple) and every
    (early, iterations) of runs; returns the mirror's results by setting + (early,)."""
    out = {}
    for st in settings:
        for early, iters in runs:
            m = out[st + (early,)] = mirror(st, early, iters)
            same(decode(st, early, iters), m, (st, early))
    return out


def check_split_batch(run, llr, cut=20):
    """run(llr) equals run on the first `cut` frames followed by run on the rest; returns run(llr)."""
    one = run(llr)
    a, b = run(llr[:cut]), run(llr[cut:])
    for k in WANT:
        assert np.array_equal(np.concatenate((a[k], b[k])), one[k]), k
    return one


def check_no_iteration(z):
    """Results of a decode with iterations = 0: decisions, outputs and counts all zero."""
    assert not z["hard"].any() and not z["llr_out"].view(np.uint64).any() and not z["iters"].any()
    assert np.array_equal(z["bit_errors"], np.zeros(len(z["iters"]), np.uint32))


def write(path, rows):
    """rows: list of column lists -> a parity-check file of "row col" lines."""
    open(path, "w").write("\n".join(f"{i} {c}" for i, cs in enumerate(rows) for c in cs))
    return str(path)


def check_decode_stages(d, switch_on, switch_off):
    """One `whole` launch for BP_MS while the variant is on; BP keeps its stages; everything back when it is off."""
    before = {(dec, early, it): d.decode_stages(early, it, dec) for dec in ("BP", "BP_MS") for early in (True, False)
              for it in (50, 0)}
    switch_on(d)
    for (dec, early, it), st in before.items():
        now = d.decode_stages(early, it, dec)
        if dec == "BP_MS":
            assert now == ["whole"], (early, it)
        else:
            assert now == st, (early, it)
    switch_off(d)
    assert all(d.decode_stages(e, i, dec) == st for (dec, e, i), st in before.items())


def check_nothing_else_moves(v):
    """With the variant on, BP (AWGN, BSC) and BEC outputs equal a fresh context's and BP_MS differs in v.changes; with it off
    again, BP_MS equals a fresh context's — flooding, then under each variant of v.afterwards.  Returns the flooding results
    of the context that had the variant on, by early termination."""
    import libldpc_amd
    want = WANT + ("llr_in",)
    var = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    fresh = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    v.on(var)
    for ch, x, dec, early in (("AWGN", -4.0, "BP", True), ("AWGN", -4.0, "BP", False), ("BSC", 0.24, "BP", True),
                              ("BEC", 0.7, "BP", True), ("BEC", 0.7, "BP_MS", True)):
        rs = []
        for d in (var, fresh):
            d.stream_begin(ch, 2, x)
            rs.append(d.stream_decode(64, early_term=early, iterations=50, decoding=dec, want=want))
        for k in want:
            assert np.array_equal(rs[0][k], rs[1][k]), (ch, dec, early, k)
        if ch != "BEC":
            a = var.decode_batch(rs[1]["llr_in"], early_term=early, decoding=dec, want=WANT)
            b = fresh.decode_batch(rs[1]["llr_in"], early_term=early, decoding=dec, want=WANT)
            for k in WANT:
                assert np.array_equal(a[k], b[k]), (ch, dec, k)
    if v.changes:  # the variant does change BP_MS ...
        rs = []
        for d in (var, fresh):
            d.stream_begin("AWGN", 4, -4.5)
            rs.append(d.stream_decode(32, iterations=50, decoding="BP_MS", want=want))
        assert np.array_equal(rs[0]["llr_in"], rs[1]["llr_in"])
        if v.changes == "llr_out":
            assert not np.array_equal(rs[0]["llr_out"].view(np.uint64), rs[1]["llr_out"].view(np.uint64))
        else:
            assert not np.array_equal(rs[0][v.changes], rs[1][v.changes])
    # ... and the other min-sum decoders are back when it is off
    v.off(var)
    flooding = {}
    for other in (None,) + v.afterwards:
        for d in (var, fresh):
            if other:
                VARIANTS[other].on(d)
        for early in (True, False):
            rs = []
            for d in (var, fresh):
                d.stream_begin("AWGN", 4, -4.5)
                rs.append(d.stream_decode(32, early_term=early, iterations=50, decoding="BP_MS", want=want))
            for k in want:
                assert np.array_equal(rs[0][k], rs[1][k]), (other, early, k)
            if not other:
                flooding[early] = rs[0]
        for d in (var, fresh):
            if other:
                VARIANTS[other].off(d)
    return flooding


def fold(d, x, frames, seed, channel="AWGN"):
    d.stream_begin(channel, seed, x)
    r = d.stream_decode(frames, early_term=True, iterations=50, decoding="BP_MS", want=("iters", "bit_errors"))
    return frames, int((r["bit_errors"] > 0).sum()), int(r["bit_errors"].sum()), int(r["iters"].sum())


def file_rows(path):
    return [ln.split()[:5] for ln in open(path).read().splitlines()]


def check_simulation_and_cli(v, d, tmp_path, code_file=orc.H_TXT):
    """simulate() with the variant on gives the totals of a host fold of stream_decode over the same frames; the CLI with
    v.flags writes the same result file as the Python run, alone and as two ranks over shared memory; without the flags its
    banner and file are plain min-sum's (v.plain); the command lines of v.refused end non-zero with their texts and write no
    file.  Returns what a test needs to go on: the command line's head and tail, the one-rank run's result file, frames and seed."""
    if v.counter:
        d.set_noise("counter")
    (v.sim_on or v.on)(d)
    frames, xr, seed = 6000, v.xr, 5
    py_file = str(tmp_path / "py.txt")
    res = d.simulate(v.channel, xr, seed=seed, decoding="BP_MS", max_frames=frames, fec=10**9, result_file=py_file,
                     cli_output=True)  # (the result file is written with the console table)
    assert res["totals"].shape == (2, 4)
    for i, x in enumerate(v.points):
        n, fe, be, it = fold(d, x, frames, seed, v.channel)
        assert res["totals"][i].tolist() == [n, fe, be, it], (x, res["totals"][i], (n, fe, be, it))
        assert 0 < fe < n
    head = [os.path.join(ROOT, "libldpc_amd", "ldpcsim"), code_file]
    tail = [str(x) for x in xr] + ["-s", str(seed), "--decoding", "BP_MS", "--max-frames", str(frames), "--frame-error-count", str(10**9)]
    tail += ["--noise", "counter"] * v.counter + ["--channel", v.channel] * (v.channel != "AWGN")
    flags = list(v.flags)
    run = lambda args, **kw: subprocess.run(head + args, stdout=subprocess.PIPE, text=True, timeout=120, **kw)
    one, two = str(tmp_path / "one.txt"), str(tmp_path / "two.txt")
    p = run([one] + tail + flags, check=True)
    for text in v.banner:
        assert text in p.stdout, text
    run([two] + tail + flags + ["--devices", "0,0", "--comm", "shm"], check=True)
    assert file_rows(one) == file_rows(py_file) == file_rows(two)
    if v.plain:
        absent, differs = v.plain
        plain = str(tmp_path / "plain.txt")
        p = run([plain] + tail, check=True)
        assert absent not in p.stdout and (not differs or file_rows(plain) != file_rows(one))
    other = str(tmp_path / "other.txt")
    for bp, args, texts in v.refused:
        p = run([other] + (tail[:5] if bp else tail) + list(args))
        assert p.returncode != 0 and all(t in p.stdout for t in texts), args
    assert not os.path.exists(other)
    return SimpleNamespace(head=head, tail=tail, one=one, frames=frames, seed=seed)


def ran(r, noise, ch, x, early):
    assert r["iters"].max() > 0


def check_fused_channel(d, points=(("AWGN", -5.0), ("BSC", 0.2)), n=64, each=ran):
    """stream_decode with the settings in force == decode_batch of the same frames' dumped llr_in: every point under the
    reference stream and the counter-based noise, with and without early termination; each(r, noise, ch, x, early) sees every
    stream result.  Returns the last one (with llr_in)."""
    for noise in ("reference", "counter"):
        d.set_noise(noise)
        for ch, x in points:
            for early in (True, False):
                d.stream_begin(ch, 6, x)
                r = d.stream_decode(n, early_term=early, iterations=30, decoding="BP_MS", want=WANT + ("llr_in",))
                b = d.decode_batch(r["llr_in"], early_term=early, iterations=30, decoding="BP_MS", want=WANT)
                same(b, r, (noise, ch, x, early))
                each(r, noise, ch, x, early)
    d.set_noise("reference")
    return r
