"""Layered min-sum on the GPU (include/ldpc_amd.h, ldpc_hip_set_min_sum_schedule; kernels_layered_ms.hip) against the numpy
mirror (tests/layered_minsum_ref.py), bit for bit: iters, hard, bit_errors, and llr_out as uint64.  Then the fused channel
paths, the paths that must not move, the simulation loop and the CLI, and what the schedule is for: fewer sweeps."""
import subprocess

import numpy as np
import pytest

import orc
from layered_minsum_ref import LayeredMinSumMirror
from minsum_common import (VARIANTS, WANT, against_mirror, check_fused_channel, check_no_iteration, check_nothing_else_moves,
                           check_simulation_and_cli, check_split_batch, dumped, file_rows, same)
from test_gpu_random_codes import make_code_by_degrees

pytestmark = pytest.mark.gpu


def _flooding(d):
    d.set_min_sum_schedule("flooding")


def _layered(d, llr, s, o, early, iters):
    d.set_min_sum_schedule("layered")
    d.set_min_sum_correction(s, o)
    return d.decode_batch(llr, early_term=early, iterations=iters, decoding="BP_MS", want=WANT)


def _against_mirror(d, mir, llr, corrections, settings):
    """Every (correction, (early, iterations)) against the mirror; returns the mirror's results."""
    out = against_mirror(corrections, settings, lambda c, early, iters: _layered(d, llr, *c, early, iters),
                         lambda c, early, iters: mir.decode(llr, *c, early_term=early, iterations=iters))
    d.set_min_sum_correction()
    d.set_min_sum_schedule("flooding")
    return out


def test_h_txt():
    """h.txt: 24 steps of degree 3 and 4, partial steps of 16 / 32 / 48 lanes, 128 punctured columns; 48 frames at -5.0 dB,
    three corrections, with early termination at 50 iterations and without at 20; tail workgroups (n = 1, 7) and a batch
    split in two."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    code = orc.Code(orc.H_TXT)
    n_steps, step_of = code.layer_steps()
    counts = np.bincount(step_of, minlength=n_steps)
    assert n_steps == 24 and {16, 32, 48, 64} >= set(counts.tolist()) and len(set(counts.tolist())) > 1 and code.num_puncture == 128
    llr = dumped(d, _flooding, "AWGN", -5.0, 48)
    mir = LayeredMinSumMirror(code)
    ms = _against_mirror(d, mir, llr, [(1.0, 0.0), (0.75, 0.0), (0.8125, 0.25)], [(True, 50), (False, 20)])
    m = ms[(1.0, 0.0, True)]
    converged, failed = (m["iters"] < 50) & (m["bit_errors"] == 0), m["bit_errors"] > 0
    assert converged.any() and failed.any(), (int(converged.sum()), int(failed.sum()))
    for n in (1, 7):
        same(_layered(d, llr[:n], 1.0, 0.0, True, 50), m, n, slice(0, n))
    check_split_batch(lambda part: _layered(d, part, 0.75, 0.0, True, 50), llr)
    # no sweep at all: decisions and outputs all zero, as the layered sum-product modes
    check_no_iteration(_layered(d, llr[:3], 1.0, 0.0, True, 0))


def test_8k_code(h8k_file):
    """The 8k (3,6) code: 144 KB of totals and records, the frame that nearly fills a CU's LDS."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(h8k_file)
    assert 140 * 1024 < d.layered_min_sum_lds_bytes() <= 160 * 1024
    llr = dumped(d, _flooding, "AWGN", 1.4, 8)
    _against_mirror(d, LayeredMinSumMirror(orc.Code(h8k_file)), llr, [(1.0, 0.0), (0.8125, 0.0)], [(True, 25), (False, 25)])


def irregular_code(path):
    """237 x 125, every check degree 2..8, variable degrees 1, 2, 3 and one of 22 (its 22 check nodes sit in 22 different
    steps: steps of few lanes, down to one), punctured and shortened columns."""
    rng = np.random.default_rng(20)
    cn = [2] * 10 + [3] * 30 + [4] * 30 + [5] * 20 + [6] * 15 + [7] * 10 + [8] * 10
    vn = [22] + [1] * 20 + [2] * 120 + [3] * 96
    rng.shuffle(cn)
    make_code_by_degrees(path, vn, cn, rng)
    body = open(path).read()
    open(path, "w").write("puncture [3]: 5 40 41\nshorten [2]: 100 230\n" + body)
    return path


def test_irregular_code(tmp_path):
    import libldpc_amd
    path = irregular_code(str(tmp_path / "irregular.txt"))
    code = orc.Code(path)
    assert (code.nc, code.mc, code.num_puncture, code.num_shorten) == (237, 125, 3, 2)
    assert set(np.bincount(code.edge_row).tolist()) == set(range(2, 9))
    vdeg = np.bincount(code.edge_col, minlength=code.nc)
    assert (vdeg == 1).any() and vdeg.max() >= 20 and vdeg.min() >= 1
    n_steps, step_of = code.layer_steps()
    counts = np.bincount(step_of, minlength=n_steps)
    assert n_steps >= 22 and counts.min() == 1 and (counts % 2 == 1).any() and counts.max() < 64
    d = libldpc_amd.HipDecoder(path)
    llr = dumped(d, _flooding, "AWGN", 2.0, 16)
    ms = _against_mirror(d, LayeredMinSumMirror(code), llr, [(1.0, 0.0), (0.8125, 0.25)], [(True, 15), (False, 15)])
    for m in ms.values():
        assert not np.isnan(m["llr_out"]).any()
    m = ms[(1.0, 0.0, True)]
    assert (m["iters"] < 15).any() and (m["bit_errors"] > 0).any()


def test_fused_channel_equals_decode_of_its_llrs():
    """stream_decode with the schedule set == decode_batch of the same frames' dumped llr_in: AWGN and BSC, the reference
    stream and the counter-based noise."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    d.set_min_sum_schedule("layered")
    d.set_min_sum_correction(0.8125, 0.25)
    r = check_fused_channel(d)
    # ... and it is the layered decoder that ran: the mirror on the last frames
    m = LayeredMinSumMirror(orc.Code(orc.H_TXT)).decode(r["llr_in"][:8], 0.8125, 0.25, early_term=False, iterations=30)
    same({k: r[k][:8] for k in WANT}, m, "mirror")


def test_nothing_else_moves():
    """With the schedule set, BP (AWGN, BSC) and BEC outputs equal a fresh context's; after switching back to flooding,
    BP_MS equals a fresh context's."""
    check_nothing_else_moves(VARIANTS["layered"])


def test_simulation_and_cli(tmp_path):
    """simulate() with the schedule gives the totals of a host fold of stream_decode over the same frames; the CLI with
    --ms-schedule layered writes the same result file as the Python run, alone and as two ranks over shared memory."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    v = VARIANTS["layered"]
    run = check_simulation_and_cli(v, d, tmp_path)
    # without the flag: today's output and file (flooding, normalized: its own NON-PARITY line, no schedule line)
    d.set_min_sum_schedule("flooding")
    flood_py, flood = str(tmp_path / "flood_py.txt"), str(tmp_path / "flood.txt")
    d.simulate("AWGN", v.xr, seed=run.seed, decoding="BP_MS", max_frames=run.frames, fec=10**9, result_file=flood_py, cli_output=True)
    p = subprocess.run(run.head + [flood] + run.tail + list(v.flags[2:]), stdout=subprocess.PIPE, text=True, timeout=120, check=True)
    assert "Min-Sum Schedule" not in p.stdout and file_rows(flood) == file_rows(flood_py) != file_rows(run.one)


def test_what_it_is_for():
    """h.txt, AWGN -3.5 dB, plain min-sum, the same 8 192 frames of one stream under both schedules: over the frames both
    converge on, the layered schedule needs fewer than 0.7 of the flooding iterations (CPU prototype: 0.56), and it is still
    a decoder: fer_layered < 2 fer_flooding + 0.005."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    N, r = 8192, {}
    for sched in ("flooding", "layered"):
        d.set_min_sum_schedule(sched)
        d.stream_begin("AWGN", 1, -3.5)
        r[sched] = d.stream_decode(N, early_term=True, iterations=50, decoding="BP_MS", want=("iters", "bit_errors"))
    both = (r["flooding"]["iters"] < 50) & (r["layered"]["iters"] < 50)
    sweeps, its = r["layered"]["iters"][both].mean(), r["flooding"]["iters"][both].mean()
    fer = {k: float((v["bit_errors"] > 0).mean()) for k, v in r.items()}
    print("sweeps", sweeps, "iterations", its, "ratio", sweeps / its, "fer", fer, "both", int(both.sum()))
    assert both.sum() > N // 2 and sweeps < 0.7 * its
    assert fer["layered"] < 2 * fer["flooding"] + 0.005
