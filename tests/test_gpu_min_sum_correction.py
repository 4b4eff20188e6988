"""Corrected min-sum on the GPU (include/ldpc_amd.h, ldpc_hip_set_min_sum_correction): every decoder residency against the
numpy mirror (tests/minsum_ref.py) bit for bit, the fused channel paths, the paths that must not move, the simulation loop
and the CLI, and the error-rate gain on the 8k (3,6)-regular code."""
import math
import os
import subprocess
import zlib

import numpy as np
import pytest

import orc
from minsum_ref import MinSumMirror
from test_gpu_random_codes import make_code

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORRECTIONS = [(0.75, 0.0), (1.0, 0.5), (0.8125, 0.25)]
WANT = ("iters", "hard", "llr_out", "bit_errors")


def _same(r, m, what):
    for k in WANT:
        a, b = r[k], np.asarray(m[k]).astype(r[k].dtype)
        if k == "llr_out":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (what, k)


def _dumped(d, ch, x, n, seed=3):
    """llr_in of n frames of the reference stream (the inputs some of which plain min-sum fails on)."""
    d.set_min_sum_correction()
    d.stream_begin(ch, seed, x)
    r = d.stream_decode(n, decoding="BP_MS", want=("llr_in", "bit_errors"))
    return r["llr_in"], r["bit_errors"]


def _against_mirror(d, mir, llr, iters=20, earlies=(True, False)):
    for s, o in CORRECTIONS:
        d.set_min_sum_correction(s, o)
        for early in earlies:
            r = d.decode_batch(llr, early_term=early, iterations=iters, decoding="BP_MS", want=WANT)
            _same(r, mir.decode(llr, s, o, early_term=early, iterations=iters), (s, o, early))
    d.set_min_sum_correction()


def test_h_txt_fused_and_lds():
    """h.txt: the fused plan's min-sum kernel without early termination, the general LDS-resident one with it."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    assert d.residency == "lds" and d.fused_plan()["ok"]
    llr, be = _dumped(d, "AWGN", -5.0, 48)
    assert (be > 0).any() and (be == 0).any()
    _against_mirror(d, MinSumMirror(orc.Code(orc.H_TXT)), llr, iters=50)


def test_8k_totals_form(h8k_file):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(h8k_file)
    assert d.residency == "registers" and d.register_form == "totals"
    llr, be = _dumped(d, "AWGN", 1.4, 12)
    assert (be > 0).any()
    _against_mirror(d, MinSumMirror(orc.Code(h8k_file)), llr, iters=25)


RANDOM = [
    # name, nc, mc, CN degree pool, puncture, shorten, skipped columns, residency, register form, x
    ("lds_wide_cn", 600, 200, [5, 6, 7, 8], (), (10, 11), (3,), "lds", None, 1.0),
    ("reg_tile_8x4", 9000, 6000, [3, 4], (1, 2, 3), (), (7,), "registers", "messages", 1.0),
    ("mem_cn12", 900, 100, [9, 12, 16], (), (), (), "memory", None, 1.0),
    ("mem_cn20", 1200, 120, [20], (), (), (), "memory", None, 3.0),
]


@pytest.mark.parametrize("case", RANDOM, ids=[c[0] for c in RANDOM])
def test_random_codes(case, tmp_path):
    import libldpc_amd
    name, nc, mc, pool, punct, short, skip, residency, form, x = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    path = make_code(str(tmp_path / f"{name}.txt"), nc, mc, rng.choice(pool, size=mc), rng, punct, short, skip)
    code = orc.Code(path)
    d = libldpc_amd.HipDecoder(path)
    assert d.residency == residency, d.residency
    if form:
        assert d.register_form == form
    if name == "reg_tile_8x4":
        assert (np.bincount(code.edge_col, minlength=code.nc) == 1).any()  # degree-1 variable nodes
    llr, _ = _dumped(d, "AWGN", x, 8)
    _against_mirror(d, MinSumMirror(code), llr, iters=15)


@pytest.mark.parametrize("code_name", ["h", "8k"])
def test_fused_channel_equals_decode_of_its_llrs(code_name, h8k_file):
    """stream_decode with the correction == decode_batch of the same frames' dumped llr_in: AWGN and BSC, the reference
    stream and the counter-based noise, with and without early termination."""
    import libldpc_amd
    path = orc.H_TXT if code_name == "h" else h8k_file
    d = libldpc_amd.HipDecoder(path)
    pts = {"h": (("AWGN", -5.0), ("BSC", 0.2)), "8k": (("AWGN", 1.5), ("BSC", 0.07))}[code_name]
    n = 64 if code_name == "h" else 16
    d.set_min_sum_correction(0.8125, 0.25)
    for noise in ("reference", "counter"):
        d.set_noise(noise)
        for ch, x in pts:
            for early in (True, False):
                d.stream_begin(ch, 6, x)
                r = d.stream_decode(n, early_term=early, iterations=30, decoding="BP_MS", want=WANT + ("llr_in",))
                b = d.decode_batch(r["llr_in"], early_term=early, iterations=30, decoding="BP_MS", want=WANT)
                _same(b, r, (noise, ch, x, early))
    d.set_noise("reference")


def test_nothing_else_moves():
    """With (0.75, 0.25) set, BP and BEC outputs equal a fresh context's; after resetting to (1, 0) BP_MS equals a fresh
    context's plain BP_MS and the det oracle."""
    import libldpc_amd
    want = ("iters", "hard", "llr_out", "bit_errors", "llr_in")
    corr = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    fresh = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    corr.set_min_sum_correction(0.75, 0.25)
    for ch, x, dec, early in (("AWGN", -4.0, "BP", True), ("AWGN", -4.0, "BP", False), ("BSC", 0.24, "BP", True),
                              ("BEC", 0.7, "BP", True), ("BEC", 0.7, "BP_MS", True)):
        rs = []
        for d in (corr, fresh):
            d.stream_begin(ch, 2, x)
            rs.append(d.stream_decode(64, early_term=early, iterations=50, decoding=dec, want=want))
        for k in want:
            assert np.array_equal(rs[0][k], rs[1][k]), (ch, dec, early, k)
        llr = rs[1]["llr_in"]
        if ch != "BEC":
            a = corr.decode_batch(llr, early_term=early, decoding=dec, want=WANT)
            b = fresh.decode_batch(llr, early_term=early, decoding=dec, want=WANT)
            for k in WANT:
                assert np.array_equal(a[k], b[k]), (ch, dec, k)
    corr.set_min_sum_correction(1.0, 0.0)
    code = orc.Code(orc.H_TXT, orc.G_TXT)
    for early in (True, False):
        rs = []
        for d in (corr, fresh):
            d.stream_begin("AWGN", 4, -4.5)
            rs.append(d.stream_decode(32, early_term=early, iterations=50, decoding="BP_MS", want=want))
        for k in want:
            assert np.array_equal(rs[0][k], rs[1][k]), (early, k)
        o = code.run_frames("AWGN", -4.5, seed=4, count=4, min_sum=True, early_term=early, iters=50, math=orc.MATH_DET)
        for k in ("iters", "hard", "llr_out", "bit_errors"):
            assert np.array_equal(rs[0][k][:4], o[k].astype(rs[0][k].dtype)), (early, k)


def _fold(d, x, frames, seed):
    d.stream_begin("AWGN", seed, x)
    r = d.stream_decode(frames, early_term=True, iterations=50, decoding="BP_MS", want=("iters", "bit_errors"))
    return frames, int((r["bit_errors"] > 0).sum()), int(r["bit_errors"].sum()), int(r["iters"].sum())


def _file_rows(path):
    return [ln.split()[:5] for ln in open(path).read().splitlines()]


def test_simulation_and_cli(tmp_path):
    """simulate() with the correction gives the totals of a host fold of stream_decode over the same frames; the CLI with
    --ms-scale / --ms-offset writes the same result file as the Python run, alone and as two ranks over shared memory."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    d.set_min_sum_correction(0.8125, 0.25)
    frames, xr, seed = 6000, (-4.5, -3.5, 0.5), 5
    py_file = str(tmp_path / "py.txt")
    res = d.simulate("AWGN", xr, seed=seed, decoding="BP_MS", max_frames=frames, fec=10**9, result_file=py_file,
                     cli_output=True)  # (the result file is written with the console table)
    assert res["totals"].shape == (2, 4)
    for i, x in enumerate((-4.5, -4.0)):
        n, fe, be, it = _fold(d, x, frames, seed)
        assert res["totals"][i].tolist() == [n, fe, be, it], (x, res["totals"][i], (n, fe, be, it))
        assert 0 < fe < n
    exe = os.path.join(ROOT, "libldpc_amd", "ldpcsim")
    args = [exe, orc.H_TXT, "", "-4.5", "-3.5", "0.5", "-s", str(seed), "--decoding", "BP_MS", "--ms-scale", "0.8125",
            "--ms-offset", "0.25", "--max-frames", str(frames), "--frame-error-count", str(10**9)]
    one, two = str(tmp_path / "one.txt"), str(tmp_path / "two.txt")
    p = subprocess.run(args[:2] + [one] + args[3:], stdout=subprocess.PIPE, text=True, timeout=120, check=True)
    assert "NON-PARITY" in p.stdout and "Min-Sum Correction" in p.stdout
    subprocess.run(args[:2] + [two] + args[3:] + ["--devices", "0,0", "--comm", "shm"], stdout=subprocess.PIPE, text=True,
                   timeout=120, check=True)
    assert _file_rows(one) == _file_rows(py_file) == _file_rows(two)
    # without the flags: plain min-sum, no NON-PARITY line
    plain = str(tmp_path / "plain.txt")
    p = subprocess.run(args[:2] + [plain] + args[3:10] + args[14:], stdout=subprocess.PIPE, text=True, timeout=120, check=True)
    assert "NON-PARITY" not in p.stdout and _file_rows(plain) != _file_rows(one)


def test_normalized_min_sum_helps(h8k_file):
    """NMS beats plain BP_MS on the 8k (3,6)-regular code.  Point and scale from the sweep in
    profiles/min_sum_correction_fer.jsonl (counter noise, seed 1, 65 536 frames, 50 iterations, early termination), FER at
    1.4 / 1.6 / 1.8 dB: BP_MS 0.992 / 0.802 / 0.238, NMS 0.75 0.153 / 0.0049 / 0, NMS 0.8125 0.107 / 0.0026 / 0, BP
    0.041 / 0.00066 / 0.  At 1.6 dB with scale 0.8125 the gap is some 500 standard errors; 5 are asked for."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(h8k_file)
    d.set_noise("counter")
    N, B, x = 65536, 8192, 1.6
    fer = {}
    for s in (1.0, 0.8125):
        d.set_min_sum_correction(s, 0.0)
        d.stream_begin("AWGN", 1, x)
        fails = sum(int((d.stream_decode(B, decoding="BP_MS")["bit_errors"] > 0).sum()) for _ in range(N // B))
        fer[s] = fails / N
    p_ms, p_nms = fer[1.0], fer[0.8125]
    se = math.sqrt(p_ms * (1 - p_ms) / N + p_nms * (1 - p_nms) / N)
    assert p_ms - p_nms >= 5 * se, fer
