"""Corrected min-sum on the GPU (include/ldpc_amd.h, ldpc_hip_set_min_sum_correction): every decoder residency against the
numpy mirror (tests/minsum_ref.py) bit for bit, the fused channel paths, the paths that must not move, the simulation loop
and the CLI, and the error-rate gain on the 8k (3,6)-regular code."""
import math
import zlib

import numpy as np
import pytest

import orc
from minsum_common import VARIANTS, WANT, check_fused_channel, check_nothing_else_moves, check_simulation_and_cli, same
from minsum_ref import MinSumMirror
from test_gpu_random_codes import make_code

pytestmark = pytest.mark.gpu
CORRECTIONS = [(0.75, 0.0), (1.0, 0.5), (0.8125, 0.25)]


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
            same(r, mir.decode(llr, s, o, early_term=early, iterations=iters), (s, o, early))
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
    check_fused_channel(d, pts, n, each=lambda *a: None)


def test_nothing_else_moves():
    """With (0.75, 0.25) set, BP and BEC outputs equal a fresh context's; after resetting to (1, 0) BP_MS equals a fresh
    context's plain BP_MS and the det oracle."""
    flooding = check_nothing_else_moves(VARIANTS["correction"])
    code = orc.Code(orc.H_TXT, orc.G_TXT)
    for early in (True, False):
        o = code.run_frames("AWGN", -4.5, seed=4, count=4, min_sum=True, early_term=early, iters=50, math=orc.MATH_DET)
        for k in ("iters", "hard", "llr_out", "bit_errors"):
            assert np.array_equal(flooding[early][k][:4], o[k].astype(flooding[early][k].dtype)), (early, k)


def test_simulation_and_cli(tmp_path):
    """simulate() with the correction gives the totals of a host fold of stream_decode over the same frames; the CLI with
    --ms-scale / --ms-offset writes the same result file as the Python run, alone and as two ranks over shared memory."""
    import libldpc_amd
    check_simulation_and_cli(VARIANTS["correction"], libldpc_amd.HipDecoder(orc.H_TXT), tmp_path)


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
