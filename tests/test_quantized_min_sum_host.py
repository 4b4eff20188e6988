"""Quantized min-sum (include/ldpc_amd.h, ldpc_hip_set_min_sum_quantization) without a GPU: the setter's validity check,
the codes it takes, the launch stages it reports, and the numpy mirror (tests/quantized_minsum_ref.py) by itself — against the
binary64 mirror where the two must agree, and on what quantization costs."""
import os
import sys

import numpy as np
import pytest

import orc
from minsum_common import check_decode_stages, write
from minsum_ref import MinSumMirror
from quantized_minsum_ref import QuantizedMinSumMirror, correction_table, quantize

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


def test_setter_accepts_and_rejects(lib):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    assert d.min_sum_quantization == (0, 1.0)  # off by default
    for bits in range(2, 9):
        d.set_min_sum_quantization(bits, 0.25 * bits)
        assert d.min_sum_quantization == (bits, 0.25 * bits)
    d.set_min_sum_quantization(6, 0.25)
    bad = [(1, 0.25), (9, 0.25), (-1, 0.25)] + [(5, s) for s in (0.0, -1.0, float("nan"), float("inf"), 1e-30)]
    for bits, step in bad:
        with pytest.raises(RuntimeError, match="ldpc_hip_set_min_sum_quantization"):
            d.set_min_sum_quantization(bits, step)
        assert lib.ldpc_hip_set_min_sum_quantization(d.ctx, bits, step) == -1 and len(lib.ldpc_hip_last_error()) > 0
        assert d.min_sum_quantization == (6, 0.25), (bits, step)  # unchanged
    # the edges of the step's range
    d.set_min_sum_quantization(4, 2.0 ** -20)
    d.set_min_sum_quantization(4, 2.0 ** 20)
    assert d.min_sum_quantization == (4, 2.0 ** 20)
    d.set_min_sum_quantization(0, float("nan"))  # off: the step is ignored
    assert d.min_sum_quantization[0] == 0
    d.set_min_sum_quantization()
    assert d.min_sum_quantization[0] == 0


def test_layered_schedule_and_quantization_exclude_each_other(lib):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    d.set_min_sum_quantization(6, 0.25)
    with pytest.raises(RuntimeError, match="ldpc_hip_set_min_sum_schedule"):
        d.set_min_sum_schedule("layered")
    assert lib.ldpc_hip_last_error()
    assert d.min_sum_schedule == "flooding" and d.min_sum_quantization == (6, 0.25)
    d.set_min_sum_schedule("flooding")  # (the schedule in force may be set again)
    d.set_min_sum_quantization(0)
    d.set_min_sum_schedule("layered")
    with pytest.raises(RuntimeError, match="ldpc_hip_set_min_sum_quantization"):
        d.set_min_sum_quantization(6, 0.25)
    assert lib.ldpc_hip_last_error()
    assert d.min_sum_schedule == "layered" and d.min_sum_quantization[0] == 0
    d.set_min_sum_quantization(0)  # switching it off is always taken
    d.set_min_sum_schedule("flooding")
    d.set_min_sum_quantization(6, 0.25)
    assert d.min_sum_quantization == (6, 0.25)


def _lds_bytes(code):
    """The formula beside ldpc_hip_quantized_min_sum_lds_bytes."""
    slots = int(((np.bincount(code.edge_row, minlength=code.mc) + 3) // 4 * 4).sum())
    work = (max(8 * code.nc, slots + 4 * code.nc + 144) + 3) // 4 * 4
    return (work + code.nc + 15) // 16 * 16


def test_codes(lib, tmp_path, h8k_file):
    import libldpc_amd
    for path in (orc.H_TXT, h8k_file):
        d = libldpc_amd.HipDecoder(path)
        assert d.quantized_min_sum_lds_bytes() == _lds_bytes(orc.Code(path)) <= 160 * 1024
    # the 8k code: 8 x fewer bytes per message than binary64, two frames per CU
    assert 2 * libldpc_amd.HipDecoder(h8k_file).quantized_min_sum_lds_bytes() <= 160 * 1024
    # what the layered modes refuse: a check node wider than 8, an isolated column
    base = [[0, 1, 2], [2, 3, 4], [4, 5, 0], [1, 3, 5]]
    cases = {
        "degree9_row": base + [list(range(9))],
        "isolated_column": [[0, 1, 2], [2, 3, 5], [5, 6, 0], [1, 3, 6]],  # column 4 has no edge
    }
    for name, rows in cases.items():
        path = write(tmp_path / f"{name}.txt", rows)
        dd = libldpc_amd.HipDecoder(path)
        with pytest.raises(RuntimeError, match="ldpc_hip_set_min_sum_schedule"):
            dd.set_min_sum_schedule("layered")
        dd.set_min_sum_quantization(5, 0.5)
        assert dd.min_sum_quantization == (5, 0.5), name
        assert dd.quantized_min_sum_lds_bytes() == _lds_bytes(orc.Code(path)), name
    # messages alone beyond 160 KB: 30 000 columns, 21 000 check nodes of degree 8 = 168 000 edges
    nc = 30000
    rows = [sorted({(8 * i + j * (1 + i // 2500)) % nc for j in range(8)}) for i in range(21000)]
    assert all(len(r) == 8 for r in rows) and sum(len(r) for r in rows) > 163840
    big = libldpc_amd.HipDecoder(write(tmp_path / "big.txt", rows))
    assert big.quantized_min_sum_lds_bytes() == -1
    with pytest.raises(RuntimeError, match="LDS"):
        big.set_min_sum_quantization(6, 0.25)
    assert lib.ldpc_hip_set_min_sum_quantization(big.ctx, 6, 0.25) == -1 and b"LDS" in lib.ldpc_hip_last_error()
    assert big.min_sum_quantization[0] == 0


def test_decode_stages(lib, h8k_file):
    """One `whole` launch for BP_MS while quantization is on; BP keeps its stages; everything back when it is off."""
    import libldpc_amd
    for path in (orc.H_TXT, h8k_file):
        check_decode_stages(libldpc_amd.HipDecoder(path), lambda d: d.set_min_sum_quantization(6, 0.25),
                            lambda d: d.set_min_sum_quantization(0))


def test_table():
    assert correction_table(6, 0.25).tolist() == list(range(32))  # (1, 0): the identity
    assert correction_table(2, 7.0).tolist() == [0, 1] and correction_table(8, 0.0625).tolist() == list(range(128))
    t = correction_table(6, 0.25, 0.8125, 0.0)
    assert len(t) == 32 and t[[1, 2, 3, 4]].tolist() == [1, 2, 2, 3]  # 0.8125, 1.625 (-> 2), 2.4375, 3.25
    for bits, step, s, o in ((5, 0.5, 0.75, 0.5), (8, 0.0625, 0.8125, 0.1), (4, 1.0, 0.5, 3.0)):
        t = correction_table(bits, step, s, o)
        assert t[0] == 0 and (np.diff(t) >= 0).all() and (t <= np.arange(len(t))).all(), (bits, step, s, o)
    assert correction_table(5, 0.5, 0.75, 0.5).tolist()[:5] == [0, 0, 0, 1, 2]  # 0.75 m - 1: rint(-0.25), 0.5 -> 0, 1.25, 2


def test_quantizer():
    x = np.array([0.0, 0.124, 0.125, 0.126, 0.375, -0.125, -0.375, 7.75, 7.8, -7.9, 99999.9, np.inf, -np.inf, np.nan])
    assert quantize(x, 6, 0.25).tolist() == [0, 0, 0, 1, 2, 0, -2, 31, 31, -31, 31, 31, -31, 0]  # halves go to even
    assert quantize(np.array([-5.0, 5.0, 0.4, 1.0]), 2, 2.0).tolist() == [-1, 1, 0, 0]


def test_mirror_equals_the_float_mirror_where_nothing_rounds_or_saturates(tmp_path):
    """(3,6)-regular code, channel values L in {-1, 1, 3} steps: every message that is read is an odd number of steps —
    never zero, so the sign conventions of the two mirrors cannot differ — and at most 3 (2^5 - 1) = 93 <= 127 after 5
    iterations, so 8 bits never saturate: iters, hard, bit_errors and llr_out equal MinSumMirror's on the same LLRs."""
    import gen_regular_code
    path = tmp_path / "r96.txt"
    path.write_text(gen_regular_code.generate(96, 3, 6, 5))
    code = orc.Code(str(path))
    rng = np.random.default_rng(7)
    L = rng.choice([-1] + [1] * 9 + [3] * 10, size=(64, code.nc))
    llr = L * 0.5
    seen = set()
    for early in (True, False):
        f = MinSumMirror(code).decode(llr, early_term=early, iterations=5)
        q = QuantizedMinSumMirror(code).decode(llr, 8, 0.5, early_term=early, iterations=5)
        for k in ("iters", "hard", "bit_errors", "llr_out"):
            assert np.array_equal(np.asarray(f[k]), np.asarray(q[k])), (early, k)
        assert np.abs(q["llr_out"]).max() <= 127 * 0.5
        if early:
            seen = set(q["iters"].tolist())
            assert (q["bit_errors"] > 0).any() and (q["iters"] < 5).any()
    assert seen == set(range(6))  # frames stop at every count


def _awgn_llrs(code, snr_db, n, seed):
    """All-zero codewords over AWGN with numpy's normals: LLR 2 y / sigma^2, punctured columns 0."""
    rng = np.random.default_rng(seed)
    sigma2 = 10.0 ** (-snr_db / 10.0)
    llr = np.zeros((n, code.nc))
    llr[:, code.bit_pos] = 2.0 * (1.0 + np.sqrt(sigma2) * rng.standard_normal((n, code.nct))) / sigma2
    return llr


def test_mirror_what_it_is_for():
    """h.txt, AWGN -4 dB, 256 frames, 50 iterations with early termination: 6 bits at step 0.25 decode like binary64
    (failures <= 1.5 x), 4 bits at step 1.0 cost frames (failures >= 2 x).  Measured: 12, 12 and 34 failing frames."""
    code = orc.Code(orc.H_TXT)
    llr = _awgn_llrs(code, -4.0, 256, seed=2)
    flo = int((MinSumMirror(code).decode(llr)["bit_errors"] > 0).sum())
    mir = QuantizedMinSumMirror(code)
    q6 = int((mir.decode(llr, 6, 0.25)["bit_errors"] > 0).sum())
    q4 = int((mir.decode(llr, 4, 1.0)["bit_errors"] > 0).sum())
    print("failing frames: binary64", flo, "6 bits / 0.25", q6, "4 bits / 1.0", q4)
    assert flo > 0
    assert q6 <= 1.5 * flo
    assert q4 >= 2 * flo
