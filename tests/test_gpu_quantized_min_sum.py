"""Quantized min-sum on the GPU (include/ldpc_amd.h, ldpc_hip_set_min_sum_quantization; kernels_qms.hip) against the numpy
mirror (tests/quantized_minsum_ref.py), bit for bit: iters, hard, bit_errors, and llr_out as uint64.  Then the fused channel
paths, the paths that must not move, the simulation loop and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import orc
from minsum_common import WANT, against_mirror, check_no_iteration, check_split_batch, dumped, same
from quantized_minsum_ref import QuantizedMinSumMirror, quantize
from test_gpu_random_codes import make_code_by_degrees

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (bits, step, scale, offset)
H_SETTINGS = [(6, 0.25, 1.0, 0.0), (6, 0.25, 0.8125, 0.0), (5, 0.5, 0.75, 0.5), (4, 1.0, 1.0, 0.0), (4, 0.25, 1.0, 0.0),
              (2, 2.0, 1.0, 0.0), (8, 0.0625, 0.8125, 0.1)]


def _binary64(d):
    d.set_min_sum_quantization(0)


def _quantized(d, llr, setting, early, iters):
    bits, step, s, o = setting
    d.set_min_sum_quantization(bits, step)
    d.set_min_sum_correction(s, o)
    return d.decode_batch(llr, early_term=early, iterations=iters, decoding="BP_MS", want=WANT)


def _against_mirror(d, mir, llr, settings, runs):
    """Every (setting, (early, iterations)) against the mirror; returns the mirror's results."""
    out = against_mirror(settings, runs, lambda st, early, iters: _quantized(d, llr, st, early, iters),
                         lambda st, early, iters: mir.decode(llr, *st, early_term=early, iterations=iters))
    d.set_min_sum_correction()
    d.set_min_sum_quantization(0)
    return out


@pytest.fixture(scope="module")
def h_txt():
    """h.txt, 48 frames of the reference stream at -5.0 dB, and a cache of the mirror's results on them."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    return {"d": d, "llr": dumped(d, _binary64, "AWGN", -5.0, 48), "mir": QuantizedMinSumMirror(orc.Code(orc.H_TXT)), "ref": {}}


def _h_ref(h, st, early, iters):
    key = st + (early, iters)
    if key not in h["ref"]:
        bits, step, s, o = st
        h["ref"][key] = h["mir"].decode(h["llr"], bits, step, s, o, early_term=early, iterations=iters)
    return h["ref"][key]


@pytest.mark.parametrize("setting", H_SETTINGS, ids=lambda s: "q%d_step%g_a%g_b%g" % s)
def test_h_txt(h_txt, setting):
    """Seven settings, each with early termination at 50 iterations and without at 20."""
    d, llr = h_txt["d"], h_txt["llr"]
    for early, iters in ((True, 50), (False, 20)):
        same(_quantized(d, llr, setting, early, iters), _h_ref(h_txt, setting, early, iters), (setting, early))
    bits, step = setting[:2]
    sat = float((np.abs(quantize(llr, bits, step)) == (1 << (bits - 1)) - 1).mean())
    print(setting, "channel values at +-Qmax:", sat)
    if setting == (4, 0.25, 1.0, 0.0):
        assert sat > 0.05  # the heavy channel saturation case
    if setting == (6, 0.25, 1.0, 0.0):
        m = _h_ref(h_txt, setting, True, 50)
        converged, failed = (m["iters"] < 50) & (m["bit_errors"] == 0), m["bit_errors"] > 0
        assert converged.any() and failed.any(), (int(converged.sum()), int(failed.sum()))
    d.set_min_sum_correction()
    d.set_min_sum_quantization(0)


def test_h_txt_batches(h_txt):
    """Batches of n = 1 and 7, one batch split in two, and no iteration at all."""
    d, llr = h_txt["d"], h_txt["llr"]
    st = (6, 0.25, 1.0, 0.0)
    m = _h_ref(h_txt, st, True, 50)
    for n in (1, 7):
        same(_quantized(d, llr[:n], st, True, 50), m, n, slice(0, n))
    st2 = (5, 0.5, 0.75, 0.5)
    one = check_split_batch(lambda part: _quantized(d, part, st2, True, 50), llr)
    same(one, _h_ref(h_txt, st2, True, 50), "whole batch")
    for early in (True, False):
        check_no_iteration(_quantized(d, llr[:3], st, early, 0))
    d.set_min_sum_correction()
    d.set_min_sum_quantization(0)


def test_8k_code(h8k_file):
    """The 8k (3,6) code: check nodes of degree 6 in two words each, 32 variable nodes per thread."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(h8k_file)
    assert 0 < 2 * d.quantized_min_sum_lds_bytes() <= 160 * 1024
    llr = dumped(d, _binary64, "AWGN", 1.4, 8)
    _against_mirror(d, QuantizedMinSumMirror(orc.Code(h8k_file)), llr, [(6, 0.25, 1.0, 0.0), (5, 0.5, 0.8125, 0.0)],
                    [(True, 25), (False, 25)])


def wide_irregular_code(path):
    """243 x 109, 586 edges: check degrees 2..40 (rows of one word up to ten, with and without padding), variable degrees
    1, 2, 3 and one of 22, punctured and shortened columns."""
    rng = np.random.default_rng(21)
    cn = [2] * 10 + [3] * 30 + [4] * 30 + [6] * 20 + [9] * 10 + [12] * 6 + [17] * 2 + [40]
    vn = [22] + [1] * 20 + [2] * 122 + [3] * 100
    rng.shuffle(cn)
    make_code_by_degrees(path, vn, cn, rng)
    body = open(path).read()
    open(path, "w").write("puncture [3]: 5 40 41\nshorten [2]: 100 230\n" + body)
    return path


def test_wide_irregular_code(tmp_path):
    import libldpc_amd
    path = wide_irregular_code(str(tmp_path / "wide.txt"))
    code = orc.Code(path)
    assert (code.nc, code.mc, code.nnz, code.num_puncture, code.num_shorten) == (243, 109, 586, 3, 2)
    rdeg = np.bincount(code.edge_row, minlength=code.mc)
    assert rdeg.max() > 32 and ((rdeg >= 9) & (rdeg <= 16)).any() and rdeg.min() >= 2
    vdeg = np.bincount(code.edge_col, minlength=code.nc)
    assert (vdeg == 1).any() and vdeg.max() >= 20 and code.nc % 64 != 0
    d = libldpc_amd.HipDecoder(path)
    with pytest.raises(RuntimeError):
        d.set_min_sum_schedule("layered")  # (a code the layered kernel refuses)
    llr = dumped(d, _binary64, "AWGN", 2.0, 16)
    assert (np.abs(llr) > 90000).any() and (llr == 0).any()  # shortened columns saturate, punctured ones are zero
    ms = _against_mirror(d, QuantizedMinSumMirror(code), llr, [(6, 0.25, 1.0, 0.0), (5, 0.5, 0.8125, 0.25)],
                         [(True, 15), (False, 15)])
    m = ms[(6, 0.25, 1.0, 0.0, True)]
    assert (m["iters"] < 15).any()


def test_fused_channel_equals_decode_of_its_llrs():
    """stream_decode with quantization on == decode_batch of the same frames' dumped llr_in: AWGN and BSC, the reference
    stream and the counter-based noise."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    d.set_min_sum_quantization(5, 0.5)
    d.set_min_sum_correction(0.8125, 0.25)
    for noise in ("reference", "counter"):
        d.set_noise(noise)
        for ch, x in (("AWGN", -5.0), ("BSC", 0.2)):
            for early in (True, False):
                d.stream_begin(ch, 6, x)
                r = d.stream_decode(64, early_term=early, iterations=30, decoding="BP_MS", want=WANT + ("llr_in",))
                b = d.decode_batch(r["llr_in"], early_term=early, iterations=30, decoding="BP_MS", want=WANT)
                same(b, r, (noise, ch, x, early))
                assert r["iters"].max() > 0
    d.set_noise("reference")
    # ... and it is the quantized decoder that ran: the mirror on the last frames
    m = QuantizedMinSumMirror(orc.Code(orc.H_TXT)).decode(r["llr_in"][:8], 5, 0.5, 0.8125, 0.25, early_term=False, iterations=30)
    same({k: r[k][:8] for k in WANT}, m, "mirror")


def test_nothing_else_moves():
    """With quantization on, BP (AWGN, BSC) and BEC outputs equal a fresh context's; with it off again, BP_MS — flooding,
    and then layered — equals a fresh context's."""
    import libldpc_amd
    want = ("iters", "hard", "llr_out", "bit_errors", "llr_in")
    qms = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    fresh = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    qms.set_min_sum_quantization(6, 0.25)
    for ch, x, dec, early in (("AWGN", -4.0, "BP", True), ("AWGN", -4.0, "BP", False), ("BSC", 0.24, "BP", True),
                              ("BEC", 0.7, "BP", True), ("BEC", 0.7, "BP_MS", True)):
        rs = []
        for d in (qms, fresh):
            d.stream_begin(ch, 2, x)
            rs.append(d.stream_decode(64, early_term=early, iterations=50, decoding=dec, want=want))
        for k in want:
            assert np.array_equal(rs[0][k], rs[1][k]), (ch, dec, early, k)
        if ch != "BEC":
            a = qms.decode_batch(rs[1]["llr_in"], early_term=early, decoding=dec, want=WANT)
            b = fresh.decode_batch(rs[1]["llr_in"], early_term=early, decoding=dec, want=WANT)
            for k in WANT:
                assert np.array_equal(a[k], b[k]), (ch, dec, k)
    # quantization does change BP_MS ...
    rs = []
    for d in (qms, fresh):
        d.stream_begin("AWGN", 4, -4.5)
        rs.append(d.stream_decode(32, iterations=50, decoding="BP_MS", want=want))
    assert np.array_equal(rs[0]["llr_in"], rs[1]["llr_in"])
    assert not np.array_equal(rs[0]["llr_out"].view(np.uint64), rs[1]["llr_out"].view(np.uint64))
    # ... and binary64 min-sum is back when it is off: flooding, then layered
    qms.set_min_sum_quantization(0)
    for sched in ("flooding", "layered"):
        for d in (qms, fresh):
            d.set_min_sum_schedule(sched)
        for early in (True, False):
            rs = []
            for d in (qms, fresh):
                d.stream_begin("AWGN", 4, -4.5)
                rs.append(d.stream_decode(32, early_term=early, iterations=50, decoding="BP_MS", want=want))
            for k in want:
                assert np.array_equal(rs[0][k], rs[1][k]), (sched, early, k)


def _fold(d, x, frames, seed):
    d.stream_begin("AWGN", seed, x)
    r = d.stream_decode(frames, early_term=True, iterations=50, decoding="BP_MS", want=("iters", "bit_errors"))
    return frames, int((r["bit_errors"] > 0).sum()), int(r["bit_errors"].sum()), int(r["iters"].sum())


def _file_rows(path):
    return [ln.split()[:5] for ln in open(path).read().splitlines()]


def test_simulation_and_cli(tmp_path):
    """simulate() with quantization and counter noise gives the totals of a host fold of stream_decode over the same frames;
    the CLI with --ms-bits 6 --ms-step 0.25 --noise counter writes the same result file as the Python run, alone and as two
    ranks over shared memory; --ms-bits is refused with BP and with --ms-schedule layered."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    d.set_noise("counter")
    d.set_min_sum_quantization(6, 0.25)
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
    head = [exe, orc.H_TXT]
    tail = ["-4.5", "-3.5", "0.5", "-s", str(seed), "--decoding", "BP_MS", "--max-frames", str(frames),
            "--frame-error-count", str(10**9), "--noise", "counter"]
    flags = ["--ms-bits", "6", "--ms-step", "0.25"]
    one, two = str(tmp_path / "one.txt"), str(tmp_path / "two.txt")
    p = subprocess.run(head + [one] + tail + flags, stdout=subprocess.PIPE, text=True, timeout=120, check=True)
    assert "Min-Sum Quantization: 6 bits, step 0.25" in p.stdout and "NON-PARITY" in p.stdout
    subprocess.run(head + [two] + tail + flags + ["--devices", "0,0", "--comm", "shm"], stdout=subprocess.PIPE, text=True,
                   timeout=120, check=True)
    assert _file_rows(one) == _file_rows(py_file) == _file_rows(two)
    # without the flags: binary64 min-sum, another file and no quantization line
    plain = str(tmp_path / "plain.txt")
    p = subprocess.run(head + [plain] + tail, stdout=subprocess.PIPE, text=True, timeout=120, check=True)
    assert "Min-Sum Quantization" not in p.stdout and _file_rows(plain) != _file_rows(one)
    # BP_MS only, and not with the layered schedule
    other = str(tmp_path / "other.txt")
    p = subprocess.run(head + [other] + tail[:5] + flags, stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode != 0 and "--ms-bits" in p.stdout
    p = subprocess.run(head + [other] + tail + flags + ["--ms-schedule", "layered"], stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode != 0 and "--ms-bits" in p.stdout and "layered" in p.stdout
    p = subprocess.run(head + [other] + tail + ["--ms-bits", "9"], stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode != 0 and "--ms-bits" in p.stdout
    assert not os.path.exists(other)
