"""Quantized min-sum on the GPU (include/ldpc_amd.h, ldpc_hip_set_min_sum_quantization; kernels_qms.hip) against the numpy
mirror (tests/quantized_minsum_ref.py), bit for bit: iters, hard, bit_errors, and llr_out as uint64.  Then the fused channel
paths, the paths that must not move, the simulation loop and the CLI."""
import numpy as np
import pytest

import orc
from minsum_common import (VARIANTS, WANT, against_mirror, check_fused_channel, check_no_iteration, check_nothing_else_moves,
                           check_simulation_and_cli, check_split_batch, dumped, same)
from quantized_minsum_ref import QuantizedMinSumMirror, quantize
from test_gpu_random_codes import make_code_by_degrees

pytestmark = pytest.mark.gpu
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
    r = check_fused_channel(d)
    # ... and it is the quantized decoder that ran: the mirror on the last frames
    m = QuantizedMinSumMirror(orc.Code(orc.H_TXT)).decode(r["llr_in"][:8], 5, 0.5, 0.8125, 0.25, early_term=False, iterations=30)
    same({k: r[k][:8] for k in WANT}, m, "mirror")


def test_nothing_else_moves():
    """With quantization on, BP (AWGN, BSC) and BEC outputs equal a fresh context's; with it off again, BP_MS — flooding,
    and then layered — equals a fresh context's."""
    check_nothing_else_moves(VARIANTS["quantized"])


def test_simulation_and_cli(tmp_path):
    """simulate() with quantization and counter noise gives the totals of a host fold of stream_decode over the same frames;
    the CLI with --ms-bits 6 --ms-step 0.25 --noise counter writes the same result file as the Python run, alone and as two
    ranks over shared memory; --ms-bits is refused with BP and with --ms-schedule layered."""
    import libldpc_amd
    check_simulation_and_cli(VARIANTS["quantized"], libldpc_amd.HipDecoder(orc.H_TXT), tmp_path)
