"""Fixed-point layered min-sum on the GPU (include/ldpc_amd.h, ldpc_hip_set_min_sum_layered_fixed;
kernels_layered_fixed.hip) against the numpy mirror (tests/layered_fixed_minsum_ref.py), bit for bit: iters, hard, bit_errors,
and llr_out as uint64.  Then the fused channel paths, the paths that must not move, the simulation loop and the CLI."""
import numpy as np
import pytest

import orc
from layered_fixed_minsum_ref import LayeredFixedMinSumMirror
from minsum_common import (VARIANTS, WANT, against_mirror, check_fused_channel, check_no_iteration, check_nothing_else_moves,
                           check_simulation_and_cli, check_split_batch, dumped, same)
from test_gpu_layered_min_sum import irregular_code

pytestmark = pytest.mark.gpu
# (msg_bits, app_bits, step, scale, offset)
H_SETTINGS = [(6, 8, 0.25, 1.0, 0.0), (6, 8, 0.25, 0.8125, 0.0), (6, 6, 0.25, 0.8125, 0.0), (5, 7, 0.5, 0.75, 0.5),
              (4, 6, 1.0, 1.0, 0.0), (2, 2, 2.0, 1.0, 0.0), (8, 16, 0.0625, 0.8125, 0.1)]


def _off(d):
    d.set_min_sum_layered_fixed(0)


def _fixed(d, llr, setting, early, iters):
    q, p, step, s, o = setting
    d.set_min_sum_layered_fixed(q, p, step)
    d.set_min_sum_correction(s, o)
    return d.decode_batch(llr, early_term=early, iterations=iters, decoding="BP_MS", want=WANT)


def _against_mirror(d, mir, llr, settings, runs):
    """Every (setting, (early, iterations)) against the mirror; returns the mirror's results."""
    out = against_mirror(settings, runs, lambda st, early, iters: _fixed(d, llr, st, early, iters),
                         lambda st, early, iters: mir.decode(llr, *st, early_term=early, iterations=iters))
    d.set_min_sum_correction()
    d.set_min_sum_layered_fixed(0)
    return out


@pytest.fixture(scope="module")
def h_txt():
    """h.txt, 48 frames of the reference stream at -5.0 dB, and a cache of the mirror's results on them."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    code = orc.Code(orc.H_TXT)
    n_steps, step_of = code.layer_steps()
    counts = set(np.bincount(step_of, minlength=n_steps).tolist())
    assert n_steps == 24 and {16, 32, 48, 64} >= counts and len(counts) > 1 and code.num_puncture == 128
    return {"d": d, "llr": dumped(d, _off, "AWGN", -5.0, 48), "mir": LayeredFixedMinSumMirror(code), "ref": {}}


def _h_ref(h, st, early, iters):
    key = st + (early, iters)
    if key not in h["ref"]:
        h["ref"][key] = h["mir"].decode(h["llr"], *st, early_term=early, iterations=iters)
    return h["ref"][key]


@pytest.mark.parametrize("setting", H_SETTINGS, ids=lambda s: "q%d_p%d_step%g_a%g_b%g" % s)
def test_h_txt(h_txt, setting):
    """Seven settings, each with early termination at 50 iterations and without at 20."""
    d, llr = h_txt["d"], h_txt["llr"]
    for early, iters in ((True, 50), (False, 20)):
        m = _h_ref(h_txt, setting, early, iters)
        print(setting, early, "clamp share", m["clamp_share"], "converged", int(((m["iters"] < iters) & (m["bit_errors"] == 0)).sum()),
              "failed", int((m["bit_errors"] > 0).sum()))
        same(_fixed(d, llr, setting, early, iters), m, (setting, early))
    m = _h_ref(h_txt, setting, True, 50)
    if setting == (6, 8, 0.25, 1.0, 0.0):
        converged, failed = (m["iters"] < 50) & (m["bit_errors"] == 0), m["bit_errors"] > 0
        assert converged.any() and failed.any(), (int(converged.sum()), int(failed.sum()))
    if setting == (6, 6, 0.25, 0.8125, 0.0):
        assert m["clamp_share"] > 0
    d.set_min_sum_correction()
    d.set_min_sum_layered_fixed(0)


def test_h_txt_batches(h_txt):
    """Batches of n = 1 and 7, one batch split in two, and no iteration at all."""
    d, llr = h_txt["d"], h_txt["llr"]
    st = (6, 8, 0.25, 1.0, 0.0)
    m = _h_ref(h_txt, st, True, 50)
    for n in (1, 7):
        same(_fixed(d, llr[:n], st, True, 50), m, n, slice(0, n))
    st2 = (5, 7, 0.5, 0.75, 0.5)
    one = check_split_batch(lambda part: _fixed(d, part, st2, True, 50), llr)
    same(one, _h_ref(h_txt, st2, True, 50), "whole batch")
    for early in (True, False):
        check_no_iteration(_fixed(d, llr[:3], st, early, 0))
    d.set_min_sum_correction()
    d.set_min_sum_layered_fixed(0)


def test_8k_code(h8k_file):
    """The 8k (3,6) code: 65 steps of degree 6, two frames per CU."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(h8k_file)
    code = orc.Code(h8k_file)
    assert code.layer_steps()[0] == 65 and 0 < 2 * d.layered_fixed_lds_bytes() <= 160 * 1024
    llr = dumped(d, _off, "AWGN", 1.4, 8)
    second = (5, 6, 0.5, 0.8125, 0.0)
    ms = _against_mirror(d, LayeredFixedMinSumMirror(code), llr, [(6, 7, 0.25, 1.0, 0.0), second], [(True, 25), (False, 25)])
    m = ms[second + (True,)]
    print("converged", int(((m["iters"] < 25) & (m["bit_errors"] == 0)).sum()), "clamp share", m["clamp_share"])
    assert ((m["iters"] < 25) & (m["bit_errors"] == 0)).any() and m["clamp_share"] > 0


def test_irregular_code(tmp_path):
    """237 x 125, every check degree 2..8, steps down to one lane, odd counts, nc % 64 != 0, punctured and shortened columns."""
    import libldpc_amd
    path = irregular_code(str(tmp_path / "irregular.txt"))
    code = orc.Code(path)
    assert (code.nc, code.mc, code.num_puncture, code.num_shorten) == (237, 125, 3, 2) and code.nc % 64 != 0
    assert set(np.bincount(code.edge_row).tolist()) == set(range(2, 9))
    n_steps, step_of = code.layer_steps()
    counts = np.bincount(step_of, minlength=n_steps)
    assert counts.min() == 1 and (counts % 2 == 1).any() and counts.max() < 64
    d = libldpc_amd.HipDecoder(path)
    llr = dumped(d, _off, "AWGN", 2.0, 16)
    assert (np.abs(llr) > 90000).any() and (llr == 0).any()  # shortened columns saturate, punctured ones are zero
    settings = [(6, 8, 0.25, 1.0, 0.0), (5, 6, 0.5, 0.8125, 0.25), (4, 5, 1.0, 1.0, 0.0)]
    ms = _against_mirror(d, LayeredFixedMinSumMirror(code), llr, settings, [(True, 15), (False, 15)])
    for key, m in ms.items():
        print(key, "clamp share", m["clamp_share"])
        assert m["clamp_share"] > 0, key
    m = ms[settings[0] + (True,)]
    converged, failed = (m["iters"] < 15) & (m["bit_errors"] == 0), m["bit_errors"] > 0
    assert converged.any() and failed.any(), (int(converged.sum()), int(failed.sum()))


def test_fused_channel_equals_decode_of_its_llrs():
    """stream_decode with the mode on == decode_batch of the same frames' dumped llr_in: AWGN and BSC, the reference stream
    and the counter-based noise, early termination and not; then once with a generator matrix, so that bit_errors is taken
    against a non-zero codeword."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    d.set_min_sum_layered_fixed(5, 7, 0.5)
    d.set_min_sum_correction(0.8125, 0.25)
    r = check_fused_channel(d)
    # ... and it is the fixed-point layered decoder that ran: the mirror on the last frames
    mir = LayeredFixedMinSumMirror(orc.Code(orc.H_TXT))
    m = mir.decode(r["llr_in"][:8], 5, 7, 0.5, 0.8125, 0.25, early_term=False, iterations=30)
    same({k: r[k][:8] for k in WANT}, m, "mirror")
    # transmitted codewords that are not all zero
    g = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    g.set_min_sum_layered_fixed(6, 8, 0.25)
    g.stream_begin("AWGN", 9, -4.5)
    r = g.stream_decode(64, early_term=True, iterations=30, decoding="BP_MS", want=WANT + ("llr_in", "codeword"))
    assert r["codeword"].any()
    m = mir.decode(r["llr_in"], 6, 8, 0.25, early_term=True, iterations=30, codeword=r["codeword"])
    same({k: r[k] for k in WANT}, m, "codewords")
    assert (m["bit_errors"] == 0).any() and (m["bit_errors"] > 0).any()


def test_nothing_else_moves():
    """With the mode on, BP (AWGN, BSC) and BEC outputs equal a fresh context's; with it off again, BP_MS — flooding,
    layered binary64 and quantized — equals a fresh context's."""
    check_nothing_else_moves(VARIANTS["layered-fixed"])


def test_simulation_and_cli(tmp_path):
    """simulate() with the mode and counter noise gives the totals of a host fold of stream_decode over the same frames; the
    CLI with --ms-layered-fixed 6,8,0.25 --noise counter writes the same result file as the Python run, alone and as two
    ranks over shared memory; the flag is refused with BP, with each of the other three variants' flags and with 6,5,0.25."""
    import libldpc_amd
    check_simulation_and_cli(VARIANTS["layered-fixed"], libldpc_amd.HipDecoder(orc.H_TXT), tmp_path)
