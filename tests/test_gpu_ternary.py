"""Ternary min-sum on the GPU (include/ldpc_amd.h, ldpc_hip_set_min_sum_ternary; kernels_ternary.hip) against the numpy mirror
(tests/ternary_ref.py), bit for bit: iters, hard, bit_errors, and llr_out as uint64.  Then the fused channel paths, the
paths that must not move, the simulation loop and the CLI."""
import importlib.util
import os

import numpy as np
import pytest

import orc
from minsum_common import (VARIANTS, WANT, check_fused_channel, check_no_iteration, check_nothing_else_moves, check_simulation_and_cli,
                           check_split_batch, dumped, same)
from ternary_ref import CASES, TernaryMirror, flipped_llrs
from test_gpu_quantized_min_sum import wide_irregular_code

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 70  # frames of the mirror's inputs the GPU decodes: two full groups of 32 and a short one


def _off(d):
    d.set_min_sum_ternary(0)


def _ternary(d, llr, w, early=True, iters=50, codeword=None):
    d.set_min_sum_ternary(w)
    return d.decode_batch(llr, early_term=early, iterations=iters, decoding="BP_MS", want=WANT)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """The two regular codes of the host tests with the first 70 of their frames, a decoder each, and the mirror's results
    (computed once): key -> dict(d, mir, llr, w, path, ref{(early, iters): results})."""
    import libldpc_amd
    # (the generator by its path in this tree, not by whatever the module search path holds under that name)
    spec = importlib.util.spec_from_file_location("gen_regular_code", os.path.join(ROOT, "tools", "gen_regular_code.py"))
    gen_regular_code = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen_regular_code)
    assert os.path.realpath(libldpc_amd.LIB_PATH) == os.path.realpath(os.path.join(ROOT, "libldpc_amd", "libldpc.so"))
    out = {}
    for key, (nc, dv, dc, cseed, w, eps, n, seed) in CASES.items():
        path = tmp_path_factory.mktemp("codes") / f"{key}.txt"
        path.write_text(gen_regular_code.generate(nc, dv, dc, cseed))
        mir = TernaryMirror(orc.Code(str(path)))
        llr = flipped_llrs(nc, eps, n, seed)[:N]
        ref = {(e, i): mir.decode(llr, w, early_term=e, iterations=i) for e, i in ((True, 50), (False, 20))}
        out[key] = {"d": libldpc_amd.HipDecoder(str(path)), "mir": mir, "llr": llr, "w": w, "path": str(path), "ref": ref}
    return out


@pytest.mark.parametrize("key", sorted(CASES))
def test_regular_codes(cases, key):
    """Early termination at 50 iterations and none at 20; converged and failed frames both occur among the 70."""
    c = cases[key]
    for (early, iters), m in c["ref"].items():
        same(_ternary(c["d"], c["llr"], c["w"], early, iters), m, (key, early))
    m = c["ref"][(True, 50)]
    assert ((m["iters"] < 50) & (m["bit_errors"] == 0)).any() and (m["bit_errors"] > 0).any()
    assert len(set(m["iters"].tolist())) > 3  # frames of one group stop at different iterations
    _off(c["d"])


def test_batch_shapes(cases):
    """Batches of 1, 31, 32, 33 and 70 frames (a short group, a full one, one frame into the next), a batch split at a frame
    that is no multiple of 32, and no iteration at all."""
    c = cases["r36"]
    d, llr, w, m = c["d"], c["llr"], c["w"], c["ref"][(True, 50)]
    for n in (1, 31, 32, 33, N):
        same(_ternary(d, llr[:n], w), m, n, slice(0, n))
    same(_ternary(d, llr[37:38], w), m, "frame 37 alone", slice(37, 38))
    one = check_split_batch(lambda part: _ternary(d, part, w), llr, cut=20)
    same(one, m, "whole batch")
    for early in (True, False):
        check_no_iteration(_ternary(d, llr[:33], w, early, 0))
    _off(d)


def test_corner_inputs(cases):
    """Item 1: +0.0, -0.0 and NaN are r = 0, the infinities and 99999.9 are +-1, like every other nonzero value."""
    c = cases["r36"]
    llr = c["llr"][:40].copy()
    rng = np.random.default_rng(2)
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 99999.9, -99999.9, 5e-324, -1e-300])
    where = rng.random(llr.shape) < 0.1
    llr[where] = rng.choice(vals, size=int(where.sum()))
    for v in vals:
        assert (np.isnan(llr).any() if np.isnan(v) else ((llr == v) & (np.signbit(llr) == np.signbit(v))).any())
    for early, iters in ((True, 30), (False, 8)):
        same(_ternary(c["d"], llr, 1, early, iters), c["mir"].decode(llr, 1, early_term=early, iterations=iters), ("corner", early))
    _off(c["d"])


def test_weight_7(cases):
    c = cases["r48"]
    for early, iters in ((True, 30), (False, 6)):
        m = c["mir"].decode(c["llr"], 7, early_term=early, iterations=iters)
        same(_ternary(c["d"], c["llr"], 7, early, iters), m, ("w7", early))
    assert np.abs(m["llr_out"]).max() > 7
    _off(c["d"])


def test_wide_irregular_code(tmp_path):
    """Check degrees 2..40, a column of degree 22 (six planes at weight 3), leaves, punctured and shortened columns; AWGN
    LLRs, so the staged channel route."""
    import libldpc_amd
    path = wide_irregular_code(str(tmp_path / "wide.txt"))
    code = orc.Code(path)
    d = libldpc_amd.HipDecoder(path)
    assert 0 < d.ternary_lds_bytes() <= 160 * 1024
    llr = dumped(d, _off, "AWGN", 2.0, 33)
    assert (np.abs(llr) > 90000).any() and (llr == 0).any()  # shortened columns saturate, punctured ones are zero
    mir = TernaryMirror(code)
    for n in (16, 33):
        for early, iters in ((True, 15), (False, 15)):
            m = mir.decode(llr[:n], 3, early_term=early, iterations=iters)
            same(_ternary(d, llr[:n], 3, early, iters), m, ("wide", n, early))


def test_h_txt():
    """Degree-15 columns (six planes at weight 2), leaves, punctured columns; at -4 dB nothing converges."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    llr = dumped(d, _off, "AWGN", -4.0, 40)
    m = TernaryMirror(orc.Code(orc.H_TXT)).decode(llr, 2, iterations=10)
    same(_ternary(d, llr, 2, True, 10), m, "h.txt")
    assert (m["iters"] == 10).all() and (m["bit_errors"] > 0).all()


def test_fused_channel_equals_decode_of_its_llrs(cases):
    """stream_decode with the mode on == decode_batch of the same frames' dumped llr_in: AWGN and BSC, the reference stream
    and the counter-based noise, early termination on and off; and the BSC's direct route (no dump wanted) equals the
    staged one."""
    c = cases["r36"]
    d = c["d"]
    d.set_min_sum_ternary(1)

    def each(r, noise, ch, x, early):
        assert r["iters"].max() > 0 and (r["iters"] < 30).any() == early
        for want in (("iters", "bit_errors"), WANT):
            d.stream_begin(ch, 6, x)
            q = d.stream_decode(N, early_term=early, iterations=30, decoding="BP_MS", want=want)
            for k in want:
                assert np.array_equal(q[k], r[k]), (noise, ch, early, k)

    r = check_fused_channel(d, points=(("AWGN", 4.5), ("BSC", 0.04)), n=N, each=each)
    # ... and it is the ternary decoder that ran: the mirror on the last frames
    same({k: r[k] for k in WANT}, c["mir"].decode(r["llr_in"], 1, early_term=False, iterations=30), "mirror")
    _off(d)


def test_correction_has_no_effect(cases):
    c = cases["r36"]
    c["d"].set_min_sum_correction(0.75, 0.5)
    same(_ternary(c["d"], c["llr"], c["w"]), c["ref"][(True, 50)], "corrected")
    c["d"].set_min_sum_correction()
    _off(c["d"])


def test_nothing_else_moves():
    """With the mode on, BP (AWGN, BSC) and BEC outputs equal a fresh context's; with it off again, BP_MS — flooding, layered
    and quantized — equals a fresh context's."""
    check_nothing_else_moves(VARIANTS["ternary"])


def test_simulation_and_cli(cases, tmp_path):
    """simulate() with the mode on and counter noise gives the totals of a host fold of stream_decode over the same frames;
    the CLI with --ms-ternary 1 --noise counter writes the same result file as the Python run, alone and as two ranks over
    shared memory; --ms-ternary is refused with BP, --ms-bits, --ms-schedule layered and --ms-scale."""
    c = cases["r36"]
    check_simulation_and_cli(VARIANTS["ternary"], c["d"], tmp_path, c["path"])
    c["d"].set_noise("reference")
    _off(c["d"])
