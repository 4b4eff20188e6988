"""Caller-supplied LLRs at the edges (tests/edge_llrs.py) without a GPU: the oracle's deterministic arithmetic (detmath.h, the
kernels' header) against its libm arithmetic (the reference's) on whole decodes, and the numpy mirrors against the oracle on
the same frames, so that both can serve as yardsticks for the kernels in test_gpu_edge_llrs.py.

Class P: both modes agree on iters and hard, on llr_out within DESIGN.md's 1e-5 (bit for bit for min-sum, which has no
transcendental), and the det-mode output holds no NaN.  Class T (0 < L < 2^-53): the same verdicts — the ratio form refuses
such a frame (detmath.h, dm_ratio_llr_refused) and the E-domain check node hands a node with such an input to the term-by-term
box-plus (dm_llr_tiny).  Class N: what the oracle does is recorded, nothing about it is promised."""
import math
import zlib

import numpy as np
import pytest

import edge_llrs as el
import orc
from layered_minsum_ref import LayeredMinSumMirror
from minsum_ref import MinSumMirror
from quantized_minsum_ref import quantize
from test_gpu_random_codes import FUSED_CASES, make_fused_code

ITERS = 20
RUNS = [(ms, early) for ms in (False, True) for early in (True, False)]


def _fused_small(directory):
    name, cn_spec, vn_degs, punct, short = FUSED_CASES[0]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return make_fused_code(str(directory / f"{name}.txt"), rng, cn_spec, vn_degs, punct, short)


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    """name -> (code, base frames that converge and that fail, class-P frames)"""
    out = {}
    for name, path, x in (("h_txt", orc.H_TXT, -4.5), ("fused_small", _fused_small(tmp_path_factory.mktemp("edge")), 3.0)):
        code = orc.Code(path)
        r = code.run_frames("AWGN", x, seed=7, count=8, iters=ITERS, math=orc.MATH_DET)
        assert (r["bit_errors"] == 0).any() and (r["bit_errors"] > 0).any(), name
        out[name] = (code, r["llr_in"], el.class_p(code, r["llr_in"]))
    return out


def _agree(code, frames, ms, early):
    det = el.oracle_decode(code, frames, ms, early, ITERS, orc.MATH_DET)
    ref = el.oracle_decode(code, frames, ms, early, ITERS, orc.MATH_LIBM)
    bad = [f.name for i, f in enumerate(frames) if det["iters"][i] != ref["iters"][i] or not np.array_equal(det["hard"][i], ref["hard"][i])]
    return det, ref, bad


def test_builder(codes):
    """Every value sits on a column of every degree class, the structural rule calls no class-P frame NaN-making, and the
    two doubles around ln 2^k are neighbours that enclose it."""
    for lo, hi, k in (el.HANDOVER + (220,), el.BOX + (240,)):
        assert hi == math.nextafter(lo, math.inf) and math.exp(lo) <= 2.0 ** k <= math.exp(hi) and abs(lo - k * math.log(2)) < 1e-12
    assert el.LIMIT[0] < 166.0 < el.LIMIT[2]
    for name, (code, base, frames) in codes.items():
        g = el.Graph(code)
        assert {"degree2", "degree3up", "leaf", "widest"} == set(g.classes), name
        assert len({f.name for f in frames}) == len(frames)
        assert not any(el.makes_nan(g, f.llr) for f in frames)
        for v in el.ALL_VALUES:
            hit = np.zeros(code.nc, bool)
            for f in frames:
                hit |= (f.llr.view(np.uint64) == np.float64(v).view(np.uint64)) & f.name.startswith(("eight", "one_"))
            assert all(hit[cols].any() for cols in g.classes.values()), (name, v)
        assert sum(np.isinf(f.llr).any() for f in frames) == 2


@pytest.mark.parametrize("ms,early", RUNS, ids=lambda v: str(int(v)))
@pytest.mark.parametrize("name", ["h_txt", "fused_small"])
def test_class_p_det_mode_equals_libm_mode(codes, name, ms, early):
    code, base, frames = codes[name]
    det, ref, bad = _agree(code, frames, ms, early)
    assert not np.isnan(det["llr_out"]).any(), "a class-P frame makes a NaN: a mistake in the builder"
    assert not np.isnan(ref["llr_out"]).any()
    assert not bad, bad
    if ms:
        assert np.array_equal(det["llr_out"].view(np.uint64), ref["llr_out"].view(np.uint64))
    else:
        a, b = det["llr_out"], ref["llr_out"]
        fin = np.isfinite(a) & np.isfinite(b)
        assert np.array_equal(a[~fin], b[~fin])  # (infinities: equal as values)
        assert (np.abs(a[fin] - b[fin]) <= 1e-5).all(), float(np.abs(a[fin] - b[fin]).max())  # DESIGN.md's tier 2
    assert (det["iters"] < ITERS).any() or not early


@pytest.mark.parametrize("name", ["h_txt", "fused_small"])
def test_class_t_det_mode_equals_libm_mode(codes, name):
    """Tiny positive inputs: e^L rounds to exactly 1 and the ratio form would decide the tie as 1; it refuses such frames, the
    LLR-domain form decides `L <= 0` as the reference does."""
    code, base, _ = codes[name]
    frames = el.class_t(code, base)
    assert all(((f.llr > 0) & (f.llr < 2.0 ** -53)).any() for f in frames)
    for ms, early in RUNS:
        det, ref, bad = _agree(code, frames, ms, early)
        assert not bad, (ms, early, bad)
        assert not np.isnan(det["llr_out"]).any()
    det = el.oracle_decode(code, frames[:2], False, True, ITERS, orc.MATH_DET)
    assert not det["iters"].any() and not det["hard"].any()  # all inputs positive: the all-zero word at once


@pytest.mark.parametrize("name", ["h_txt", "fused_small"])
def test_mirrors_against_their_yardsticks(codes, name):
    """MinSumMirror at (1, 0) is the oracle's min-sum on class P (it finds second minima by masking with np.inf: an infinite
    input must not confuse it); the layered mirror gives the same bits whatever the order within a step; the quantized
    mirror's quantizer is item 1 of ldpc_hip_set_min_sum_quantization, computed value by value."""
    code, base, frames = codes[name]
    llr = el.stack(frames)
    mir = MinSumMirror(code)
    for early in (True, False):
        o = el.oracle_decode(code, frames, True, early, ITERS, orc.MATH_DET)
        for idx, short in el.batches(frames, early, size=len(frames)):
            m = mir.decode(llr[idx], 1.0, 0.0, early_term=early, iterations=el.SHORT_ITERATIONS if short else ITERS)
            for k in ("iters", "hard", "bit_errors"):
                assert np.array_equal(m[k], o[k][idx]), (early, k)
            assert np.array_equal(m["llr_out"].view(np.uint64), o["llr_out"][idx].view(np.uint64)), early
    lay = LayeredMinSumMirror(code)
    some = llr[::7]
    for early in (True, False):
        a = lay.decode(some, 0.8125, 0.25, early_term=early, iterations=6)
        b = lay.decode(some, 0.8125, 0.25, early_term=early, iterations=6, row_order="reversed")
        for k in ("iters", "hard", "bit_errors"):
            assert np.array_equal(a[k], b[k]), (early, k)
        assert np.array_equal(a["llr_out"].view(np.uint64), b["llr_out"].view(np.uint64)), early
    for bits, step in ((6, 0.25), (8, 0.3), (2, 2.0)):
        qmax, inv = float((1 << (bits - 1)) - 1), 1.0 / step
        got = quantize(llr, bits, step)
        for v in np.unique(llr.view(np.uint64)).view(np.float64):
            x = v * inv
            want = 0 if x != x else int(max(-qmax, min(qmax, x if math.isinf(x) else float(round(x)))))
            assert (got[llr.view(np.uint64) == np.float64(v).view(np.uint64)] == want).all(), (bits, step, v)


def test_class_n_what_the_oracle_does(codes):
    """Recorded, not promised: every class-N frame does make NaNs in the reference's arithmetic in at least one decoding, and
    the iteration count stays within the limit."""
    code, base, _ = codes["h_txt"]
    frames = el.class_n(code, base)
    made = np.zeros(len(frames), bool)
    for ms, early in RUNS:
        for math_mode, tag in ((orc.MATH_LIBM, "libm"), (orc.MATH_DET, "det")):
            r = el.oracle_decode(code, frames, ms, early, ITERS, math_mode)
            nans = np.isnan(r["llr_out"]).sum(axis=1)
            made |= nans > 0
            assert (r["iters"] <= ITERS).all() and (r["hard"] <= 1).all()
            print(f"class N, h.txt, {'BP_MS' if ms else 'BP'}, early={int(early)}, {tag}: NaN outputs "
                  + ", ".join(f"{f.name} {n}" for f, n in zip(frames, nans)))
    assert made.all(), [f.name for f, m in zip(frames, made) if not m]
