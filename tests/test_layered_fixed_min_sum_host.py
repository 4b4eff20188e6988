"""Fixed-point layered min-sum (include/ldpc_amd.h, ldpc_hip_set_min_sum_layered_fixed) without a GPU: the setter's validity
check, the codes it takes and how the four min-sum variants exclude each other, the launch stages and decoder it reports, the
LDS figure and the kernel's resources, and the numpy mirror (tests/layered_fixed_minsum_ref.py) by itself — its own
properties and what the mode is for: how many total (APP) bits a code needs."""
import itertools

import numpy as np
import pytest

import orc
from layered_fixed_minsum_ref import LayeredFixedMinSumMirror
from minsum_common import EXCLUSIVE, VARIANTS, check_decode_stages, write
from quantized_minsum_ref import QuantizedMinSumMirror

NAME = "ldpc_hip_set_min_sum_layered_fixed"


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


def test_setter_accepts_and_rejects(lib):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    assert d.min_sum_layered_fixed == (0, 8, 1.0)  # off by default
    for q in range(2, 9):
        for p in (q, q + 3, 16):
            d.set_min_sum_layered_fixed(q, p, 0.25 * q)
            assert d.min_sum_layered_fixed == (q, p, 0.25 * q)
    d.set_min_sum_layered_fixed(6, 8, 0.25)
    bad = [(1, 8, 0.25), (9, 12, 0.25), (-1, 8, 0.25), (6, 5, 0.25), (6, 17, 0.25), (8, 7, 0.25), (6, 0, 0.25)]
    bad += [(5, 7, s) for s in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 2.0 ** 21)]
    for q, p, step in bad:
        with pytest.raises(RuntimeError, match=NAME):
            d.set_min_sum_layered_fixed(q, p, step)
        assert lib.ldpc_hip_set_min_sum_layered_fixed(d.ctx, q, p, step) == -1 and NAME.encode() in lib.ldpc_hip_last_error()
        assert d.min_sum_layered_fixed == (6, 8, 0.25), (q, p, step)  # unchanged
    # the edges of the ranges
    d.set_min_sum_layered_fixed(2, 2, 2.0 ** -20)
    d.set_min_sum_layered_fixed(8, 16, 2.0 ** 20)
    assert d.min_sum_layered_fixed == (8, 16, 2.0 ** 20)
    d.set_min_sum_layered_fixed(0, -5, float("nan"))  # off: the other arguments are ignored
    assert d.min_sum_layered_fixed[0] == 0
    d.set_min_sum_layered_fixed(4, 6, 1.0)
    d.set_min_sum_layered_fixed()
    assert d.min_sum_layered_fixed[0] == 0
    # the getter's pointers may be null
    assert lib.ldpc_hip_min_sum_layered_fixed(d.ctx, None, None, None) == 0


def _lds_bytes(code):
    """The formula beside ldpc_hip_layered_fixed_lds_bytes, from the oracle's restatement of the layered plan."""
    n, step_of = code.layer_steps()
    slots = int(((np.bincount(step_of, minlength=n) + 1) // 2 * 2).sum())
    return (max(8 * code.nc, (2 * code.nc + 3) // 4 * 4 + 4 * slots) + 128 + 15) // 16 * 16


def test_codes_and_lds(lib, tmp_path, h8k_file):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    h = d.layered_fixed_lds_bytes()
    assert h == _lds_bytes(orc.Code(orc.H_TXT)) <= 9600 and 17 * h <= 160 * 1024  # 17 frames per CU
    d8 = libldpc_amd.HipDecoder(h8k_file)
    assert d8.layered_fixed_lds_bytes() == _lds_bytes(orc.Code(h8k_file)) <= 80 * 1024  # two frames per CU
    d8.set_min_sum_layered_fixed(6, 7, 0.25)
    assert d8.min_sum_layered_fixed == (6, 7, 0.25)
    # a code whose records, not its channel values, set the figure: 4 columns, 8 check nodes of degree 2
    small = write(tmp_path / "small.txt", [[0, 1], [1, 2], [2, 3], [3, 0], [0, 2], [1, 3], [0, 1], [2, 3]])
    ds = libldpc_amd.HipDecoder(small)
    assert ds.layered_fixed_lds_bytes() == _lds_bytes(orc.Code(small)) > 8 * 4 + 128
    ds.set_min_sum_layered_fixed(6, 8, 0.25)
    # codes outside what the layered plan takes
    cases = {
        "isolated_column": [[0, 1, 2], [2, 3, 5], [5, 6, 0], [1, 3, 6]],  # column 4 has no edge
        "degree9_row": [[0, 1, 2], [2, 3, 4], [4, 5, 0], [1, 3, 5]] + [list(range(9))],
    }
    for name, rows in cases.items():
        dd = libldpc_amd.HipDecoder(write(tmp_path / f"{name}.txt", rows))
        assert dd.layered_fixed_lds_bytes() == -1, name
        with pytest.raises(RuntimeError, match=NAME):
            dd.set_min_sum_layered_fixed(6, 8, 0.25)
        assert lib.ldpc_hip_set_min_sum_layered_fixed(dd.ctx, 6, 8, 0.25) == -1 and NAME.encode() in lib.ldpc_hip_last_error(), name
        assert dd.min_sum_layered_fixed[0] == 0, name
        assert dd.decoder_choice(decoding="BP_MS") == "resident", name
    # beyond 160 KB of LDS: 30 000 columns of channel values alone are 240 000 bytes
    nc = 30000
    rows = [[c, (c + 1) % nc] for c in range(0, nc, 2)] + [[c, (c + 3) % nc] for c in range(1, nc, 2)]
    big = libldpc_amd.HipDecoder(write(tmp_path / "big.txt", rows))
    assert big.layered_fixed_lds_bytes() == -1
    with pytest.raises(RuntimeError, match="LDS"):
        big.set_min_sum_layered_fixed(6, 8, 0.25)
    assert NAME.encode() in lib.ldpc_hip_last_error() and big.min_sum_layered_fixed[0] == 0


def _state(d):
    return d.min_sum_schedule, d.min_sum_quantization[0], d.min_sum_ternary, d.min_sum_layered_fixed[0]


OFF = ("flooding", 0, 0, 0)
PAIRS = list(itertools.permutations(EXCLUSIVE, 2))


# (the ids this test had when it walked the pairs with the fixed-point mode alone: that mode is "fixed" in them)
@pytest.mark.parametrize("first,second", PAIRS, ids=["-".join(p).replace("layered-fixed", "fixed") for p in PAIRS])
def test_excludes_the_other_variants(lib, first, second):
    """Every ordered pair of the four variants (layered, quantized, ternary, fixed-point layered): with the first in force,
    switching the second on returns -1 naming that setter and changes nothing; switching the first off lets the second in,
    and then the first is refused."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    v1, v2 = VARIANTS[first], VARIANTS[second]
    v1.on(d)
    before = _state(d)
    assert before != OFF and v1.state(d) and not v2.state(d) and d.decoder_choice(decoding="BP_MS") == v1.choice
    with pytest.raises(RuntimeError, match=v2.setter):
        v2.on(d)
    assert v2.setter.encode() in lib.ldpc_hip_last_error()
    assert _state(d) == before and v1.state(d) and not v2.state(d) and d.decoder_choice(decoding="BP_MS") == v1.choice
    v2.off(d)  # switching off what is off is always taken
    v1.on(d)   # and the setting in force may be set again
    assert _state(d) == before and v1.state(d)
    v1.off(d)
    assert _state(d) == OFF and d.decoder_choice(decoding="BP_MS") == "resident"
    v2.on(d)
    assert _state(d) != before and _state(d) != OFF
    assert v2.state(d) and not v1.state(d) and d.decoder_choice(decoding="BP_MS") == v2.choice
    with pytest.raises(RuntimeError, match=v1.setter):
        v1.on(d)
    assert v1.setter.encode() in lib.ldpc_hip_last_error()


def test_choice_stages_and_plan(lib, h8k_file):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    before = {(e, i): d.decoder_choice(e, i, "BP") for e in (True, False) for i in (50, 0)}
    assert lib.ldpc_hip_selftest_layer_plan(d.ctx, None) == 0  # lazy: nothing has asked yet
    d.set_min_sum_layered_fixed(6, 8, 0.25)
    for (e, i), c in before.items():
        assert d.decoder_choice(e, i, "BP_MS") == "layered-fixed-min-sum" and d.decoder_choice(e, i, "BP") == c
    assert libldpc_amd.HipDecoder.DECODERS.index("layered-fixed-min-sum") == 7
    d.set_fast_mode(1)  # sum-product's switch: min-sum ignores it
    assert d.decoder_choice(decoding="BP_MS") == "layered-fixed-min-sum" and d.decoder_choice(decoding="BP") == "fast32"
    d.set_fast_mode(0)
    # the LDS figure, the setter and the layered schedule's own figure share one plan
    assert d.layered_fixed_lds_bytes() > 0 and d.layered_min_sum_lds_bytes() > 0
    d.set_min_sum_layered_fixed(0)
    d.set_min_sum_schedule("layered")
    d.set_min_sum_schedule("flooding")
    d.set_min_sum_layered_fixed(5, 7, 0.5)
    assert lib.ldpc_hip_selftest_layer_plan(d.ctx, None) == 1
    d.set_min_sum_layered_fixed(0)
    assert d.decoder_choice(decoding="BP_MS") == "resident"
    for path in (orc.H_TXT, h8k_file):
        check_decode_stages(libldpc_amd.HipDecoder(path), lambda x: x.set_min_sum_layered_fixed(6, 8, 0.25),
                            lambda x: x.set_min_sum_layered_fixed(0))


def test_kernel_uses_no_scratch(lib):
    from libldpc_amd import build
    res = build.kernel_resources("kernels_layered_fixed.hip")
    assert res and len(res) == 2  # WANT_LLR or not
    for name, r in res.items():
        assert "decode_layered_fixed_kernel" in name
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)


def _awgn_llrs(code, snr_db, n, seed):
    """All-zero codewords over AWGN with numpy's normals: LLR 2 y / sigma^2, punctured columns 0."""
    rng = np.random.default_rng(seed)
    sigma2 = 10.0 ** (-snr_db / 10.0)
    llr = np.zeros((n, code.nc))
    llr[:, code.bit_pos] = 2.0 * (1.0 + np.sqrt(sigma2) * rng.standard_normal((n, code.nct))) / sigma2
    return llr


KEYS = ("iters", "hard", "bit_errors", "llr_out")


@pytest.fixture(scope="module")
def h_case():
    code = orc.Code(orc.H_TXT)
    return code, LayeredFixedMinSumMirror(code), _awgn_llrs(code, -3.5, 256, seed=2)


def test_mirror_sixteen_total_bits_never_clamp(h_case):
    """h.txt: the totals of 6-bit messages stay far inside 16 bits (a column of degree 15: |T| <= 31 + 15 * 31), so p = 16
    gives exactly what the mirror gives with the total clamp removed."""
    _, mir, llr = h_case
    for early, iters in ((True, 50), (False, 10)):
        a = mir.decode(llr[:64], 6, 16, 0.25, 0.8125, 0.0, early_term=early, iterations=iters)
        b = mir.decode(llr[:64], 6, None, 0.25, 0.8125, 0.0, early_term=early, iterations=iters)
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), (early, k)
        assert a["clamp_share"] == 0.0 and np.abs(a["llr_out"]).max() > 31 * 0.25


def test_mirror_step_order_within_a_step_does_not_matter(h_case):
    """The check nodes of a step share no variable node: one by one, forward or reversed, equals all at once — with a
    total width that clamps."""
    _, mir, llr = h_case
    ref = mir.decode(llr[:24], 6, 7, 0.25, 0.8125, 0.0, early_term=True, iterations=12)
    assert ref["clamp_share"] > 0
    for order in ("forward", "reversed"):
        r = mir.decode(llr[:24], 6, 7, 0.25, 0.8125, 0.0, early_term=True, iterations=12, row_order=order)
        for k in KEYS + ("clamp_share",):
            assert np.array_equal(r[k], ref[k]), (order, k)


def test_mirror_what_it_is_for(h_case):
    """h.txt, AWGN -3.5 dB, 256 frames, plain min-sum, 6-bit messages at step 0.25, 50 sweeps with early termination.  Eight
    total bits decode (observed: 3 failing frames; binary64 layered and 6-bit flooding fail 2 each), six do not (observed:
    all 256 fail — the degree-15 punctured columns pin their totals at +-31), and the layered schedule keeps its point in
    fixed point: 0.538 of the flooding quantized decoder's iterations over the 251 frames both converge on."""
    code, mir, llr = h_case
    p8 = mir.decode(llr, 6, 8, 0.25)
    p6 = mir.decode(llr, 6, 6, 0.25)
    flood = QuantizedMinSumMirror(code).decode(llr, 6, 0.25)
    fail8, fail6 = int((p8["bit_errors"] > 0).sum()), int((p6["bit_errors"] > 0).sum())
    both = (p8["iters"] < 50) & (flood["iters"] < 50)
    ratio = p8["iters"][both].mean() / flood["iters"][both].mean()
    print("failing frames: p = 8:", fail8, "p = 6:", fail6, "flooding 6-bit:", int((flood["bit_errors"] > 0).sum()),
          "sweeps / iterations:", ratio, "over", int(both.sum()), "clamp shares", p8["clamp_share"], p6["clamp_share"])
    assert fail8 <= 8
    assert fail6 >= 200
    assert both.sum() >= 200 and ratio < 0.7
