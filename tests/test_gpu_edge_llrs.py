"""Caller-supplied LLRs at the edges (tests/edge_llrs.py) through ldpc_hip_decode_batch and ldpc_hip_decode_batch_typed on every
binary64 decoder: the kernels' prologues, escape votes, list launch and decision rules where the arithmetic forms switch.

Class P and class T: bit for bit against the det-mode oracle (or the mode's numpy mirror) over iters, hard, bit_errors, llr_out
and llr_in as uint64, after the oracle's output has been checked to hold no NaN.  Class N (frames in which the reference's
arithmetic makes NaN): containment and determinism only — include/ldpc_amd.h, ldpc_hip_decode_batch.  Fast modes 1..3 are a
tolerance tier: a metamorphic check through their input clip.  test_edge_llrs_host.py holds the yardsticks themselves."""
import zlib

import numpy as np
import pytest

import edge_llrs as el
import orc
from layered_fixed_minsum_ref import LayeredFixedMinSumMirror
from layered_minsum_ref import LayeredMinSumMirror
from minsum_common import WANT, same
from minsum_ref import MinSumMirror
from quantized_minsum_ref import QuantizedMinSumMirror
from test_gpu_layered_min_sum import irregular_code
from test_gpu_random_codes import CASES as RANDOM_CASES, FUSED_CASES, make_code, make_code_by_degrees, make_fused_code
from test_gpu_typed_batch import typed

pytestmark = pytest.mark.gpu
ITERS = 20
ALL = WANT + ("llr_in",)
RUNS = {"bp_early": (False, True), "bp_full": (False, False), "ms_early": (True, True), "ms_full": (True, False)}


def _random_case(name):
    return next(c for c in RANDOM_CASES if c[0] == name)


def _write(name, path):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name in ("h_txt", "h_txt_program"):
        return orc.H_TXT
    if name == "h_txt_shortened":
        return orc.shortened_variant(path)
    if name == "fused_general":
        _, cn_spec, vn_degs, punct, short = next(c for c in FUSED_CASES if c[0] == name)
        return make_fused_code(path, rng, cn_spec, vn_degs, punct, short)
    if name in ("lds_wide_cn", "mem_cn20"):
        _, nc, mc, pool, punct, short, skip, _ = _random_case(name)
        return make_code(path, nc, mc, rng.choice(pool, size=mc), rng, punct, short, skip)
    if name == "irregular_237":
        return irregular_code(path)
    vn, cn = {"lds_regular_3_6": ([3] * 600, [6] * 300), "registers_totals": ([3] * 8192, [6] * 4096),
              "registers_messages": ([1] * 600 + [3] * 7200, [6] * 3700)}[name]
    return make_code_by_degrees(path, vn, cn, rng)


# name -> (AWGN point of the base frames, base frames, the cut of the value list, what the context must report)
SPECS = {
    "h_txt_program": (-4.5, 8, None, lambda d: d.residency == "lds" and d.fused_plan()["ok"] == 1 and d.fused_program() >= 0),
    "h_txt": (-4.5, 8, None, lambda d: d.residency == "lds" and d.fused_plan()["ok"] == 1 and d.fused_plan()["small"] == 1),
    "fused_general": (3.0, 8, None, lambda d: d.residency == "lds" and d.fused_plan()["ok"] == 1 and d.fused_plan()["small"] == 0
                      and d.fused_plan()["vnb"] > 4 and d.fused_plan()["cnl"] == 2 and d.fused_program() < 0),
    "lds_wide_cn": (3.0, 8, None, lambda d: d.residency == "lds" and d.fused_plan()["ok"] == 0),
    "lds_regular_3_6": (2.0, 8, None, lambda d: d.residency == "lds" and d.fused_plan()["ok"] == 0),
    "mem_cn20": (6.0, 8, None, lambda d: d.residency == "memory"),
    "registers_totals": (2.2, 2, el.BOX_VALUES, lambda d: d.residency == "registers" and d.register_form == "totals"),
    "registers_messages": (2.2, 2, el.BOX_VALUES, lambda d: d.residency == "registers" and d.register_form == "messages"),
    "irregular_237": (2.0, 8, None, lambda d: d.nc == 237),
    "h_txt_shortened": (-4.5, 8, None, lambda d: d.residency == "lds"),
}


class Ctx:
    """One code: the oracle's view, one decoder, its base and class-P frames, and a cache of yardstick results."""

    def __init__(self, name, directory):
        import libldpc_amd
        self.name = name
        x, n_base, values, self.runs_where = SPECS[name]
        self.path = _write(name, str(directory / f"{name}.txt"))
        self.code = orc.Code(self.path)
        self.d = libldpc_amd.HipDecoder(self.path)
        assert (self.d.nc, self.d.mc, self.d.nnz) == (self.code.nc, self.code.mc, self.code.nnz)
        self.base = self.code.run_frames("AWGN", x, seed=7, count=max(n_base, 8), iters=0, math=orc.MATH_DET)["llr_in"]
        cut = values is not None
        self.frames = el.class_p(self.code, self.base[:n_base], values=values, placements=("eight",) if cut else ("eight", "one"),
                                 whole=not cut)
        self.llr = el.stack(self.frames)
        self.ref = {}

    def oracle(self, ms, early, frames=None, key="p"):
        """The det-mode oracle on the frames, checked for the class-P condition before anything is compared with it."""
        k = (key, ms, early)
        if k not in self.ref:
            self.ref[k] = r = el.oracle_decode(self.code, self.frames if frames is None else frames, ms, early, ITERS, orc.MATH_DET)
            assert not np.isnan(r["llr_out"]).any(), (self.name, k, "a NaN in the oracle's output: a mistake in the builder")
        return self.ref[k]


@pytest.fixture(scope="module")
def ctxs(tmp_path_factory):
    directory, made = tmp_path_factory.mktemp("edge_llrs"), {}

    def get(name):
        if name not in made:
            made[name] = Ctx(name, directory)
            assert made[name].runs_where(made[name].d), (name, made[name].d.residency, made[name].d.fused_plan())
        return made[name]
    return get


def _plain(d):
    d.set_min_sum_layered_fixed(0)
    d.set_min_sum_quantization(0)
    d.set_min_sum_ternary(0)
    d.set_min_sum_schedule("flooding")
    d.set_fast_mode(0)
    d.set_min_sum_correction()


def _compare(r, y, rows, what, want):
    for k in want:
        a, b = r[k], np.asarray(y[k])[rows].astype(r[k].dtype)
        if k in ("llr_out", "llr_in"):
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero((a != b).reshape(len(rows), -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, [what[-1][i] for i in bad[:6]])


def _decode_in_batches(c, frames, llr, early, decode):
    """decode(rows of llr, iteration limit) over the batches of the frames -> [(row indices, results)]"""
    return [(idx, decode(llr[idx], el.SHORT_ITERATIONS if short else ITERS)) for idx, short in el.batches(frames, early)]


PARITY_CASES = [n for n in SPECS if n != "h_txt_shortened"]


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("name", PARITY_CASES)
def test_class_p_parity(ctxs, name, run):
    """Every class-P frame on the decoder the case names, sum-product and min-sum, with and without early termination."""
    c = ctxs(name)
    ms, early = RUNS[run]
    _plain(c.d)
    want = ("iters", "hard", "bit_errors") if name == "h_txt_program" else ALL  # (no llr_out: the compiled program's kernel)
    assert c.d.decoder_choice(early, ITERS, "BP_MS" if ms else "BP") == "resident"
    y = c.oracle(ms, early)
    for idx, r in _decode_in_batches(c, c.frames, c.llr, early, lambda part, iters: c.d.decode_batch(
            part, early_term=early, iterations=iters, decoding="BP_MS" if ms else "BP", want=want)):
        _compare(r, y, idx, (name, run, [c.frames[i].name for i in idx]), want)
    if run == "bp_early" and SPECS[name][2] is None:
        b = c.d.decode_batch(c.base, early_term=True, iterations=ITERS, want=("iters", "bit_errors"))
        print(name, "base frames: iters", b["iters"].tolist(), "bit errors", b["bit_errors"].tolist())
        assert (y["iters"] < ITERS).any() and (y["iters"] == ITERS).any()  # frames that converge and frames that do not


# setting, the decoder it must select, the mirror's class, how the mirror is called
VARIANT_RUNS = {
    "corrected": (lambda d: d.set_min_sum_correction(0.8125, 0.25), "resident", MinSumMirror,
                  lambda m, llr, early, iters: m.decode(llr, 0.8125, 0.25, early_term=early, iterations=iters)),
    "layered": (lambda d: d.set_min_sum_schedule("layered"), "layered-min-sum", LayeredMinSumMirror,
                lambda m, llr, early, iters: m.decode(llr, 1.0, 0.0, early_term=early, iterations=iters)),
    "quantized": (lambda d: d.set_min_sum_quantization(6, 0.25), "quantized-min-sum", QuantizedMinSumMirror,
                  lambda m, llr, early, iters: m.decode(llr, 6, 0.25, early_term=early, iterations=iters)),
    "layered_fixed": (lambda d: d.set_min_sum_layered_fixed(6, 8, 0.25), "layered-fixed-min-sum", LayeredFixedMinSumMirror,
                      lambda m, llr, early, iters: m.decode(llr, 6, 8, 0.25, early_term=early, iterations=iters)),
}


@pytest.mark.parametrize("variant", list(VARIANT_RUNS))
@pytest.mark.parametrize("name", ["h_txt", "irregular_237"])
def test_class_p_min_sum_variants(ctxs, name, variant):
    """Corrected, layered, quantized and fixed-point layered min-sum (binary64 input: the widened path) against their mirrors."""
    c = ctxs(name)
    on, choice, mirror_class, call = VARIANT_RUNS[variant]
    mir = mirror_class(c.code)
    _plain(c.d)
    on(c.d)
    try:
        assert c.d.decoder_choice(True, ITERS, "BP_MS") == choice
        for early in (True, False):
            for idx, short in el.batches(c.frames, early):
                iters = el.SHORT_ITERATIONS if short else ITERS
                m = call(mir, c.llr[idx], early, iters)
                assert not np.isnan(m["llr_out"]).any(), (name, variant, early)
                r = c.d.decode_batch(c.llr[idx], early_term=early, iterations=iters, decoding="BP_MS", want=ALL)
                m["llr_in"] = c.llr[idx]
                _compare(r, m, list(range(len(idx))), (name, variant, early, [c.frames[i].name for i in idx]), ALL)
    finally:
        _plain(c.d)


@pytest.mark.parametrize("name", ["h_txt", "fused_general", "lds_regular_3_6", "registers_totals", "mem_cn20"])
def test_class_t_parity(ctxs, name):
    """Tiny positive inputs (0 < L < 2^-53): the ratio forms refuse the frame (detmath.h, dm_ratio_llr_refused) and the
    LLR-domain form evaluates a check node that holds such an input term by term (dm_llr_tiny), as the oracle does."""
    c = ctxs(name)
    _plain(c.d)
    frames = el.class_t(c.code, c.base[:2])
    llr = el.stack(frames)
    for run, (ms, early) in RUNS.items():
        y = c.oracle(ms, early, frames, key="t")
        r = c.d.decode_batch(llr, early_term=early, iterations=ITERS, decoding="BP_MS" if ms else "BP", want=ALL)
        _compare(r, y, list(range(len(frames))), (name, run, [f.name for f in frames]), ALL)
    y = c.oracle(False, True, frames, key="t")
    assert not y["iters"][:2].any() and not y["hard"][:2].any()  # all inputs positive: the all-zero word at once


@pytest.mark.parametrize("kind", ["float32", "float16"])
def test_typed_entry(ctxs, kind):
    """The same frames as float32 and float16 on h.txt with columns 130 and 290 (two of check node 0's three neighbours)
    shortened: the typed call equals decode_batch on the widened values W bit for bit, whatever W holds; W equals the oracle
    wherever the structural rule (edge_llrs.makes_nan) finds no NaN-making pair of infinities — in binary16 the shortened
    columns' 99999.9 are +inf twice on check node 0, and every frame that keeps them is class N."""
    c = ctxs("h_txt_shortened")
    assert c.code.num_shorten == 4 and (c.base[:, [130, 290]] == 99999.9).all()
    _plain(c.d)
    g = el.Graph(c.code)
    t, W = typed(c.llr, kind)
    wide = [el.Frame(f.name, W[i], f.short) for i, f in enumerate(c.frames)]
    clean = [i for i, f in enumerate(wide) if not el.makes_nan(g, f.llr)]
    twice = [i for i in range(len(wide)) if np.isinf(W[i, [130, 290]]).all()]  # (the whole-frame edges overwrite the columns)
    assert not set(twice) & set(clean) and (len(twice) > 90 if kind == "float16" else len(clean) > 90)
    for run, (ms, early) in RUNS.items():
        dec = "BP_MS" if ms else "BP"
        if clean:
            y = c.oracle(ms, early, [wide[i] for i in clean], key=kind)
        for idx, short in el.batches(wide, early):
            iters = el.SHORT_ITERATIONS if short else ITERS
            r = c.d.decode_batch_typed(t[idx], early_term=early, iterations=iters, decoding=dec, want=ALL)
            w = c.d.decode_batch(W[idx], early_term=early, iterations=iters, decoding=dec, want=ALL)
            _compare(r, w, list(range(len(idx))), (kind, run, "typed against widened", [wide[i].name for i in idx]), ALL)
            assert (w["iters"] <= iters).all() and (w["hard"] <= 1).all()
            sel = [j for j, i in enumerate(idx) if i in clean]
            if sel:
                part = {k: w[k][sel] for k in ALL}
                _compare(part, y, [clean.index(idx[j]) for j in sel], (kind, run, "widened against the oracle",
                                                                       [wide[idx[j]].name for j in sel]), ALL)


@pytest.mark.parametrize("mode,choice", [(1, "fast32"), (2, "layered32"), (3, "layered16")])
def test_fast_modes_clip_their_input(ctxs, mode, choice):
    """Modes 1..3 clip the channel LLRs at +-27.7, so a frame with +-inf, +-1e300, +-1e13 or +-99999.9 on some columns decodes
    bit for bit like the same frame with +-1e6 there, on the same kernel."""
    c = ctxs("h_txt")
    rows = [i for i, f in enumerate(c.frames) if (np.abs(f.llr) >= 99999.9).any()]
    assert len(rows) >= 14 and any(np.isinf(c.llr[i]).any() for i in rows)
    big = c.llr[rows]
    mild = np.where(np.abs(big) >= 99999.9, np.copysign(1e6, big), big)
    _plain(c.d)
    c.d.set_fast_mode(mode)
    try:
        assert c.d.decoder_choice(True, ITERS, "BP") == choice
        for early in (True, False):
            a = c.d.decode_batch(big, early_term=early, iterations=ITERS, decoding="BP", want=WANT)
            b = c.d.decode_batch(mild, early_term=early, iterations=ITERS, decoding="BP", want=WANT)
            same(a, b, (mode, early))
            assert not np.isnan(a["llr_out"]).any() and a["iters"].max() > 0
    finally:
        _plain(c.d)


# ---- class N: containment and determinism ----
N_POSITIONS = (0, 31, 32, 69)
N_DECODERS = {
    # name -> (code, what to ask for, the setting, the decodings)
    "h_txt_with_llr_out": ("h_txt", ALL, None, ("BP", "BP_MS")),
    "h_txt_program": ("h_txt_program", ("iters", "hard", "bit_errors"), None, ("BP", "BP_MS")),
    "fused_general": ("fused_general", ALL, None, ("BP", "BP_MS")),
    "registers_totals": ("registers_totals", ALL, None, ("BP", "BP_MS")),
    "mem_cn20": ("mem_cn20", ALL, None, ("BP", "BP_MS")),
    "layered_min_sum": ("h_txt", ALL, "layered", ("BP_MS",)),
    "quantized_min_sum": ("h_txt", ALL, "quantized", ("BP_MS",)),
}


def _bits(r, k, i):
    v = r[k][i]
    return v.view(np.uint64).tobytes() if v.dtype == np.float64 else np.asarray(v).tobytes()


@pytest.mark.parametrize("decoder", list(N_DECODERS))
def test_class_n_containment(ctxs, decoder):
    """70 frames with class-N frames at positions 0, 31, 32 and 69: every ordinary frame comes out as in a batch without them,
    a class-N frame keeps iters <= the limit and hard in {0, 1}, and two runs give the same bits.  How a class-N frame compares
    with the det-mode oracle is printed, not asserted (profiles/README.md holds the table)."""
    name, want, variant, decodings = N_DECODERS[decoder]
    c = ctxs(name)
    ordinary = c.code.run_frames("AWGN", SPECS[name][0], seed=11, count=70 - len(N_POSITIONS), iters=0, math=orc.MATH_DET)["llr_in"]
    nan_frames = el.class_n(c.code, c.base)
    where = [i for i in range(70) if i not in N_POSITIONS]
    _plain(c.d)
    if variant:
        VARIANT_RUNS[variant][0](c.d)
    try:
        for dec in decodings:
            for early in (True, False):
                alone = c.d.decode_batch(ordinary, early_term=early, iterations=ITERS, decoding=dec, want=want)
                for first in (0, 1):  # the five class-N frames, four to a batch
                    chosen = [nan_frames[(first + k) % len(nan_frames)] for k in range(len(N_POSITIONS))]
                    llr = np.empty((70, c.code.nc))
                    llr[where] = ordinary
                    llr[list(N_POSITIONS)] = el.stack(chosen)
                    r1 = c.d.decode_batch(llr, early_term=early, iterations=ITERS, decoding=dec, want=want)
                    r2 = c.d.decode_batch(llr, early_term=early, iterations=ITERS, decoding=dec, want=want)
                    for k in want:
                        for j, i in enumerate(where):
                            assert _bits(r1, k, i) == _bits(alone, k, j), (decoder, dec, early, k, "ordinary frame", i)
                        for i in N_POSITIONS:
                            assert _bits(r1, k, i) == _bits(r2, k, i), (decoder, dec, early, k, "two runs differ", i)
                    rows = list(N_POSITIONS)
                    assert (r1["iters"][rows] <= ITERS).all() and (r1["hard"][rows] <= 1).all()
                    if variant is None and first == 0:
                        _report(c, decoder, dec, early, chosen, r1, rows, want)
    finally:
        _plain(c.d)


def _report(c, decoder, dec, early, frames, r, rows, want):
    """Not asserted: a class-N frame against the det-mode oracle, by NaN positions and by bits elsewhere."""
    for f, i in zip(frames, rows):
        it, out, hard = c.code.decode(f.llr, min_sum=dec == "BP_MS", early_term=early, iters=ITERS, math=orc.MATH_DET)
        if it != r["iters"][i] or not np.array_equal(hard, r["hard"][i]):
            verdict = "differs in hard or iters"
        elif "llr_out" not in want:
            verdict = "equal (iters, hard)"
        else:
            a, b = r["llr_out"][i], out
            nan_same = np.array_equal(np.isnan(a), np.isnan(b))
            rest = ~np.isnan(b)
            verdict = "equal" if nan_same and np.array_equal(a[rest].view(np.uint64), b[rest].view(np.uint64)) else "differs in llr_out"
        print(f"CLASS-N {decoder} {dec} early={int(early)} {f.name}: {verdict} (oracle NaN outputs {int(np.isnan(out).sum())})")
