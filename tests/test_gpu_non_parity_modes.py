"""The three opt-in NON-PARITY sum-product modes (ldpc_hip_set_fast_mode: 1 flooding binary32, kernels_fast.hip; 2 / 3 layered
with binary32 / binary16 messages, kernels_layered.hip) on the four codes of non_parity_codes.py — whose docstring says which
check-node and variable-node instantiations each code reaches — against their plain-C mirror (oracle/ldpc_oracle.c,
orc.Code.decode_fast), element by element, and against themselves and the host, bit for bit.

Tolerances come from the mirror, never from the kernels.  The YARDSTICK is the mirror against itself on inputs moved by
2e-7 (non_parity_codes.yardstick_inputs), the deviation |a - b| / max(|a|, 1) of llr_out with a the mirror's; it is computed
at run time, and test_non_parity_modes_host.py checks on the CPU that it is neither zero nor large.

A, fixed sweeps (1, 2, 3, no early termination): iters exact; every llr_out within 16 x the yardstick's largest deviation for
   that code, mode, channel and sweep count; hard equal wherever the mirror's |llr_out| exceeds that bound (at most 1 % of the
   elements may be left out).  Why 16: the mirror uses libm and IEEE division, the kernels v_exp_f32, v_log_f32 and v_rcp_f32,
   each about one ulp off, and they depart at every one of those instructions, not only at the input as the yardstick does; the
   longest chain through a degree-8 check node has about 16 of them (exp2, up to 7 rho / lambda each with a reciprocal, log2).
   A structural error — a wrong neighbour, a missing clip, a wrong order — gives deviations of order 1.
B, whole decodes (early termination, 30 iterations): the frames whose iters or hard differ from the mirror's number at most
   4 x the yardstick's such frames + 4 of 512 — counted once over all frames and once more over the frames in which the
   mirror has no |llr_out| within the bound (np_mix has exact ties on the BSC, which make the first count's cap a loose one
   there: non_parity_codes.py, Whole); on the agreeing frames the mirror converged on, llr_out within 16 x the yardstick's
   largest deviation over ITS agreeing converged frames of the same run.
C, exact properties of every mode, and D, the refusals: see the tests.

Measured on an MI355X, the largest deviation as a multiple of the yardstick's (worst case over the four codes, AWGN and BSC):
  fixed sweeps   mode 1: 1.87 (np_mix)   mode 2: 1.52 (np_r48)   mode 3: 2.30 (np_r48)
  whole decodes  mode 1: 2.63 (np_r37)   mode 2: 2.59 (np_r48)   mode 3: 2.39 (np_r37)
  mode 1's variable-node codes (fixed sweeps): np_vn16 0.85, np_vn20 1.20, np_vn12 0.96, np_vn7 0.59
against the margin of 16; the tests print each run's figure (pytest -s).  Frames that disagree in B: none, or one where the
yardstick has one, except np_mix on the BSC in modes 1 and 2 (60 and 63 against the yardstick's 49: exact ties,
non_parity_codes.py, Whole) — and none there among the 399 frames without a tie.
"""
import zlib

import numpy as np
import pytest

import non_parity_codes as npc
import orc
from minsum_common import WANT, check_no_iteration, check_split_batch, dumped, same, write
from test_gpu_random_codes import make_code_by_degrees

pytestmark = pytest.mark.gpu
CASES = [(mode, name) for name in npc.NAMES for mode in npc.MODES]
IDS = [f"mode{mode}-{name}" for mode, name in CASES]
ALL = ("iters", "bit_errors", "hard", "llr_out", "llr_in", "codeword")


class Ctx:
    """One code: its file, the oracle's view, ONE decoder for the module, and the dumped inputs."""

    def __init__(self, name, path):
        import libldpc_amd
        self.name, self.path, self.code = name, path, orc.Code(path)
        self.d = libldpc_amd.HipDecoder(path)
        self.llr = {}

    @property
    def fresh(self):
        """A second context that is never switched to a mode: what "a fresh context" gives."""
        if not hasattr(self, "_fresh"):
            import libldpc_amd
            self._fresh = libldpc_amd.HipDecoder(self.path)
        return self._fresh

    def inputs(self, ch):
        """llr_in of 512 frames of the reference stream, seed 7, dumped with the mode off."""
        if ch not in self.llr:
            x = dict(npc.CHANNELS[self.name])[ch]
            self.llr[ch] = dumped(self.d, lambda d: d.set_fast_mode(0), ch, x, npc.FRAMES, seed=npc.SEED)
        return self.llr[ch]

    def run(self, mode, llr, early, iters, want=WANT):
        self.d.set_fast_mode(mode)
        try:
            return self.d.decode_batch(llr, early_term=early, iterations=iters, decoding="BP", want=want)
        finally:
            self.d.set_fast_mode(0)


@pytest.fixture(scope="module")
def ctxs(tmp_path_factory):
    paths = npc.write_codes(tmp_path_factory.mktemp("non_parity"), npc.NAMES + npc.VN_NAMES)
    return {name: Ctx(name, path) for name, path in paths.items()}


@pytest.mark.parametrize("mode,name", CASES, ids=IDS)
def test_fixed_sweeps_against_the_mirror(ctxs, mode, name):
    """A.  One, two and three sweeps without early termination, AWGN and BSC (BSC: two input magnitudes only, so equal
    operands everywhere in the first sweep), through decode_batch.  np_mix: cn_fast / cn_layered of every degree 2..8 with the
    D == 2 special case, the generic variable-node loop (degree 17), vn_fast_wide 9 / 6 / 4, vn_fast_any 4 / 3, vn_fast<1> and
    <2>, seven degree classes of layered steps with partly filled ones, shortened columns (+-99999.9 into the +-40 clip) and
    punctured ones (a zero input: rho = 1); the regular codes: degrees 6, 8 and 7 alone, vn_fast_wide / vn_fast_any 3 and 4."""
    c = ctxs[name]
    worst = 0.0
    for ch, _ in npc.CHANNELS[name]:
        llr = c.inputs(ch)
        for iters in npc.SWEEPS:
            s = npc.Sweeps(c.code, mode, llr, iters)
            worst = max(worst, s.check(c.run(mode, llr, False, iters), (name, mode, ch, iters)))
    print(f"MULTIPLE sweeps mode {mode} {name}: {worst:.3f}")


@pytest.mark.parametrize("name", npc.VN_NAMES)
def test_variable_node_switches(ctxs, name):
    """A again, mode 1 only, on the four codes that between them put every degree 3..16 first in a wave (vn_fast_wide: the slot
    indices unpacked from registers) and every degree 3..16 behind another block (vn_fast_any: the slot table), and degrees
    17..20 into the generic loop (non_parity_codes.py says which code reaches which); and the same sweeps without llr_out."""
    c = ctxs[name]
    llr = c.inputs("AWGN")
    worst = 0.0
    for iters in npc.SWEEPS:
        s = npc.Sweeps(c.code, 1, llr, iters)
        got = c.run(1, llr, False, iters)
        worst = max(worst, s.check(got, (name, 1, "AWGN", iters)))
        assert np.array_equal(got["hard"], (got["llr_out"] <= 0).astype(np.uint8)), (name, iters)
        part = c.run(1, llr, False, iters, want=("iters", "hard", "bit_errors"))
        assert all(np.array_equal(part[k], got[k]) for k in part), (name, iters)
    print(f"MULTIPLE sweeps mode 1 {name}: {worst:.3f}")


@pytest.mark.parametrize("mode,name", CASES, ids=IDS)
def test_whole_decodes_against_the_mirror(ctxs, mode, name):
    """B.  Early termination, 30 iterations: the syndrome vote of mode 1 (sign bits through cn_fast<D>, the ballot), cn_parity<D>
    of modes 2 / 3, the iteration-count conventions (mode 1 counts back by one, the layered modes do not count the sweep that
    passed), frames that stop in different sweeps and frames that never do."""
    c = ctxs[name]
    worst = 0.0
    for ch, _ in npc.CHANNELS[name]:
        llr = c.inputs(ch)
        w = npc.Whole(c.code, mode, llr)
        worst = max(worst, w.check(c.run(mode, llr, True, npc.WHOLE_ITERATIONS), (name, mode, ch)))
    print(f"MULTIPLE whole mode {mode} {name}: {worst:.3f}")


@pytest.mark.parametrize("mode,name", CASES, ids=IDS)
def test_exact_properties(ctxs, mode, name):
    """C 1..7, bit for bit: decisions are the signs of llr_out; bit_errors is the host's count over the transmitted positions;
    a frame that stopped early has a zero syndrome; a batch split in two, and one frame alone (tail workgroups, the frame
    index), give the batch's rows; the WANT_LLR = false kernels (no llr_out asked for) give the values of the full ones;
    iterations = 0 gives zeros with early termination on and off; stream_decode with the mode on (the fused binary64 channel,
    AWGN and BSC) equals decode_batch of its own dumped llr_in — and on np_mix, with punctured and shortened columns, that
    llr_in and codeword are the oracle's."""
    c = ctxs[name]
    code, iters = c.code, npc.WHOLE_ITERATIONS
    for ch, x in npc.CHANNELS[name]:
        llr = c.inputs(ch)[:70]
        for early, its in ((True, iters), (False, 2)):
            what = (name, mode, ch, early)
            one = check_split_batch(lambda part: c.run(mode, part, early, its), llr)                      # 4
            same(c.run(mode, llr[37:38], early, its), one, what, slice(37, 38))
            assert np.array_equal(one["hard"], (one["llr_out"] <= 0).astype(np.uint8)), what                # 1
            count = (one["hard"][:, code.bit_pos] != 0).sum(axis=1)  # (decode_batch has no codeword: all-zero)
            assert np.array_equal(one["bit_errors"], count.astype(np.uint32)), what                         # 2
            stopped = np.flatnonzero(one["iters"] < its)
            assert (stopped.size > 0) == early, what
            for f in stopped:                                                                               # 3
                assert not code.syndrome(one["hard"][f]).any(), (what, f)
            for want in (("iters", "bit_errors"), ("iters", "hard")):                                       # 5
                part = c.run(mode, llr, early, its, want=want)
                for k in want:
                    assert np.array_equal(part[k], one[k]), (what, want, k)
            check_no_iteration(c.run(mode, llr[:5], early, 0))                                              # 6
            c.d.set_fast_mode(mode)                                                                         # 7
            c.d.stream_begin(ch, npc.SEED, x)
            r = c.d.stream_decode(70, early_term=early, iterations=its, decoding="BP", want=ALL)
            c.d.set_fast_mode(0)
            assert np.array_equal(r["llr_in"], llr), what  # the channel is the binary64 one in every mode
            same({k: r[k] for k in WANT}, one, what)
            count = (r["hard"][:, code.bit_pos] != r["codeword"][:, code.bit_pos]).sum(axis=1)
            assert np.array_equal(r["bit_errors"], count.astype(np.uint32)), what
            if name == "np_mix":
                o = code.run_frames(ch, x, seed=npc.SEED, count=70, iters=0, math=orc.MATH_DET)
                assert np.array_equal(r["llr_in"], o["llr_in"]) and np.array_equal(r["codeword"], o["codeword"]), what
                # a shortened column: 99999.9 on the AWGN channel (into the +-40 clip), the magnitude of every other on the BSC
                assert (r["llr_in"][:, code.shorten] == (99999.9 if ch == "AWGN" else np.abs(r["llr_in"][:, :1]))).all(), what
                assert not r["llr_in"][:, code.puncture].any(), what


@pytest.mark.parametrize("mode,name", CASES, ids=IDS)
def test_nothing_else_moves(ctxs, mode, name):
    """C 8.  With the mode on, BP_MS results equal a fresh context's (min-sum ignores the mode); after set_fast_mode(0), BP
    equals a fresh context's."""
    c = ctxs[name]
    ch, x = npc.CHANNELS[name][0]

    def stream(d, dec, early):
        d.stream_begin(ch, 2, x)
        return d.stream_decode(48, early_term=early, iterations=20, decoding=dec, want=ALL)
    c.d.set_fast_mode(mode)
    try:
        on = {early: stream(c.d, "BP_MS", early) for early in (True, False)}
        moved = stream(c.d, "BP", True)
    finally:
        c.d.set_fast_mode(0)
    for early in (True, False):
        ref = stream(c.fresh, "BP_MS", early)
        for k in ALL:
            assert np.array_equal(on[early][k], ref[k]), (name, mode, "BP_MS", early, k)
        off, ref = stream(c.d, "BP", early), stream(c.fresh, "BP", early)
        for k in ALL:
            assert np.array_equal(off[k], ref[k]), (name, mode, "BP", early, k)
        if early:  # ... and the mode did change BP, on the same inputs
            assert np.array_equal(moved["llr_in"], ref["llr_in"]) and not np.array_equal(moved["llr_out"], ref["llr_out"])


@pytest.mark.parametrize("mode", npc.MODES)
def test_counter_noise_does_not_combine(ctxs, mode):
    """C 9.  set_noise("counter") with a mode on: stream_decode fails and says what to do; after set_noise("reference") the
    context decodes again, in the mode."""
    c = ctxs["np_r36"]
    ch, x = npc.CHANNELS["np_r36"][0]
    c.d.set_fast_mode(mode)
    try:
        c.d.set_noise("counter")
        c.d.stream_begin(ch, npc.SEED, x)
        with pytest.raises(RuntimeError, match=r"set_fast_mode\(0\)"):
            c.d.stream_decode(4, decoding="BP")
        c.d.set_noise("reference")
        c.d.stream_begin(ch, npc.SEED, x)
        r = c.d.stream_decode(8, iterations=npc.WHOLE_ITERATIONS, decoding="BP", want=WANT)
    finally:
        c.d.set_noise("reference")
        c.d.set_fast_mode(0)
    same(r, c.run(mode, c.inputs(ch)[:8], True, npc.WHOLE_ITERATIONS), ("after counter", mode))


FAST_TEXT = "fast mode: this code is outside what the binary32 kernel takes"
LAYERED_TEXT = "layered mode: this code is outside what the layered kernel takes"


def _refused_codes(directory):
    """name -> (path, modes that refuse it)."""
    out = {}
    # one check node of degree 9 among degree-6 ones: 9 + 6 * 50 = 3 * 103 edges
    rng = np.random.default_rng(zlib.crc32(b"np_cn9"))
    out["cn9"] = (make_code_by_degrees(str(directory / "np_cn9.txt"), [3] * 103, [9] + [6] * 50, rng), npc.MODES)
    # an isolated column: a (3,6) code of 96 columns with column 10 left out of every row
    rng = np.random.default_rng(zlib.crc32(b"np_isolated"))
    tmp = make_code_by_degrees(str(directory / "np_isolated_src.txt"), [3] * 96, [6] * 48, rng)
    rows = [[] for _ in range(48)]
    for line in open(tmp).read().split("\n"):
        r, col = map(int, line.split())
        rows[r].append(col + (col >= 10))
    out["isolated"] = (write(directory / "np_isolated.txt", rows), npc.MODES)
    # (3,6), 2304 columns: 36 variable-node blocks, nine to a wave — more than the eight kernels_fast.hip keeps; the layered
    # modes take it
    rng = np.random.default_rng(zlib.crc32(b"np_r36_2304"))
    out["r36_2304"] = (make_code_by_degrees(str(directory / "np_r36_2304.txt"), [3] * 2304, [6] * 1152, rng), (1,))
    return out


def _marked(n, nc, dtype, per_bit):
    """An output array of n frames with every byte 0xA5."""
    a = np.full((n, (nc if per_bit else 1) * np.dtype(dtype).itemsize), 0xA5, np.uint8).view(dtype)
    return a if per_bit else a.reshape(n)


@pytest.mark.parametrize("which", ["cn9", "isolated", "r36_2304"])
def test_refusals(which, tmp_path):
    """D.  A code a mode does not take: the first BP decode raises with the text of Engine::refusal for that mode and writes
    no output array; a mode that does take it decodes; after set_fast_mode(0) the same context decodes BP as a fresh one."""
    import libldpc_amd
    path, refusing = _refused_codes(tmp_path)[which]
    d, fresh = libldpc_amd.HipDecoder(path), libldpc_amd.HipDecoder(path)
    assert np.bincount(orc.Code(path).edge_col, minlength=d.nc).min() == (0 if which == "isolated" else 3)
    llr = np.where(np.random.default_rng(3).random((6, d.nc)) < 0.03, -2.0, 3.0)
    ref = fresh.decode_batch(llr, iterations=20, decoding="BP", want=WANT)
    for mode in npc.MODES:
        d.set_fast_mode(mode)
        assert d.decoder_choice() == npc.DECODER[mode]
        if mode in refusing:
            out = {k: _marked(6, d.nc, *d.OUT_SPEC[k]) for k in WANT}
            with pytest.raises(RuntimeError) as e:
                d.decode_batch(llr, iterations=20, decoding="BP", want=WANT, out=out)
            assert (FAST_TEXT if mode == 1 else LAYERED_TEXT) in str(e.value), (which, mode, str(e.value))
            for k, v in out.items():
                assert (v.view(np.uint8) == 0xA5).all(), (which, mode, k)
        else:
            r = d.decode_batch(llr, iterations=20, decoding="BP", want=WANT)
            it, _, hard = orc.Code(path).decode_fast(mode, llr, early_term=True, iters=20)  # (far below the code's threshold)
            assert np.array_equal(r["hard"], hard) and np.array_equal(r["iters"], it) and (it < 20).all(), (which, mode)
            assert np.array_equal(r["hard"], (r["llr_out"] <= 0).astype(np.uint8)), (which, mode)
        d.set_fast_mode(0)
        same(d.decode_batch(llr, iterations=20, decoding="BP", want=WANT), ref, (which, mode, "off again"))
