"""Ternary min-sum on the GPU (include/ldpc_amd.h, ldpc_hip_set_min_sum_ternary; kernels_ternary.hip) against the numpy mirror
(tests/ternary_ref.py), bit for bit: iters, hard, bit_errors, and llr_out as uint64.  Then the fused channel paths, the
paths that must not move, the simulation loop and the CLI."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import orc
from minsum_common import WANT, check_no_iteration, check_split_batch, dumped, same
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
    for noise in ("reference", "counter"):
        d.set_noise(noise)
        for ch, x in (("AWGN", 4.5), ("BSC", 0.04)):
            for early in (True, False):
                d.stream_begin(ch, 6, x)
                r = d.stream_decode(N, early_term=early, iterations=30, decoding="BP_MS", want=WANT + ("llr_in",))
                b = d.decode_batch(r["llr_in"], early_term=early, iterations=30, decoding="BP_MS", want=WANT)
                same(b, r, (noise, ch, x, early))
                assert r["iters"].max() > 0 and (r["iters"] < 30).any() == early
                for want in (("iters", "bit_errors"), WANT):
                    d.stream_begin(ch, 6, x)
                    q = d.stream_decode(N, early_term=early, iterations=30, decoding="BP_MS", want=want)
                    for k in want:
                        assert np.array_equal(q[k], r[k]), (noise, ch, early, k)
    d.set_noise("reference")
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
    import libldpc_amd
    want = ("iters", "hard", "llr_out", "bit_errors", "llr_in")
    ter = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    fresh = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    ter.set_min_sum_ternary(2)
    for ch, x, dec, early in (("AWGN", -4.0, "BP", True), ("AWGN", -4.0, "BP", False), ("BSC", 0.24, "BP", True),
                              ("BEC", 0.7, "BP", True), ("BEC", 0.7, "BP_MS", True)):
        rs = []
        for d in (ter, fresh):
            d.stream_begin(ch, 2, x)
            rs.append(d.stream_decode(64, early_term=early, iterations=50, decoding=dec, want=want))
        for k in want:
            assert np.array_equal(rs[0][k], rs[1][k]), (ch, dec, early, k)
        if ch != "BEC":
            a = ter.decode_batch(rs[1]["llr_in"], early_term=early, decoding=dec, want=WANT)
            b = fresh.decode_batch(rs[1]["llr_in"], early_term=early, decoding=dec, want=WANT)
            for k in WANT:
                assert np.array_equal(a[k], b[k]), (ch, dec, k)
    # the mode does change BP_MS ...
    rs = []
    for d in (ter, fresh):
        d.stream_begin("AWGN", 4, -4.5)
        rs.append(d.stream_decode(32, iterations=50, decoding="BP_MS", want=want))
    assert np.array_equal(rs[0]["llr_in"], rs[1]["llr_in"])
    assert not np.array_equal(rs[0]["llr_out"].view(np.uint64), rs[1]["llr_out"].view(np.uint64))
    # ... and binary64 min-sum is back when it is off: flooding, layered, quantized
    ter.set_min_sum_ternary(0)
    variants = (lambda d: None, lambda d: d.set_min_sum_schedule("layered"),
                lambda d: (d.set_min_sum_schedule("flooding"), d.set_min_sum_quantization(6, 0.25)))
    for i, switch in enumerate(variants):
        for d in (ter, fresh):
            switch(d)
        for early in (True, False):
            rs = []
            for d in (ter, fresh):
                d.stream_begin("AWGN", 4, -4.5)
                rs.append(d.stream_decode(32, early_term=early, iterations=50, decoding="BP_MS", want=want))
            for k in want:
                assert np.array_equal(rs[0][k], rs[1][k]), (i, early, k)


def _fold(d, x, frames, seed):
    d.stream_begin("BSC", seed, x)
    r = d.stream_decode(frames, early_term=True, iterations=50, decoding="BP_MS", want=("iters", "bit_errors"))
    return frames, int((r["bit_errors"] > 0).sum()), int(r["bit_errors"].sum()), int(r["iters"].sum())


def _file_rows(path):
    return [ln.split()[:5] for ln in open(path).read().splitlines()]


def test_simulation_and_cli(cases, tmp_path):
    """simulate() with the mode on and counter noise gives the totals of a host fold of stream_decode over the same frames;
    the CLI with --ms-ternary 1 --noise counter writes the same result file as the Python run, alone and as two ranks over
    shared memory; --ms-ternary is refused with BP, --ms-bits, --ms-schedule layered and --ms-scale."""
    c = cases["r36"]
    d, code_file = c["d"], c["path"]
    d.set_noise("counter")
    d.set_min_sum_ternary(1)
    frames, xr, seed = 6000, (0.03, 0.045, 0.01), 5
    py_file = str(tmp_path / "py.txt")
    res = d.simulate("BSC", xr, seed=seed, decoding="BP_MS", max_frames=frames, fec=10**9, result_file=py_file,
                     cli_output=True)  # (the result file is written with the console table)
    assert res["totals"].shape == (2, 4)
    for i, x in enumerate((0.03 + 0.01, 0.03)):  # (the loop walks an eps axis from its far end, adding the step up from MIN)
        n, fe, be, it = _fold(d, x, frames, seed)
        assert res["totals"][i].tolist() == [n, fe, be, it], (x, res["totals"][i], (n, fe, be, it))
        assert 0 < fe < n
    d.set_noise("reference")
    _off(d)
    exe = os.path.join(ROOT, "libldpc_amd", "ldpcsim")
    head = [exe, code_file]
    tail = ["0.03", "0.045", "0.01", "-s", str(seed), "--decoding", "BP_MS", "--max-frames", str(frames),
            "--frame-error-count", str(10**9), "--noise", "counter", "--channel", "BSC"]
    flags = ["--ms-ternary", "1"]
    one, two = str(tmp_path / "one.txt"), str(tmp_path / "two.txt")
    p = subprocess.run(head + [one] + tail + flags, stdout=subprocess.PIPE, text=True, timeout=120, check=True)
    assert "Min-Sum Ternary: weight 1" in p.stdout and "NON-PARITY" in p.stdout
    subprocess.run(head + [two] + tail + flags + ["--devices", "0,0", "--comm", "shm"], stdout=subprocess.PIPE, text=True,
                   timeout=120, check=True)
    assert _file_rows(one) == _file_rows(py_file) == _file_rows(two)
    # the four refused combinations: non-zero exit, no file
    other = str(tmp_path / "other.txt")
    for extra in (["--ms-bits", "6"], ["--ms-schedule", "layered"], ["--ms-scale", "0.75"], ["--ms-offset", "0.5"]):
        p = subprocess.run(head + [other] + tail + flags + extra, stdout=subprocess.PIPE, text=True, timeout=120)
        assert p.returncode != 0 and "--ms-ternary" in p.stdout, extra
    p = subprocess.run(head + [other] + tail[:5] + flags, stdout=subprocess.PIPE, text=True, timeout=120)  # BP
    assert p.returncode != 0 and "--ms-ternary" in p.stdout
    p = subprocess.run(head + [other] + tail + ["--ms-ternary", "8"], stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode != 0 and "--ms-ternary" in p.stdout
    assert not os.path.exists(other)
