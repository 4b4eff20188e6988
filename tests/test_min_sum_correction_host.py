"""Corrected min-sum (include/ldpc_amd.h, ldpc_hip_set_min_sum_correction) without a GPU: the numpy mirror
(tests/minsum_ref.py) against the oracle's plain min-sum, the C ABI's parameter checks and the CLI's."""
import math
import os
import subprocess

import numpy as np
import pytest

import orc
from minsum_ref import MinSumMirror, correct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def h_mirror():
    code = orc.Code(orc.H_TXT)
    return code, MinSumMirror(code)


def _golden_llrs(golden_frames):
    keys = [k for k in golden_frames.files if k.endswith("/llr_in") and "bec" not in k]
    return np.concatenate([golden_frames[k] for k in keys])


@pytest.mark.parametrize("early,iters", [(True, 50), (False, 50), (False, 7)])
def test_mirror_at_identity_is_the_oracles_min_sum(h_mirror, golden_frames, early, iters):
    """At (1, 0) the mirror is plain BP_MS: LLR-out, hard bits and iteration counts equal the oracle's, bit for bit, on
    the golden h.txt frames (AWGN and BSC, some of which do not converge)."""
    code, mir = h_mirror
    llr = _golden_llrs(golden_frames)
    got = mir.decode(llr, 1.0, 0.0, early_term=early, iterations=iters)
    fails = 0
    for f in range(llr.shape[0]):
        it, out, hard = code.decode(llr[f], min_sum=True, early_term=early, iters=iters)
        assert got["iters"][f] == it, f
        assert np.array_equal(got["hard"][f], hard), f
        assert np.array_equal(got["llr_out"][f].view(np.uint64), out.view(np.uint64)), f
        fails += int(hard.any())
    assert fails > 0  # the set holds frames that do not decode


def test_mirror_correction_changes_the_decode(h_mirror, golden_frames):
    code, mir = h_mirror
    llr = _golden_llrs(golden_frames)
    plain = mir.decode(llr, 1.0, 0.0, early_term=False, iterations=10)
    nms = mir.decode(llr, 0.75, 0.0, early_term=False, iterations=10)
    assert not np.array_equal(plain["llr_out"], nms["llr_out"])


def test_correction_function():
    m = np.array([0.0, 0.1, 0.25, 0.5, 1.0, 3.0, 1e300])
    np.testing.assert_array_equal(correct(m, 1.0, 0.0), m)
    r = correct(m, 0.75, 0.25)
    assert r[0] == 0.0 and not np.signbit(r[0]) and r[1] == 0.0 and not np.signbit(r[1])
    assert r[4] == 0.5 and r[5] == 2.0
    # no fused multiply-add: fl(fl(a * m) - b)
    a, x, b = 0.8125, 0.1 + 2 ** -40, 0.0812
    assert correct(np.array([x]), a, b)[0] == (a * x) - b


def test_set_min_sum_correction_validates():
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)  # creating a context touches no GPU
    L = d.lib
    bad = [(0.0, 0.0), (-0.5, 0.0), (1.0000001, 0.0), (1.5, 0.0), (0.75, -0.25), (0.75, 2e6), (math.nan, 0.0),
           (0.75, math.nan), (math.inf, 0.0), (0.75, math.inf), (-math.inf, 0.0)]
    for s, o in bad:
        assert L.ldpc_hip_set_min_sum_correction(d.ctx, s, o) == -1, (s, o)
        assert b"set_min_sum_correction" in L.ldpc_hip_last_error()
        with pytest.raises(RuntimeError):
            d.set_min_sum_correction(s, o)
    for s, o in [(1.0, 0.0), (0.75, 0.25), (1e-9, 0.0), (1.0, 1e6), (0.8125, 0.0)]:
        assert L.ldpc_hip_set_min_sum_correction(d.ctx, s, o) == 0, (s, o)
    d.set_min_sum_correction()
    d.close()


CLI = os.path.join(ROOT, "libldpc_amd", "ldpcsim")


@pytest.mark.parametrize("extra", [
    ["--decoding", "BP", "--ms-scale", "0.75"],
    ["--ms-offset", "0.5"],                          # the default decoding is BP
    ["--decoding", "BP_MS", "--ms-scale", "0"],
    ["--decoding", "BP_MS", "--ms-scale", "1.5"],
    ["--decoding", "BP_MS", "--ms-scale", "nan"],
    ["--decoding", "BP_MS", "--ms-offset", "-1"],
    ["--decoding", "BP_MS", "--ms-offset", "inf"],
    ["--decoding", "BP_MS", "--ms-scale", "abc"],
])
def test_cli_rejects_bad_corrections(tmp_path, extra):
    """A parse error: non-zero exit before any GPU is touched, and no result file."""
    out = tmp_path / "out.txt"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")  # a GPU is never needed to refuse these
    p = subprocess.run([CLI, orc.H_TXT, str(out), "-4", "-4", "1", "--max-frames", "10"] + extra, capture_output=True,
                       text=True, timeout=60, env=env)
    assert p.returncode != 0, p.stdout
    assert "Usage" in p.stdout
    assert not out.exists()
