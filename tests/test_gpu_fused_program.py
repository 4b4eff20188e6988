"""The kernel of a compile-time wave program (kernels_fused.hip, decode_fused_prog; libldpc_amd/csrc/fused_program.hpp) on the
code that has one, the reference's n = 1024 test code: bit for bit against the det-mode oracle over iteration counts, bit
errors and hard decisions, no frame excluded.  tests/test_gpu_random_codes.py keeps covering the interpreted plans."""
import ctypes as ct

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
OUT = ("iters", "bit_errors", "hard")
# seed 0 at -4 dB: frame 1216 is the first that runs all 50 iterations (none of the first 200 does)
N_HEADLINE = 1280


@pytest.fixture(scope="module")
def dec():
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    assert d.fused_program() >= 0  # otherwise everything below would pass on the interpreter
    assert d.decode_stages() == ["ratio-first", "list-chain"]
    return d


@pytest.fixture(scope="module")
def code():
    return orc.Code(orc.H_TXT)


@pytest.fixture(scope="module")
def headline_ref(code):
    return code.run_frames("AWGN", -4.0, seed=0, count=N_HEADLINE, early_term=True, iters=50, math=orc.MATH_DET)


def check(dec, ref, ch, x, count, iters, skip=0):
    dec.stream_begin(ch, 0, x)
    if skip:
        dec.stream_skip(skip)
    r = dec.stream_decode(count, early_term=True, iterations=iters, want=OUT)
    for k in OUT:
        assert np.array_equal(r[k], ref[k].astype(r[k].dtype)), (ch, x, iters, k, np.nonzero(r["iters"] != ref["iters"])[0][:8])


def test_headline_point(dec, headline_ref):
    """AWGN at -4 dB, 50 iterations, early termination: frames end at every pass count up to the limit."""
    assert (headline_ref["iters"] == 50).any() and (headline_ref["iters"] < 50).any()
    check(dec, headline_ref, "AWGN", -4.0, N_HEADLINE, 50)


@pytest.mark.parametrize("iters", [0, 1, 2])
def test_iteration_limits(dec, code, iters):
    """The loop's exits at the limit (0: no fused launch at all, the whole decode is one LLR-domain launch)."""
    ref = code.run_frames("AWGN", -4.0, seed=0, count=200, early_term=True, iters=iters, math=orc.MATH_DET)
    check(dec, ref, "AWGN", -4.0, 200, iters)


@pytest.mark.parametrize("x", [6.0, 14.0])
def test_frames_that_leave_the_box(dec, code, x):
    """High SNR: frames escape the ratio form's box (at 14 dB all of them), so the kernel writes the redo list and the later
    launches decode from it."""
    orc.ratio_stats(reset=True)
    ref = code.run_frames("AWGN", x, seed=0, count=64, early_term=True, iters=25, math=orc.MATH_DET)
    assert orc.ratio_stats()[1] > 0
    check(dec, ref, "AWGN", x, 64, 25)


def test_bsc(dec, code):
    ref = code.run_frames("BSC", 0.24, seed=0, count=64, early_term=True, iters=50, math=orc.MATH_DET)
    check(dec, ref, "BSC", 0.24, 64, 50)


def test_skipped_frames(dec, code):
    ref = code.run_frames("AWGN", -4.0, seed=0, skip=3, count=7, early_term=True, iters=50, math=orc.MATH_DET)
    check(dec, ref, "AWGN", -4.0, 7, 50, skip=3)


def test_given_llrs(dec, headline_ref):
    """Input LLRs handed in: the batch call (the program's kernel) and the reference's C ABI, decode() on one frame (which
    asks for the output LLRs: the interpreter's small instantiation, delivered early), agree on the iteration counts."""
    import libldpc_amd
    from libldpc_amd.binding import decoder_param
    dec.stream_begin("AWGN", 0, -4.0)
    s = dec.stream_decode(8, want=("llr_in", "iters"))
    assert np.array_equal(s["iters"], headline_ref["iters"][:8])
    b = dec.decode_batch(s["llr_in"], want=("iters", "hard"))
    assert np.array_equal(b["iters"], s["iters"])
    assert np.array_equal(b["hard"], headline_ref["hard"][:8])
    lib = ct.CDLL(libldpc_amd.LIB_PATH)
    n, m, nct, mct = (ct.c_int(0) for _ in range(4))
    lib.ldpc_setup(orc.H_TXT.encode(), b"", ct.byref(n), ct.byref(m), ct.byref(nct), ct.byref(mct))
    tx = ~(s["llr_in"] == 0.0).all(axis=0)  # transmitted positions (punctured inputs are exactly 0.0)
    assert int(tx.sum()) == nct.value
    frames = np.ascontiguousarray(s["llr_in"][:, tx])
    lib.decode.restype = ct.c_int
    lib.decode.argtypes = [decoder_param, ct.c_void_p, ct.c_void_p]
    vout = (ct.c_double * nct.value)()
    its = [lib.decode(decoder_param(True, 50, b"BP"), frames[f].ctypes.data, vout) for f in range(8)]
    assert np.array_equal(np.array(its), s["iters"])
