"""The typed batch call on the GPU (include/ldpc_amd.h, ldpc_hip_decode_batch_typed): float32, float16 and int8 LLRs and the
bit-packed decisions.  The yardstick is always decode_batch on the widened array W built here in numpy: every output equals
it bit for bit — iters, hard, bit_errors, llr_out and llr_in (which is W) as uint64.  The direct form of fixed-point layered
min-sum (kernels_layered_fixed_direct.hip), the conversion launch in front of every other decoder (kernels_convert.hip),
the packing launch behind all of them."""
import numpy as np
import pytest

import orc
from minsum_common import WANT, check_no_iteration, check_split_batch, dumped, same, write
from test_gpu_layered_min_sum import irregular_code

pytestmark = pytest.mark.gpu
ALL = WANT + ("llr_in",)
TYPES = ("float32", "float16", "int8")
# (msg_bits, app_bits, step, scale, offset); the last step is no power of two
DIRECT_SETTINGS = [(6, 8, 0.25, 0.8125, 0.0), (5, 7, 0.5, 0.75, 0.5), (6, 8, 0.3, 1.0, 0.0)]


def typed(llr, kind, step=None):
    """(the typed array, W): what a caller with such LLRs holds, and the binary64 array the call is defined to decode."""
    if kind == "int8":
        k = np.clip(np.rint(llr / step), -128, 127).astype(np.int8)
        return k, k.astype(np.float64) * step
    with np.errstate(over="ignore"):  # (a shortened column's 99999.9 is an infinity in binary16)
        t = llr.astype(kind)
    return t, t.astype(np.float64)


def same_all(r, y, what, rows=slice(None)):
    same(r, y, what, rows)
    assert np.array_equal(r["llr_in"].view(np.uint64), y["llr_in"][rows].view(np.uint64)), (what, "llr_in")


def pack(hard):
    """[n][nc] decision bytes -> [n][ceil(nc / 32)] words, bit c & 31 of word c >> 5."""
    n, nc = hard.shape
    padded = np.zeros((n, (nc + 31) // 32 * 32), np.uint8)
    padded[:, :nc] = hard
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4")


def _off(d):
    d.set_min_sum_layered_fixed(0)
    d.set_min_sum_quantization(0)
    d.set_min_sum_ternary(0)
    d.set_min_sum_schedule("flooding")
    d.set_fast_mode(0)
    d.set_min_sum_correction()


def _fixed_on(d, setting):
    q, p, step, s, o = setting
    _off(d)
    d.set_min_sum_layered_fixed(q, p, step)
    d.set_min_sum_correction(s, o)


def _pair(d, t, W, early, iters, decoding="BP_MS", want=ALL):
    """(the typed call on t, the yardstick on W)"""
    r = d.decode_batch_typed(t, early_term=early, iterations=iters, decoding=decoding, want=want)
    y = d.decode_batch(W, early_term=early, iterations=iters, decoding=decoding, want=ALL)
    return r, y


@pytest.fixture(scope="module")
def h_txt():
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    _off(d)
    return {"d": d, "llr": dumped(d, _off, "AWGN", -5.0, 48), "bsc": dumped(d, _off, "BSC", 0.2, 16)}


@pytest.fixture(scope="module")
def code70(tmp_path_factory):
    """70 columns, 35 check nodes of degree 4 (every column has degree 2): nc is no multiple of 4, so a frame's int8 row
    starts at every alignment, and no multiple of 32, so the last packed word is partly used."""
    import libldpc_amd
    nc = 70
    rows = [[c, (c + 1) % nc, (c + 7) % nc, (c + 8) % nc] for c in range(0, nc, 2)]
    path = write(tmp_path_factory.mktemp("codes") / "c70.txt", rows)
    d = libldpc_amd.HipDecoder(path)
    assert d.nc == 70 and d.layered_fixed_direct_lds_bytes() > 0
    _off(d)
    return {"d": d, "llr": dumped(d, _off, "AWGN", 1.0, 40), "path": path}


@pytest.mark.parametrize("kind", TYPES)
@pytest.mark.parametrize("setting", DIRECT_SETTINGS, ids=lambda s: "q%d_p%d_step%g_a%g_b%g" % s)
def test_direct_h_txt(h_txt, setting, kind):
    """Fixed-point layered min-sum reads the typed LLRs itself: 48 frames at -5 dB, early termination at 50 sweeps and none
    at 20."""
    d, llr = h_txt["d"], h_txt["llr"]
    _fixed_on(d, setting)
    assert d.decoder_choice(decoding="BP_MS") == "layered-fixed-min-sum"
    t, W = typed(llr, kind, setting[2])
    for early, iters in ((True, 50), (False, 20)):
        r, y = _pair(d, t, W, early, iters)
        same_all(r, y, (setting, kind, early))
        if early:
            converged, failed = (y["iters"] < 50) & (y["bit_errors"] == 0), y["bit_errors"] > 0
            print(setting, kind, "converged", int(converged.sum()), "failed", int(failed.sum()))
            # the frames exercise both ends, shown on the yardstick at the first setting (at (5, 7, 0.5) with scale 0.75 and
            # offset 0.5 none of the 48 converges at -5 dB, whatever decodes them)
            if setting == DIRECT_SETTINGS[0]:
                assert converged.any() and failed.any(), (int(converged.sum()), int(failed.sum()))
    _off(d)


def _small_shapes(d, llr, kind, setting=(6, 8, 0.25, 0.8125, 0.0)):
    _fixed_on(d, setting)
    t, W = typed(llr, kind, setting[2])
    r, y = _pair(d, t, W, True, 15)
    same_all(r, y, (kind, "whole"))
    for n in (1, 7):
        r = d.decode_batch_typed(t[:n], early_term=True, iterations=15, decoding="BP_MS", want=ALL)
        same_all(r, y, (kind, n), slice(0, n))
    # batches that start inside the caller's array: with nc no multiple of 4 an int8 row starts at other byte alignments
    for first in (1, 2, 3):
        r = d.decode_batch_typed(t[first:first + 5], early_term=False, iterations=6, decoding="BP_MS", want=ALL)
        yy = d.decode_batch(W[first:first + 5], early_term=False, iterations=6, decoding="BP_MS", want=ALL)
        same_all(r, yy, (kind, "from", first))
    one = check_split_batch(lambda part: d.decode_batch_typed(part, early_term=True, iterations=15, decoding="BP_MS", want=WANT), t, cut=9)
    same(one, y, (kind, "split"))
    for early in (True, False):
        z = d.decode_batch_typed(t[:3], early_term=early, iterations=0, decoding="BP_MS", want=ALL + ("hard_bits",))
        check_no_iteration(z)
        assert not z["hard_bits"].any()
        assert np.array_equal(z["llr_in"].view(np.uint64), W[:3].view(np.uint64))
    _off(d)


@pytest.mark.parametrize("kind", TYPES)
def test_direct_irregular_code(tmp_path, kind):
    """237 x 125, every check degree 2..8, nc % 64 != 0, punctured and shortened columns (an infinity in binary16)."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(irregular_code(str(tmp_path / "irregular.txt")))
    assert d.nc == 237
    llr = dumped(d, _off, "AWGN", 2.0, 16)
    _small_shapes(d, llr, kind)


@pytest.mark.parametrize("kind", TYPES)
def test_direct_nc70(code70, kind):
    _small_shapes(code70["d"], code70["llr"][:16], kind)


@pytest.mark.parametrize("bits", [(6, 8), (8, 10)])
def test_special_values(code70, bits):
    """One crafted frame per type: NaN, infinities, signed zeros, the largest finite value and a binary16 subnormal; int8's
    ends.  At 6-bit messages int8 values beyond +-31 saturate, at 8-bit ones -128 does."""
    d = code70["d"]
    step = 0.25
    _fixed_on(d, bits + (step, 1.0, 0.0))
    base = code70["llr"][:2].copy()
    for kind in ("float32", "float16"):
        fi = np.finfo(kind)
        t, _ = typed(base, kind)
        special = [np.nan, np.inf, -np.inf, 0.0, -0.0, fi.max, -fi.max, 2.0 ** -24, -(2.0 ** -24), fi.tiny, fi.smallest_subnormal]
        t[0, 3:3 + len(special)] = np.array(special, dtype=kind)
        t[1, -1] = np.nan
        W = t.astype(np.float64)
        assert np.isnan(W[0, 3]) and np.isinf(W[0, 4]) and np.signbit(W[0, 7]) and W[0, 7] == 0 and W[0, 10] == 2.0 ** -24
        r, y = _pair(d, t, W, False, 8)
        same_all(r, y, (bits, kind))
    k, _ = typed(base, "int8", step)
    k[0, :8] = [-128, -127, 127, 0, 126, -126, 31, -32]
    k[1, -4:] = [-128, 127, -127, 0]
    W = k.astype(np.float64) * step
    r, y = _pair(d, k, W, False, 8)
    same_all(r, y, (bits, "int8"))
    _off(d)


def _widen_cases():
    return {
        "bp": (lambda d: None, "BP", "llr"),
        "bp_ms": (lambda d: None, "BP_MS", "llr"),
        "corrected": (lambda d: d.set_min_sum_correction(0.8125, 0.25), "BP_MS", "llr"),
        "layered": (lambda d: d.set_min_sum_schedule("layered"), "BP_MS", "llr"),
        "quantized": (lambda d: d.set_min_sum_quantization(6, 0.25), "BP_MS", "llr"),
        "ternary": (lambda d: d.set_min_sum_ternary(2), "BP_MS", "bsc"),
        "fast1": (lambda d: d.set_fast_mode(1), "BP", "llr"),
    }


@pytest.mark.parametrize("case", sorted(_widen_cases()))
def test_widen_h_txt(h_txt, case):
    """Every other decoder takes W from the conversion launch: 16 frames of h.txt, float32 and float16 (and int8 where a
    fixed-point mode gives it a step), early termination on and off."""
    d = h_txt["d"]
    on, decoding, src = _widen_cases()[case]
    _off(d)
    on(d)
    llr = h_txt[src][:16]
    for kind in TYPES if case == "quantized" else TYPES[:2]:
        t, W = typed(llr, kind, 0.25)
        for early, iters in ((True, 30), (False, 10)):
            r, y = _pair(d, t, W, early, iters, decoding)
            same_all(r, y, (case, kind, early))
            if case != "ternary":  # (ternary min-sum decodes nothing on h.txt: include/ldpc_amd.h)
                assert y["iters"].max() > 0
    # float64 is decode_batch itself
    r, y = _pair(d, llr, llr, True, 30, decoding)
    same_all(r, y, (case, "float64"))
    _off(d)


def test_widen_8k_code(h8k_file):
    """The register-resident decoder: 8 frames, float32, both decodings."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(h8k_file)
    assert d.residency == "registers"
    llr = dumped(d, _off, "AWGN", 1.4, 8)
    t, W = typed(llr, "float32")
    for decoding in ("BP", "BP_MS"):
        r, y = _pair(d, t, W, True, 25, decoding)
        same_all(r, y, decoding)
    # ... and the direct form at four frames per CU
    _fixed_on(d, (6, 7, 0.25, 0.8125, 0.0))
    for kind in ("float32", "int8"):
        t, W = typed(llr, kind, 0.25)
        r, y = _pair(d, t, W, True, 25)
        same_all(r, y, ("direct", kind))
        assert ((y["iters"] < 25) & (y["bit_errors"] == 0)).any()
    _off(d)


def test_hard_bits(h_txt, code70):
    """hard_bits is the packed `hard` on the direct path, the widen path, with no iteration and without `hard` asked for; in
    numpy buffers and in device tensors."""
    import torch
    for c, nc in ((h_txt, 1152), (code70, 70)):
        d, llr = c["d"], c["llr"][:12]
        assert d.nc == nc
        # direct
        _fixed_on(d, (6, 8, 0.25, 0.8125, 0.0))
        t, W = typed(llr, "int8", 0.25)
        y = d.decode_batch(W, early_term=True, iterations=20, decoding="BP_MS", want=ALL)
        assert y["hard"].any()
        r = d.decode_batch_typed(t, early_term=True, iterations=20, decoding="BP_MS", want=ALL + ("hard_bits",))
        same_all(r, y, "direct")
        assert r["hard_bits"].dtype == np.uint32 and r["hard_bits"].shape == (12, (nc + 31) // 32)
        assert np.array_equal(r["hard_bits"], pack(y["hard"]))
        # ... asked for without `hard`, the buffer pre-filled: the unused high bits come back zero
        mine = np.full((12, (nc + 31) // 32), 0xFFFFFFFF, np.uint32)
        r = d.decode_batch_typed(t, early_term=True, iterations=20, decoding="BP_MS", want=("iters",), out={"hard_bits": mine})
        assert r["hard_bits"] is mine and "hard" not in r and np.array_equal(mine, pack(y["hard"]))
        assert np.array_equal(r["iters"], y["iters"])
        # no iteration
        mine[:] = 0xFFFFFFFF
        d.decode_batch_typed(t, early_term=True, iterations=0, decoding="BP_MS", want=(), out={"hard_bits": mine})
        assert not mine.any()
        # device tensors for the input, the outputs and hard_bits
        dev = torch.device("cuda", 0)
        out = {"iters": torch.zeros(12, dtype=torch.int32, device=dev), "hard": torch.zeros((12, nc), dtype=torch.uint8, device=dev),
               "hard_bits": torch.full((12, (nc + 31) // 32), -1, dtype=torch.int32, device=dev)}
        d.decode_batch_typed(torch.from_numpy(t).to(dev), early_term=True, iterations=20, decoding="BP_MS", want=(), out=out)
        torch.cuda.synchronize()
        assert np.array_equal(out["hard"].cpu().numpy(), y["hard"])
        assert np.array_equal(out["hard_bits"].cpu().numpy().view(np.uint32), pack(y["hard"]))
        assert np.array_equal(out["iters"].cpu().numpy().view(np.uint32), y["iters"])
        # widen path: sum-product on float32 (its small batches deliver after the first launch), float64 too
        _off(d)
        t, W = typed(llr, "float32")
        y = d.decode_batch(W, early_term=True, iterations=20, decoding="BP", want=ALL)
        r = d.decode_batch_typed(t, early_term=True, iterations=20, decoding="BP", want=("hard_bits",))
        assert np.array_equal(r["hard_bits"], pack(y["hard"]))
        r = d.decode_batch_typed(W, early_term=True, iterations=20, decoding="BP", want=ALL + ("hard_bits",))
        same_all(r, y, "float64")
        assert np.array_equal(r["hard_bits"], pack(y["hard"]))
        bits = torch.full((12, (nc + 31) // 32), -1, dtype=torch.int32, device=dev)
        d.decode_batch_typed(torch.from_numpy(t).to(dev), early_term=False, iterations=5, decoding="BP_MS", want=(), out={"hard_bits": bits})
        torch.cuda.synchronize()
        y = d.decode_batch(W, early_term=False, iterations=5, decoding="BP_MS", want=ALL)
        assert np.array_equal(bits.cpu().numpy().view(np.uint32), pack(y["hard"]))


def test_nothing_sticks(h_txt):
    """decode_batch after typed calls returns what it returned before them, with the mode on and off."""
    d, llr = h_txt["d"], h_txt["llr"][:16]
    _off(d)
    before_bp = d.decode_batch(llr, decoding="BP", want=ALL)
    before_ms = d.decode_batch(llr, decoding="BP_MS", want=ALL)
    _fixed_on(d, (6, 8, 0.25, 0.8125, 0.0))
    before_lf = d.decode_batch(llr, decoding="BP_MS", want=ALL)
    for kind in TYPES:
        t, _ = typed(llr, kind, 0.25)
        d.decode_batch_typed(t, decoding="BP_MS", want=ALL + ("hard_bits",))
        if kind != "int8":
            d.decode_batch_typed(t, decoding="BP", want=ALL + ("hard_bits",))
    assert d.min_sum_layered_fixed == (6, 8, 0.25)
    same_all(d.decode_batch(llr, decoding="BP_MS", want=ALL), before_lf, "fixed-point layered")
    same_all(d.decode_batch(llr, decoding="BP", want=ALL), before_bp, "BP beside the mode")
    _off(d)
    same_all(d.decode_batch(llr, decoding="BP_MS", want=ALL), before_ms, "BP_MS")
    same_all(d.decode_batch(llr, decoding="BP", want=ALL), before_bp, "BP")
