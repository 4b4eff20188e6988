"""The typed batch call (include/ldpc_amd.h, ldpc_hip_decode_batch_typed) without a GPU: the exported symbols, what the call
refuses before it touches a device, the LDS figure of the direct form of fixed-point layered min-sum, and the arithmetic fact
the int8 path rests on: quantizing fl(k * step) gives k back."""
import ctypes as ct
import os

import numpy as np
import pytest

import orc
from minsum_common import write

NAME = b"ldpc_hip_decode_batch_typed"
F64, F32, F16, I8 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


def _call(lib, d, decoding, llr_type, n=0, llr=None):
    from libldpc_amd.binding import decoder_param
    return lib.ldpc_hip_decode_batch_typed(d.ctx, decoder_param(True, 50, decoding.encode()), n, llr, llr_type, None, None, None)


def test_symbols_and_signatures(lib):
    from libldpc_amd.binding import decoder_param, ldpc_hip_out
    f = lib.ldpc_hip_decode_batch_typed
    assert f.restype is ct.c_int
    assert f.argtypes == [ct.c_void_p, decoder_param, ct.c_uint64, ct.c_void_p, ct.c_int, ct.POINTER(ldpc_hip_out), ct.c_void_p,
                          ct.c_void_p]
    g = lib.ldpc_hip_layered_fixed_direct_lds_bytes
    assert g.restype is ct.c_int64 and g.argtypes == [ct.c_void_p]
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_decode_batch_typed(ldpc_hip_ctx *ctx, decoder_param dec, uint64_t n, const void *llr_in, int llr_type, "
            "const ldpc_hip_out *out, uint32_t *hard_bits, void *hip_stream);") in flat
    assert "int64_t ldpc_hip_layered_fixed_direct_lds_bytes(const ldpc_hip_ctx *ctx);" in flat
    for name, value in (("F64", 0), ("F32", 1), ("F16", 2), ("I8", 3)):
        assert f"LDPC_HIP_LLR_{name} = {value}" in flat


def test_unknown_type(lib):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    for t in (4, -1, 1000):
        for n in (0, 3):  # refused before the frame count or the pointer is looked at
            assert _call(lib, d, "BP", t, n) == -1 and NAME in lib.ldpc_hip_last_error(), (t, n)
    for t in (F64, F32, F16):
        assert _call(lib, d, "BP", t) == 0 and _call(lib, d, "BP_MS", t) == 0  # n == 0: nothing to do, no GPU


def test_int8_needs_a_fixed_point_mode(lib):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    k = np.zeros((2, d.nc), np.int8)

    def refused(decoding, what):
        for n, p in ((0, None), (2, k.ctypes.data)):
            assert _call(lib, d, decoding, I8, n, p) == -1 and NAME in lib.ldpc_hip_last_error(), (what, n)

    refused("BP", "sum-product")
    refused("BP_MS", "no fixed-point mode on")
    d.set_min_sum_ternary(2)
    refused("BP_MS", "ternary")
    d.set_min_sum_ternary(0)
    d.set_min_sum_schedule("layered")
    refused("BP_MS", "plain layered")
    d.set_min_sum_schedule("flooding")
    # accepted once quantization or fixed-point layered is on (n == 0 needs no GPU); "BP" stays refused
    d.set_min_sum_quantization(6, 0.25)
    assert _call(lib, d, "BP_MS", I8) == 0
    refused("BP", "sum-product beside quantization")
    d.set_min_sum_quantization(0)
    refused("BP_MS", "quantization off again")
    d.set_min_sum_layered_fixed(6, 8, 0.25)
    assert _call(lib, d, "BP_MS", I8) == 0
    refused("BP", "sum-product beside fixed-point layered")
    d.set_min_sum_layered_fixed(0)
    refused("BP_MS", "fixed-point layered off again")
    # a null input with frames to decode is an error, not a crash
    assert _call(lib, d, "BP", F32, 2, None) == -1 and NAME in lib.ldpc_hip_last_error()


def _direct_bytes(code):
    """round4(2 nc) + 4 R + 128 rounded up to 16, R from the oracle's restatement of the layered plan."""
    n, step_of = code.layer_steps()
    slots = int(((np.bincount(step_of, minlength=n) + 1) // 2 * 2).sum())
    return ((2 * code.nc + 3) // 4 * 4 + 4 * slots + 128 + 15) // 16 * 16


def test_direct_lds_bytes(lib, tmp_path, h8k_file):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    h = d.layered_fixed_direct_lds_bytes()
    assert h == 6528 == _direct_bytes(orc.Code(orc.H_TXT))
    assert 25 * 6528 <= 160 * 1024 < 26 * 6528  # 25 frames per CU (17 with the binary64 staging area)
    assert h < d.layered_fixed_lds_bytes() == 9344
    d8 = libldpc_amd.HipDecoder(h8k_file)
    b8 = d8.layered_fixed_direct_lds_bytes()
    assert b8 == _direct_bytes(orc.Code(h8k_file)) and 4 * b8 <= 160 * 1024  # four frames per CU (two staged)
    small = write(tmp_path / "small.txt", [[0, 1], [1, 2], [2, 3], [3, 0], [0, 2], [1, 3], [0, 1], [2, 3]])
    ds = libldpc_amd.HipDecoder(small)
    assert ds.layered_fixed_direct_lds_bytes() == _direct_bytes(orc.Code(small))
    cases = {
        "isolated_column": [[0, 1, 2], [2, 3, 5], [5, 6, 0], [1, 3, 6]],  # column 4 has no edge
        "degree9_row": [[0, 1, 2], [2, 3, 4], [4, 5, 0], [1, 3, 5]] + [list(range(9))],
    }
    for name, rows in cases.items():
        dd = libldpc_amd.HipDecoder(write(tmp_path / f"{name}.txt", rows))
        assert dd.layered_fixed_direct_lds_bytes() == -1, name


def test_quantizing_an_int8_step_multiple_gives_the_int8_back():
    """rint(fl(fl(k * D) * fl(1 / D))) == k for all 256 int8 k and 200 011 steps D in [2^-20, 2^20] (the setters' range): the
    two roundings are off by less than 2^-51 relative, far from the half that would move rint.  So the direct path's
    clamp(k, -Qmax, +Qmax) is the contract's quantizer applied to W = fl(k * D)."""
    k = np.arange(-128, 128, dtype=np.float64)[:, None]
    rng = np.random.default_rng(11)
    steps = np.concatenate((2.0 ** np.arange(-20, 21), [0.3, 0.1, 1.0 / 3.0, 0.7, 2.0 ** 20 * (1 - 2.0 ** -53), 2.0 ** -20 * (1 + 2.0 ** -52)],
                            2.0 ** rng.uniform(-20, 20, 200011 - 41 - 6)))
    assert steps.size == 200011 and steps.min() >= 2.0 ** -20 and steps.max() <= 2.0 ** 20
    bad = 0
    for part in np.array_split(steps, 16):
        inv = 1.0 / part
        bad += int((np.rint((k * part) * inv) != k).sum())
    assert bad == 0


def test_binding_refuses_other_dtypes(lib):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    for dt in (np.int16, np.uint8, np.int32, np.complex64):
        with pytest.raises(TypeError, match="decode_batch_typed"):
            d.decode_batch_typed(np.zeros((1, d.nc), dt))
    assert set(libldpc_amd.HipDecoder.OUT_SPEC) == {"iters", "bit_errors", "hard", "llr_out", "llr_in", "codeword"}


def test_kernel_resources(lib):
    """The direct instantiations use no scratch, and the staged ones still are the two they were."""
    from libldpc_amd import build
    direct = build.kernel_resources("kernels_layered_fixed_direct.hip")
    assert direct and len(direct) == 2  # WANT_LLR or not
    for name, r in direct.items():
        assert "decode_layered_fixed_direct_kernel" in name
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
    staged = build.kernel_resources("kernels_layered_fixed.hip")
    assert staged and len(staged) == 2
    for name, r in staged.items():
        assert r["VGPRs"] == 63 and r["ScratchSize [bytes/lane]"] == 0 and r["LDS Size [bytes/block]"] == 0, (name, r)
