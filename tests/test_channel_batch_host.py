"""ldpc_hip_channel_batch (include/ldpc_amd.h) without a GPU: the exported symbol and its prototype, everything the call refuses
before it touches a device, the binding's own checks, the properties of the numpy mirror (tests/channel_ref.py) that
test_gpu_channel_batch.py relies on, and the compile-time resources of kernels_channel.hip."""
import ctypes as ct
import os

import numpy as np
import pytest

import channel_ref
import generator_codes as gc
import orc

U8, PACKED32 = 0, 1
F64, F32, F16, I8 = 0, 1, 2, 3
AWGN, BSC, BEC = 1, 2, 3
ENTRY = b"ldpc_hip_channel_batch"


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    return gc.write_pair(tmp_path_factory.mktemp("channel"), "s129x150t5")


def test_symbol_and_signature(lib):
    from libldpc_amd.binding import ldpc_hip_channel
    vp, u64, i32 = ct.c_void_p, ct.c_uint64, ct.c_int
    assert lib.ldpc_hip_channel_batch.argtypes == [vp, ct.POINTER(ldpc_hip_channel), u64, vp, i32, vp, vp, vp]
    assert lib.ldpc_hip_channel_batch.restype == i32
    assert [(n, t) for n, t in ldpc_hip_channel._fields_] == [
        ("channel", i32), ("x", ct.c_double), ("seed", u64), ("first_frame", u64), ("bits_per_symbol", i32), ("llr_type", i32),
        ("q_bits", i32), ("step", ct.c_double)]
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_channel_batch(ldpc_hip_ctx *ctx, const ldpc_hip_channel *ch, uint64_t n, const void *codeword, "
            "int codeword_format, void *llr, double *received, void *hip_stream);") in flat
    assert "} ldpc_hip_channel;" in flat
    assert "ldpc_hip_encode_batch -> ldpc_hip_channel_batch -> ldpc_hip_decode_batch_typed" in flat
    assert "the caller's modulation and channel" not in flat


def test_refusals_come_before_the_gpu(lib, pair):
    """No GPU here: a call that reached the device would fail with another message, or not at all."""
    import libldpc_amd
    from libldpc_amd.binding import ldpc_hip_channel
    d = libldpc_amd.HipDecoder(*pair)
    cw = np.zeros((2, d.nc), np.uint8)
    llr = np.zeros((2, d.nc), np.float64)
    rec = np.zeros((2, d.nct), np.float64)
    err = lib.ldpc_hip_last_error

    def spec(channel=AWGN, x=2.0, m=1, llr_type=F64, q_bits=0, step=1.0):
        return ldpc_hip_channel(channel, x, 5, 0, m, llr_type, q_bits, step)

    def call(n, ch, fmt=U8, out=llr.ctypes.data, received=rec.ctypes.data, src=cw.ctypes.data):
        return lib.ldpc_hip_channel_batch(d.ctx, ct.byref(ch) if ch is not None else None, n, src, fmt, out, received, None)

    nan, inf = float("nan"), float("inf")
    refused = {
        "null ch": dict(ch=None),
        "channel 0": dict(ch=spec(channel=0)), "the BEC": dict(ch=spec(channel=BEC, x=0.1)), "channel -1": dict(ch=spec(channel=-1)),
        "format 2": dict(ch=spec(), fmt=2), "format -1": dict(ch=spec(), fmt=-1),
        "type 4": dict(ch=spec(llr_type=4)), "type -1": dict(ch=spec(llr_type=-1)),
        "m 0": dict(ch=spec(m=0)), "m 5": dict(ch=spec(m=5)), "m -1": dict(ch=spec(m=-1)),
        "BSC m 2": dict(ch=spec(channel=BSC, x=0.1, m=2)),
        "AWGN nan": dict(ch=spec(x=nan)), "AWGN inf": dict(ch=spec(x=inf)), "AWGN -inf": dict(ch=spec(x=-inf)),
        "BSC 0": dict(ch=spec(channel=BSC, x=0.0)), "BSC 1": dict(ch=spec(channel=BSC, x=1.0)),
        "BSC -0.1": dict(ch=spec(channel=BSC, x=-0.1)), "BSC nan": dict(ch=spec(channel=BSC, x=nan)),
        "q_bits 1": dict(ch=spec(llr_type=I8, q_bits=1, step=0.25)), "q_bits 9": dict(ch=spec(llr_type=I8, q_bits=9, step=0.25)),
        "q_bits 0": dict(ch=spec(llr_type=I8, q_bits=0, step=0.25)),
        "step 0": dict(ch=spec(llr_type=I8, q_bits=6, step=0.0)), "step nan": dict(ch=spec(llr_type=I8, q_bits=6, step=nan)),
        "step small": dict(ch=spec(llr_type=I8, q_bits=6, step=2.0**-21)), "step large": dict(ch=spec(llr_type=I8, q_bits=6, step=2.0**21)),
        "step negative": dict(ch=spec(llr_type=I8, q_bits=6, step=-0.25)),
    }
    for n in (0, 2):
        for what, kw in refused.items():
            assert call(n, **kw) == -1 and ENTRY in err(), (n, what, err())
    # both outputs NULL is refused with frames to work on only
    assert call(2, spec(), out=None, received=None) == -1 and ENTRY in err()
    assert call(0, spec(), out=None, received=None) == 0
    # q_bits and step are looked at for int8 alone
    for t in (F64, F32, F16):
        assert call(0, spec(llr_type=t, q_bits=99, step=nan)) == 0
    # after the checks n == 0 returns 0 (no GPU needed): every channel, format, type and m, with and without buffers
    for fmt in (U8, PACKED32):
        for t in (F64, F32, F16, I8):
            for m in (1, 2, 3, 4):
                assert call(0, spec(m=m, llr_type=t, q_bits=6, step=0.25), fmt) == 0, (fmt, t, m)
            assert call(0, spec(channel=BSC, x=0.05, llr_type=t, q_bits=2, step=2.0**20), fmt, None, None, None) == 0
    for t, dt in (("float64", np.float64), ("float32", np.float32), ("float16", np.float16), ("int8", np.int8)):
        r = d.channel_batch(np.zeros((0, d.nc), np.uint8), "AWGN", 1.0, bits_per_symbol=3, llr=t, q_bits=6, step=0.25,
                            want=("llr", "received"))
        assert r["llr"].shape == (0, d.nc) and r["llr"].dtype == dt
        assert r["received"].shape == (0, -(-d.nct // 3)) and r["received"].dtype == np.float64
    assert d.channel_batch(None, "BSC", 0.1, frames=0)["llr"].shape == (0, d.nc)
    with pytest.raises(RuntimeError, match="ldpc_hip_channel_batch"):
        d.channel_batch(np.zeros((0, d.nc), np.uint8), "BEC", 0.1)


def test_binding_refuses_other_dtypes_and_shapes(lib, pair):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(*pair)
    for dt in (np.int8, np.int32, np.uint16, np.uint64, np.float32, np.bool_):
        with pytest.raises(TypeError, match="channel_batch"):
            d.channel_batch(np.zeros((1, d.nc), dt), "AWGN", 1.0)
    with pytest.raises(ValueError, match="channel_batch"):
        d.channel_batch(np.zeros((1, d.nc + 1), np.uint8), "AWGN", 1.0)
    with pytest.raises(ValueError, match="channel_batch"):
        d.channel_batch(np.zeros((1, d.nc), np.uint32), "AWGN", 1.0)  # packed rows are ceil(nc / 32) words
    with pytest.raises(ValueError, match="channel_batch"):
        d.channel_batch(np.zeros(d.nc, np.uint8), "AWGN", 1.0)
    with pytest.raises(ValueError, match="frames"):
        d.channel_batch(None, "AWGN", 1.0)
    with pytest.raises(ValueError, match="frames"):
        d.channel_batch(np.zeros((0, d.nc), np.uint8), "AWGN", 1.0, frames=3)
    with pytest.raises(TypeError, match="channel_batch"):
        d.channel_batch(np.zeros((0, d.nc), np.uint8), "AWGN", 1.0, llr="int16")
    with pytest.raises(KeyError):
        d.channel_batch(np.zeros((0, d.nc), np.uint8), "AWGN", 1.0, want=("hard",))
    # buffers the caller passes: their dtype and shape are those of the call
    with pytest.raises(TypeError, match="llr"):
        d.channel_batch(np.zeros((0, d.nc), np.uint8), "AWGN", 1.0, llr="float32", want=(), out={"llr": np.zeros((0, d.nc), np.float64)})
    with pytest.raises(ValueError, match="llr"):
        d.channel_batch(np.zeros((2, d.nc), np.uint8), "AWGN", 1.0, want=(), out={"llr": np.zeros((1, d.nc), np.float64)})
    with pytest.raises(TypeError, match="received"):
        d.channel_batch(np.zeros((0, d.nc), np.uint8), "AWGN", 1.0, want=(), out={"received": np.zeros((0, d.nct), np.float32)})
    with pytest.raises(ValueError, match="received"):  # m = 2: ceil(nct / 2) symbols
        d.channel_batch(np.zeros((0, d.nc), np.uint8), "AWGN", 1.0, bits_per_symbol=2, want=(), out={"received": np.zeros((0, d.nct), np.float64)})


def test_levels_have_unit_mean_energy():
    for m in (1, 2, 3, 4):
        lv = channel_ref.levels(m)
        assert lv.shape == (1 << m,) and lv.dtype == np.float64
        assert abs(float(np.mean(lv * lv)) - 1.0) <= 1e-15, m
        assert np.all(np.diff(lv) < 0) and np.array_equal(lv, -lv[::-1])  # descending, symmetric
    assert np.array_equal(channel_ref.levels(1), [1.0, -1.0])  # label 0 -> +1: binary signalling is the m = 1 table


def test_gray_inverse_round_trips():
    for m in (1, 2, 3, 4):
        g = np.arange(1 << m)
        j = channel_ref.gray_inverse(g)
        assert np.array_equal(channel_ref.gray(j), g) and np.array_equal(np.sort(j), g), m
        assert np.array_equal(channel_ref.gray_inverse(channel_ref.gray(g)), g), m
        lab = channel_ref.gray(g)
        assert all(bin(int(a ^ b)).count("1") == 1 for a, b in zip(lab[:-1], lab[1:])), m  # neighbours differ in one bit
    # labels(): the first bit of a symbol is the most significant, padding bits count as 0
    bits = np.array([[1, 0, 1, 1, 0, 1, 1]])
    assert np.array_equal(channel_ref.labels(3, bits), [[0b101, 0b101, 0b100]])
    assert np.array_equal(channel_ref.labels(2, bits), [[0b10, 0b11, 0b01, 0b10]])
    assert np.array_equal(channel_ref.labels(1, bits), bits)


def test_max_log_at_one_bit_is_the_binary_rule():
    """The contract special-cases m = 1 as (2 y) / sigma2; the max-log form (D1 - D0) / (2 sigma2) over the levels {+1, -1} is
    ((y + 1)^2 - (y - 1)^2) / (2 sigma2) = 4 y / (2 sigma2): the same value up to the rounding of the two squares, each within
    2^-53 of at most (|y| + 1)^2.  Relative to 4 |y| that is below 2^-52 (|y| + 1)^2 / (4 |y|): under 1e-12 wherever
    |y| >= 1e-3 and |y| <= 8, the range checked here (sigma2 scales both forms alike)."""
    rng = np.random.default_rng(1)
    y = np.concatenate([rng.uniform(-8, 8, 4000), np.linspace(-8, 8, 1601), [1e-3, -1e-3, 1.0, -1.0]])
    y = y[np.abs(y) >= 1e-3]
    for x in (-4.0, 0.0, 3.0, 9.5):
        sigma2, _ = channel_ref.awgn_params(x)
        rule = channel_ref.demap(1, y, sigma2)[..., 0]
        max_log = channel_ref.demap_max_log(1, y, sigma2)[..., 0]
        assert np.array_equal(rule, (2 * y) / sigma2)
        assert np.all(np.abs(max_log - rule) <= 1e-12 * np.abs(rule)), x
        assert np.array_equal(np.sign(max_log), np.sign(rule))


def test_quantizer_and_conversions_of_the_mirror():
    v = np.array([0.0, -0.0, 0.124, 0.125, 0.375, -0.375, 7.75, 7.9, -7.9, 99999.9, -np.inf, np.inf, np.nan])
    assert np.array_equal(channel_ref.quantize(v, 6, 0.25), [0, 0, 0, 0, 2, -2, 31, 31, -31, 31, -31, 31, 0])  # ties to even
    assert np.array_equal(channel_ref.quantize(v, 4, 1.0), [0, 0, 0, 0, 0, 0, 7, 7, -7, 7, -7, 7, 0])
    assert np.isposinf(channel_ref.convert(np.array([99999.9]), "float16")[0])
    assert channel_ref.convert(np.array([99999.9]), "float32")[0] == np.float32(99999.9)


def test_kernel_resources(lib):
    """kernels_channel.hip: an instantiation per (m, element type) for AWGN and per element type for the BSC; none uses
    scratch, spills a register or takes more than 128 VGPRs."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_channel.hip")
    assert res
    assert len(res) == 20 and all("channel_kernel" in k for k in res)
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] <= 128 and r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
