"""ldpc_hip_relay_decode_batch and ldpc_hip_relay_decode_lds_bytes (include/ldpc_amd.h) without a GPU: the exported symbols
and their prototypes, everything the call refuses before it touches a device, the binding's own checks, the LDS formula,
the compile-time resources of kernels_relay_decode.hip, and the properties of the numpy mirror (tests/relay_decode_ref.py):
the identity with SyndromeDecodeMirror, the prefix rule, the sign symmetry of the memory term, the iters convention, the
clamp of gamma, and the four conditions on the toric code that the GPU tests rest on."""
import ctypes as ct
import os

import numpy as np
import pytest

import gf2_ref
import orc
import philox_ref
import relay_decode_ref as rr
import syndrome_decode_ref as sd

F64, F32, F16, I8 = 0, 1, 2, 3
U8, PACKED = 0, 1
ENTRY = b"ldpc_hip_relay_decode_batch"
FIELDS = ("legs", "first_iterations", "leg_iterations", "stop_after", "q_bits", "step", "scale", "offset", "form", "flags")


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(lib):
    """Every test of this file, the mirror's included, is about the contract of one entry: without it none has a subject."""
    import libldpc_amd
    assert hasattr(lib, "ldpc_hip_relay_decode_batch") and hasattr(lib, "ldpc_hip_relay_decode_lds_bytes")
    assert hasattr(libldpc_amd.HipDecoder, "relay_decode_batch") and hasattr(libldpc_amd.HipDecoder, "relay_gammas")


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return rr.Codes(tmp_path_factory.mktemp("relay"))


def test_symbols_and_signatures(lib):
    import libldpc_amd
    from libldpc_amd import binding
    vp, u64, i32, u32 = ct.c_void_p, ct.c_uint64, ct.c_int, ct.c_uint32
    f = lib.ldpc_hip_relay_decode_batch
    assert f.argtypes == [vp, ct.POINTER(binding.ldpc_hip_relay_decode), u64, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp] and f.restype == i32
    assert lib.ldpc_hip_relay_decode_lds_bytes.argtypes == [vp, i32] and lib.ldpc_hip_relay_decode_lds_bytes.restype == ct.c_int64
    assert list(binding.ldpc_hip_relay_decode._fields_) == [
        ("legs", u32), ("first_iterations", u32), ("leg_iterations", u32), ("stop_after", u32), ("q_bits", i32), ("step", ct.c_double),
        ("scale", ct.c_double), ("offset", ct.c_double), ("form", i32), ("flags", i32)]
    assert ct.sizeof(binding.ldpc_hip_relay_decode) == 56  # (16 bytes, q_bits, padding to 24, three doubles, two ints)
    text = open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read()
    flat = " ".join(text.split())
    assert ("int ldpc_hip_relay_decode_batch(ldpc_hip_ctx *ctx, const ldpc_hip_relay_decode *p, uint64_t n, const void *llr, int llr_type, "
            "const void *syndrome, int syndrome_format, const int8_t *gamma, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight, "
            "uint32_t *solutions, uint32_t *best_leg, uint32_t *cost, void *hip_stream);") in flat
    assert "int64_t ldpc_hip_relay_decode_lds_bytes(const ldpc_hip_ctx *ctx, int form);" in flat
    assert ("typedef struct { uint32_t legs; /* 1..256 */ uint32_t first_iterations; /* 1..65535: iterations leg 0 may take */ "
            "uint32_t leg_iterations; /* 1..65535: iterations every later leg may take */ uint32_t stop_after; /* 1..legs: the call ends "
            "for a frame once this many legs have met s */ int q_bits; /* 2..8 */ double step; /* 2^-20 .. 2^20 */ double scale; "
            "/* (0, 1] */ double offset; /* [0, 1e6] */ int form; /* 0 = the library chooses, 1 = a workgroup per frame, 2 = a wave per "
            "frame; same results */ int flags; /* LDPC_HIP_SYNDROME_SHARED_LLR or 0 */ } ldpc_hip_relay_decode;") in flat
    # the entry stands after the bit-flip query and before the stream interface; the formula and tag 4 are stated
    assert text.index("ldpc_hip_bit_flip_lds_bytes(const ldpc_hip_ctx *ctx);") < text.index("} ldpc_hip_relay_decode;") < text.index("int ldpc_hip_stream_begin(")
    assert "bytes = r16(slots) + r16(4 nc) + 160 + r16(4 ceil(mc / 32)) + r16(nc) + r16(4 ceil(nc / 32))" in flat
    assert "TAG 4" in flat and "tag 4 the gamma table of ldpc_hip_relay_decode_batch" in flat
    kernel = open(os.path.join(orc.ROOT, "libldpc_amd", "csrc", "device_philox.hpp")).read()
    assert "kTagRelay = 4" in kernel and rr.TAG_RELAY == 4 == libldpc_amd.HipDecoder.TAG_RELAY
    assert libldpc_amd.HipDecoder.RELAY_OUTPUTS == rr.KEYS and libldpc_amd.HipDecoder.RELAY_NONE == rr.NONE


def _pairs_code(directory, columns):
    """Check node i lists columns 2 i and 2 i + 1."""
    path = os.path.join(str(directory), f"c{columns}.txt")
    if not os.path.exists(path):
        open(path, "w").write("\n".join(f"{i} {2 * i}\n{i} {2 * i + 1}" for i in range(columns // 2)))
    return path


def test_refusals_come_before_the_gpu(lib, codes, tmp_path_factory):
    """No GPU here: a call that reached the device would fail with another message, or not at all.  After every refusal a
    valid call is taken as before."""
    import libldpc_amd
    from libldpc_amd.binding import ldpc_hip_relay_decode as Spec
    d = codes.decoder("sd_small")
    llr = np.ones((2, d.nc), np.float64)
    syn = np.zeros((2, d.mc), np.uint8)
    gam = np.zeros((256, d.nc), np.int8)
    bits, cnt = np.zeros((2, (d.nc + 31) // 32), np.uint32), np.zeros(2, np.uint32)
    err = lib.ldpc_hip_last_error
    good = dict(legs=3, first_iterations=5, leg_iterations=4, stop_after=1, q_bits=6, step=0.25, scale=0.8125, offset=0.0, form=0, flags=0)

    def run(n, spec=good, kind=F64, src=llr.ctypes.data, fmt=U8, s=syn.ctypes.data, g=gam.ctypes.data, ctx=None, outs=True):
        p = None if spec is None else ct.byref(Spec(*(spec[k] for k in FIELDS)))
        o = [bits.ctypes.data] + [cnt.ctypes.data] * 5 if outs else [None] * 6
        return lib.ldpc_hip_relay_decode_batch(ctx or d.ctx, p, n, src, kind, s, fmt, g, *o, None)

    def still_taken():
        assert run(0) == 0 and run(0, outs=False) == 0 and run(0, src=None, s=None, g=None) == 0

    still_taken()
    nan, inf = float("nan"), float("inf")
    bad = [(None, b"null parameters")]
    bad += [(dict(good, legs=v), b"legs") for v in (0, 257, 2**32 - 1)]
    bad += [(dict(good, first_iterations=v), b"first_iterations") for v in (0, 65536, 2**32 - 1)]
    bad += [(dict(good, leg_iterations=v), b"leg_iterations") for v in (0, 65536, 2**32 - 1)]
    bad += [(dict(good, stop_after=v), b"stop_after") for v in (0, 4, 2**32 - 1)]
    bad += [(dict(good, q_bits=v), b"q_bits") for v in (-1, 0, 1, 9, 16)]
    bad += [(dict(good, step=v), b"step") for v in (nan, 0.0, -0.25, 2.0**-21, 2.0**20 * 1.0000001, inf, -inf)]
    bad += [(dict(good, scale=v), b"scale") for v in (nan, 0.0, -0.5, 1.0000001, inf)]
    bad += [(dict(good, offset=v), b"offset") for v in (nan, -1e-9, 1e6 * 1.0000001, inf)]
    bad += [(dict(good, form=v), b"form") for v in (-1, 3, 255)]
    bad += [(dict(good, flags=v), b"flag") for v in (2, 3, 4, -1, 1 << 30)]
    for spec, word in bad:
        for n in (0, 2):
            assert run(n, spec) == -1 and ENTRY in err() and word in err(), (spec, n, err())
        still_taken()
    for n in (0, 2):
        for kind in (4, -1, 17):
            assert run(n, kind=kind) == -1 and ENTRY in err() and b"LLR type" in err(), (n, kind, err())
        for fmt in (2, -1, 9):
            assert run(n, fmt=fmt) == -1 and ENTRY in err() and b"syndrome" in err(), (n, fmt, err())
        still_taken()
    assert run(2, src=None) == -1 and ENTRY in err() and b"null llr" in err()
    still_taken()
    # the edges of the ranges are taken: every type, both formats, the shared row, a null syndrome, a null gamma
    for spec in (dict(good, legs=1), dict(good, legs=256, stop_after=256), dict(good, first_iterations=1), dict(good, first_iterations=65535),
                 dict(good, leg_iterations=1), dict(good, leg_iterations=65535), dict(good, stop_after=3), dict(good, q_bits=2),
                 dict(good, q_bits=8), dict(good, step=2.0**-20), dict(good, step=2.0**20), dict(good, scale=1.0), dict(good, scale=5e-324),
                 dict(good, offset=1e6), dict(good, form=1), dict(good, form=2), dict(good, flags=1)):
        for kind in (F64, F32, F16, I8):
            for fmt in (U8, PACKED):
                assert run(0, spec, kind, fmt=fmt) == 0 and run(0, spec, kind, fmt=fmt, s=None, g=None) == 0, (spec, kind, fmt, err())
    # a code the call does not take, and a form the code does not fit, are refused before the GPU, frames or none
    where = tmp_path_factory.mktemp("relaybig")
    big = libldpc_amd.HipDecoder(_pairs_code(where, 65536))
    assert big.nc == 65536 and all(big.relay_decode_lds_bytes(form) == -1 for form in (0, 1, 2))
    wide = np.ones((2, big.nc), np.int8)
    for n in (0, 2):
        assert run(n, kind=I8, src=wide.ctypes.data, s=None, g=None, ctx=big.ctx) == -1 and ENTRY in err() and b"65 535" in err(), err()
    mid = libldpc_amd.HipDecoder(_pairs_code(where, 20000))
    assert mid.relay_decode_lds_bytes(1) == mid.relay_decode_lds_bytes(0) > 40 * 1024 and mid.relay_decode_lds_bytes(2) == -1
    for n in (0, 2):
        assert run(n, dict(good, form=2), kind=I8, src=wide.ctypes.data, s=None, g=None, ctx=mid.ctx) == -1
        assert ENTRY in err() and b"form 2 does not fit" in err(), err()
        assert run(0, dict(good, form=n // 2), kind=I8, src=wide.ctypes.data, s=None, g=None, ctx=mid.ctx) == 0, err()
    with pytest.raises(RuntimeError, match="ldpc_hip_relay_decode_batch"):
        big.relay_decode_batch(wide[:0], legs=1)
    still_taken()
    # the binding, n == 0
    for dt in (np.float64, np.float32, np.float16, np.int8):
        r = d.relay_decode_batch(np.zeros((0, d.nc), dt), legs=2)
        assert tuple(r) == rr.KEYS and r["hard_bits"].shape == (0, (d.nc + 31) // 32) and all(r[k].shape == (0,) for k in rr.KEYS[1:])
        assert all(r[k].dtype == np.uint32 for k in rr.KEYS)


def test_binding_refuses_other_dtypes_and_shapes(lib, codes):
    d = codes.decoder("sd_small")
    words, swords = (d.nc + 31) // 32, (d.mc + 31) // 32
    ok = np.zeros((0, d.nc), np.float32)
    with pytest.raises(TypeError):
        d.relay_decode_batch(ok)  # legs has no default
    with pytest.raises(TypeError):
        d.relay_decode_batch(ok, None, None, 3)  # ... and is a keyword
    for dt in (np.uint8, np.int16, np.int32, np.int64, np.uint32, np.bool_, np.complex64):
        with pytest.raises(TypeError, match="relay_decode_batch"):
            d.relay_decode_batch(np.zeros((1, d.nc), dt), legs=1)
    for shape in ((1, d.nc + 1), (1, d.nc - 1), (d.nc,), (1, 1, d.nc), (1, words)):
        with pytest.raises(ValueError, match="relay_decode_batch"):
            d.relay_decode_batch(np.zeros(shape, np.float64), legs=1)
    one = np.zeros((1, d.nc), np.float64)
    for dt in (np.int8, np.float32, np.uint16, np.int32, np.uint64):
        with pytest.raises(TypeError, match="relay_decode_batch"):
            d.relay_decode_batch(one, np.zeros((1, d.mc), dt), legs=1)
    for s in (np.zeros((1, d.mc + 1), np.uint8), np.zeros((1, swords + 1), np.uint32), np.zeros((2, d.mc), np.uint8)):
        with pytest.raises(ValueError, match="relay_decode_batch"):
            d.relay_decode_batch(one, s, legs=1)
    for g in (np.zeros((2, d.nc), np.uint8), np.zeros((2, d.nc), np.int16), np.zeros((2, d.nc), np.float32)):
        with pytest.raises(TypeError, match="gamma"):
            d.relay_decode_batch(ok, None, g, legs=2)
    for g in (np.zeros((3, d.nc), np.int8), np.zeros((2, d.nc + 1), np.int8), np.zeros(2 * d.nc, np.int8)):
        with pytest.raises(ValueError, match="gamma"):
            d.relay_decode_batch(ok, None, g, legs=2)
    with pytest.raises(ValueError, match="shared"):
        d.relay_decode_batch(np.zeros(d.nc), None, legs=1, shared_llr=True)
    for shape in ((d.nc,), (1, d.nc)):
        r = d.relay_decode_batch(np.zeros(shape), np.zeros((0, swords), np.uint32), np.zeros((2, d.nc), np.int8), legs=2, shared_llr=True)
        assert r["cost"].shape == (0,)
    for kw in (dict(legs=-1), dict(legs=2**32), dict(legs=1, first_iterations=-1), dict(legs=1, leg_iterations=2**32), dict(legs=1, stop_after=-1)):
        with pytest.raises(ValueError, match="relay_decode_batch"):
            d.relay_decode_batch(ok, **kw)
    with pytest.raises(KeyError):
        d.relay_decode_batch(ok, legs=1, want=("llr_out",))
    with pytest.raises(TypeError, match="cost"):
        d.relay_decode_batch(ok, legs=1, want=(), out={"cost": np.zeros(0, np.int32)})
    with pytest.raises(ValueError, match="best_leg"):
        d.relay_decode_batch(ok, legs=1, want=(), out={"best_leg": np.zeros(1, np.uint32)})
    with pytest.raises(ValueError, match="hard_bits"):
        d.relay_decode_batch(ok, legs=1, want=(), out={"hard_bits": np.zeros((0, words + 1), np.uint32)})
    # what the library refuses comes back as an error that names the entry
    for kw in (dict(legs=0), dict(legs=257), dict(legs=2, stop_after=3), dict(legs=1, first_iterations=0), dict(legs=1, q_bits=9),
               dict(legs=1, step=0.0), dict(legs=1, scale=1.5), dict(legs=1, offset=-1.0), dict(legs=1, form=3)):
        with pytest.raises(RuntimeError, match="ldpc_hip_relay_decode_batch"):
            d.relay_decode_batch(ok, **kw)
    for kw in (dict(legs=0, lo=0, hi=1), dict(legs=257, lo=0, hi=1), dict(legs=2, lo=2, hi=1), dict(legs=2, lo=-129, hi=0), dict(legs=2, lo=0, hi=128)):
        with pytest.raises(ValueError, match="relay_gammas"):
            d.relay_gammas(seed=1, **kw)


def _formula(code):
    """The formula of the header, restated; None where the header says -1."""
    def r16(v):
        return -(-v // 16) * 16
    degrees = np.bincount(code.h_rows, minlength=code.mc)
    if code.nc > 65535 or degrees.min() < 2:
        return None
    slots = int((-(-degrees // 4) * 4).sum())
    total = r16(slots) + r16(4 * code.nc) + 160 + r16(4 * -(-code.mc // 32)) + r16(code.nc) + r16(4 * -(-code.nc // 32))
    return total if total <= 160 * 1024 else None


def test_lds_bytes_formula(lib, codes, tmp_path_factory):
    import libldpc_amd
    seen = {}
    for name in rr.NAMES:
        code, dec = codes.gf2(name), codes.decoder(name)
        want = _formula(code)
        seen[name] = dec.relay_decode_lds_bytes()
        assert want is not None and 4 * want <= 160 * 1024
        assert [dec.relay_decode_lds_bytes(form) for form in (0, 1, 2)] == [want] * 3 == [lib.ldpc_hip_relay_decode_lds_bytes(dec.ctx, f) for f in (0, 1, 2)]
        assert want == dec.syndrome_decode_lds_bytes() + -(-(4 * -(-code.nc // 32)) // 16) * 16  # the parent's frame and the kept word
        assert all(dec.relay_decode_lds_bytes(form) == -1 for form in (-1, 3, 100))
    assert seen["sd_r36"] == 288 * 8 + 4 * 576 + 160 + 48 + 576 + 80
    assert seen["sd_small"] == 80 + 160 + 160 + 16 + 48 + 16
    assert seen["toric6"] == 36 * 4 + 288 + 160 + 16 + 80 + 16  # 704 bytes a frame
    where = tmp_path_factory.mktemp("relaybig")
    for columns, forms in ((65536, (None, None, None)), (20000, (True, True, None))):
        path = _pairs_code(where, columns)
        want = _formula(gf2_ref.Gf2Code(path))
        dec = libldpc_amd.HipDecoder(path)
        assert (want is None) == (forms[0] is None)
        assert [dec.relay_decode_lds_bytes(f) for f in (0, 1, 2)] == [want if ok else -1 for ok in forms]
        assert want is None or want <= 160 * 1024 < 4 * want


def test_kernel_resources(lib):
    """kernels_relay_decode.hip: one body in two instantiations, no scratch, no vector-register spills, no static LDS, at most
    128 registers; the parent's kernel file is as it was.  Scalar registers may spill: the call has six outputs and a gamma
    more than the parent's kernel, and a spilled scalar register lives in a lane of a vector register, not in memory — which
    ScratchSize == 0 says."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_relay_decode.hip")
    assert res and len(res) == 2 and all("relay_decode_kernel" in k for k in res)
    assert sorted(k.split("relay_decode_kernelILi")[1].split("E")[0] for k in res) == ["256", "64"]
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] <= 128 and r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
    assert len(build.kernel_resources("kernels_syndrome_decode.hip")) == 1
    source = open(os.path.join(orc.ROOT, "libldpc_amd", "csrc", "kernels_relay_decode.hip")).read()
    assert "printf" not in source and "assert(" not in source and "clock" not in source


# ---- the mirror ----
def _inputs(codes, name, n):
    """llr[n][nc], s[n][mc] of a code: the BSC frames, or the toric errors under their one prior row."""
    if name.startswith("toric"):
        f = codes.toric(name)
        return np.repeat(f["llr"][None, :], n, 0), f["s"][:n]
    f = codes.frames(name)
    return f["llr"][:n], f["s"][:n]


@pytest.mark.parametrize("name", rr.NAMES)
def test_one_leg_without_memory_is_the_syndrome_decoder(codes, name):
    """The identity of the header on the mirrors: legs = 1 and gamma null or zero."""
    m = codes.mirror(name)
    llr, s = _inputs(codes, name, 48)
    stopped = set()
    for setting in rr.SETTINGS:
        for iterations in (50, 3, 1):
            want = sd.SyndromeDecodeMirror.decode_toward(m, llr, s, *setting, True, iterations)
            for gamma in (None, np.zeros((1, m.nc), np.int8)):
                got = m.relay(llr, s, gamma, *setting, legs=1, first_iterations=iterations)
                assert all(np.array_equal(got[k], want[k]) for k in ("hard", "iters", "weight")), (name, setting, iterations)
                assert np.array_equal(got["solutions"], want["weight"] == 0) and np.array_equal(got["best_leg"] == 0, want["weight"] == 0)
            stopped |= set((want["iters"] < iterations).tolist())
    assert stopped == {True, False}
    toward_zero = m.relay(llr, None, None, *rr.SETTINGS[0], legs=1)
    assert np.array_equal(toward_zero["hard"], sd.SyndromeDecodeMirror.decode_toward(m, llr, None, *rr.SETTINGS[0])["hard"])


@pytest.mark.parametrize("name", ("toric6", "sd_mix"))
def test_prefix_rule(codes, name):
    m = codes.mirror(name)
    llr, s = _inputs(codes, name, 96)
    gamma = rr.gammas(m.nc, 7, -16, 42, rr.GAMMA_SEED, 8)
    kw = dict(first_iterations=20, leg_iterations=10)
    seen = 0
    for stop_after in (1, 2):
        long = m.relay(llr, s, gamma, *rr.SETTINGS[0], legs=7, stop_after=stop_after, **kw)
        for k in range(stop_after, 7):
            short = m.relay(llr, s, gamma[:k], *rr.SETTINGS[0], legs=k, stop_after=stop_after, **kw)
            ended = short["solutions"] >= stop_after
            seen += int(ended.sum())
            for key in ("hard", "iters", "weight", "solutions", "best_leg", "cost"):
                assert np.array_equal(short[key][ended], long[key][ended]), (name, stop_after, k, key)
            # ... and on the others the shorter run has spent all its legs
            assert (short["iters"][~ended] <= long["iters"][~ended]).all()
    assert seen > 0


def test_memory_term_is_sign_symmetric():
    """Exhaustively over g and a range of differences: f(g, L + d, L) - L is odd in d and odd in g, rounds half away from zero,
    and is 0 at g = 0; out-of-range g is its clamp."""
    g = np.arange(-128, 128)[:, None, None]
    d = np.arange(-3000, 3001)[None, :, None]
    L = np.asarray([-127, -9, 0, 1, 127])[None, None, :]
    lam = rr.memory_term(g, L + d, L) - L
    assert np.array_equal(lam, -rr.memory_term(g, L - d, L) + L)            # odd in the difference
    assert np.array_equal(lam[1:], -lam[1:][::-1])                          # odd in g (-127..127)
    assert not lam[128].any() and np.array_equal(lam[:64], np.broadcast_to(lam[64], lam[:64].shape))  # g = 0; g < -64 is -64
    assert np.array_equal(lam[193:], np.broadcast_to(lam[192], lam[193:].shape)) and np.array_equal(lam[192, :, 0], d[0, :, 0])  # g = 64: d
    exact = np.clip(g, -64, 64) * d / 64.0
    want = np.sign(exact) * np.floor(np.abs(exact) + 0.5)                   # half away from zero
    assert np.array_equal(lam, np.broadcast_to(want, lam.shape).astype(np.int64))
    # the clamp of Lambda, and the width of the product at the largest total a frame can hold
    assert rr.memory_term(64, 10**6, 100) == 32767 and rr.memory_term(-64, 10**6, 100) == -32767
    assert 64 * (32767 + 65535 * 127 + 127) < 2**31


def test_iters_convention_and_gamma_clamp(codes):
    m = codes.mirror("toric6")
    llr, s = _inputs(codes, "toric6", 64)
    gamma = codes.toric_gamma()[:4]
    r = m.relay(llr, s, gamma, *rr.SETTINGS[0], legs=4, first_iterations=9, leg_iterations=5, stop_after=4)
    # a frame that never met s has spent 9 + 3 * 5 iterations; one that met it in every leg fewer than the legs' caps
    never = r["solutions"] == 0
    assert never.any() and (r["iters"][never] == 24).all() and (r["weight"][never] > 0).all()
    assert (r["best_leg"][never] == rr.NONE).all() and (r["cost"][never] == rr.NONE).all()
    some = ~never
    assert some.any() and (r["iters"][some] < 24).all() and (r["weight"][some] == 0).all() and (r["best_leg"][some] < 4).all()
    # one leg: i of the iteration that met s, else T
    one = m.relay(llr, s, gamma[:1], *rr.SETTINGS[0], legs=1, first_iterations=9)
    assert np.array_equal(one["iters"] == 9, one["solutions"] == 0) and one["iters"].max() == 9
    # the cost is what the word contradicts of the input, and the cheapest is kept
    L = m.input_values(llr, rr.SETTINGS[0][0], rr.SETTINGS[0][1])
    cost = (np.abs(L) * (r["hard"] != (L <= 0))).sum(1)
    assert np.array_equal(cost[some], r["cost"][some])
    # out-of-range gamma is its clamp
    wild = gamma.astype(np.int64) * 3
    assert (np.abs(wild) > 64).any()
    a = m.relay(llr, s, np.clip(wild, -128, 127).astype(np.int8), *rr.SETTINGS[0], legs=4, first_iterations=9, leg_iterations=5)
    b = m.relay(llr, s, np.clip(wild, -64, 64).astype(np.int8), *rr.SETTINGS[0], legs=4, first_iterations=9, leg_iterations=5)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_gamma_table():
    g = rr.gammas(72, 12, -16, 42, rr.GAMMA_SEED, 8)
    assert g.dtype == np.int8 and g.shape == (12, 72) and (g[0] == 8).all() and g[1:].min() >= -16 and g[1:].max() <= 42
    assert len(np.unique(g[1:])) > 40 and (g[1:] < 0).any()
    w = philox_ref.blocks(rr.GAMMA_SEED, 4, [5], [17 >> 2])[0, 0, 17 & 3]
    assert g[5, 17] == -16 + ((int(w) * 59) >> 32)
    assert np.array_equal(rr.gammas(70, 3, -16, 42, rr.GAMMA_SEED, 8), g[:3, :70])  # a draw depends on (row, column) alone
    assert (rr.gammas(8, 4, 5, 5, 1) [1:] == 5).all() and (rr.gammas(8, 4, 5, 5, 1)[0] == 0).all()


def test_toric_file(codes):
    code = codes.gf2("toric6")
    assert (code.nc, code.mc, code.h_rows.size) == (72, 36, 144)
    assert (np.bincount(code.h_cols) == 2).all() and (np.bincount(code.h_rows) == 4).all()
    lines = open(codes.path("toric6")).read().split("\n")
    assert lines[:4] == ["0 0", "0 5", "0 36", "0 66"]  # vertex (0, 0): h(0, 0), h(0, 5), v(0, 0), v(5, 0)
    assert codes.gf2("toric12").nc == 288


def test_the_conditions_on_toric6(codes):
    """What the GPU comparison rests on, on the mirror alone: the four conditions of the issue under the Philox gamma of
    GAMMA_SEED, at both settings of the GPU test."""
    m, f, t = codes.mirror("toric6"), codes.toric(), rr.TORIC_RELAY
    n = rr.TORIC_FRAMES
    llr = np.repeat(f["llr"][None, :], n, 0)
    assert f["s"].shape == (n, 36) and 0.07 < f["x"].mean() < 0.11
    gamma = codes.toric_gamma()
    for setting in rr.SETTINGS[:2]:
        plain = sd.SyndromeDecodeMirror.decode_toward(m, llr, f["s"], *setting, True, 50)
        single = m.relay(llr, f["s"], gamma[:1], *setting, legs=1, first_iterations=t["first_iterations"])
        relay = {sa: codes.toric_expected(setting, sa) for sa in (1, 3)}
        full = m.relay(llr, f["s"], gamma, *setting, legs=t["legs"], first_iterations=t["first_iterations"],
                       leg_iterations=t["leg_iterations"], stop_after=3)
        reached = {sa: int((relay[sa]["weight"] == 0).sum()) for sa in (1, 3)}
        print(f"toric6 {setting}: plain {int((plain['weight'] == 0).sum())}, one leg {int((single['weight'] == 0).sum())}, relay {reached} of {n}; "
              f"later best {int(((full['best_leg'] != rr.NONE) & (full['best_leg'] > full['first_leg'])).sum())}, none {int((full['solutions'] == 0).sum())}")
        assert (plain["weight"] > 0).any()                                                      # plain min-sum leaves some short
        assert reached[1] > int((single["weight"] == 0).sum()) and reached[3] == reached[1]     # the relay reaches strictly more
        assert ((full["best_leg"] != rr.NONE) & (full["best_leg"] > full["first_leg"])).any()   # a later leg's word is cheaper
        assert (full["solutions"] == 0).any() and (relay[1]["solutions"] == 0).any()            # some frame is never solved
        assert relay[3]["solutions"].max() == 3 and relay[1]["solutions"].max() == 1
        assert np.array_equal(relay[3]["best_leg"], full["best_leg"].astype(np.uint32))
