"""ldpc_hip_syndrome_decode_batch and ldpc_hip_syndrome_decode_lds_bytes (include/ldpc_amd.h) without a GPU: the exported
symbols and their prototypes, everything the call refuses before it touches a device, the binding's own checks, the LDS
formula, the compile-time resources of kernels_syndrome_decode.hip, and the identities that tie the numpy mirror
(tests/syndrome_decode_ref.py) to the mirror of quantized min-sum: toward the zero syndrome it IS that decoder, toward any
syndrome it is that decoder on the augmented code [H | I]."""
import ctypes as ct
import os

import numpy as np
import pytest

import orc
import syndrome_decode_ref as sd
from quantized_minsum_ref import QuantizedMinSumMirror, qmax_of, quantize

F64, F32, F16, I8 = 0, 1, 2, 3
U8, PACKED = 0, 1
ENTRY = b"ldpc_hip_syndrome_decode_batch"


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(lib):
    """Every test of this file, the mirror's included, is about the contract of one entry: without it none has a subject."""
    assert hasattr(lib, "ldpc_hip_syndrome_decode_batch") and hasattr(lib, "ldpc_hip_syndrome_decode_lds_bytes")


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return sd.Codes(tmp_path_factory.mktemp("sd"))


def test_symbols_and_signatures(lib):
    import libldpc_amd
    from libldpc_amd import binding
    vp, u64, i32 = ct.c_void_p, ct.c_uint64, ct.c_int
    f = lib.ldpc_hip_syndrome_decode_batch
    assert f.argtypes == [vp, ct.POINTER(binding.ldpc_hip_syndrome_decode), u64, vp, i32, vp, i32, vp, vp, vp, vp, vp] and f.restype == i32
    assert lib.ldpc_hip_syndrome_decode_lds_bytes.argtypes == [vp] and lib.ldpc_hip_syndrome_decode_lds_bytes.restype == ct.c_int64
    fields = [(n, t) for n, t in binding.ldpc_hip_syndrome_decode._fields_]
    assert fields == [("iterations", ct.c_uint32), ("early_term", ct.c_int), ("q_bits", ct.c_int), ("step", ct.c_double),
                      ("scale", ct.c_double), ("offset", ct.c_double), ("flags", ct.c_int)]
    assert ct.sizeof(binding.ldpc_hip_syndrome_decode) == 48  # (12 bytes, padding to 16, three doubles, the flags, padding)
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_syndrome_decode_batch(ldpc_hip_ctx *ctx, const ldpc_hip_syndrome_decode *p, uint64_t n, const void *llr, "
            "int llr_type, const void *syndrome, int syndrome_format, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight, "
            "double *llr_out, void *hip_stream);") in flat
    assert "int64_t ldpc_hip_syndrome_decode_lds_bytes(const ldpc_hip_ctx *ctx);" in flat
    assert "enum { LDPC_HIP_SYNDROME_SHARED_LLR = 1 };" in flat
    assert ("typedef struct { uint32_t iterations; int early_term; /* 0 / 1 */ int q_bits; /* 2..8 */ double step; /* 2^-20 .. 2^20 */ "
            "double scale; /* (0, 1] */ double offset; /* [0, 1e6] */ int flags; /* LDPC_HIP_SYNDROME_SHARED_LLR or 0 */ } "
            "ldpc_hip_syndrome_decode;") in flat
    assert libldpc_amd.HipDecoder.SYNDROME_SHARED_LLR == 1


def _big_code(directory):
    """65 536 columns: check node i lists columns 2 i and 2 i + 1."""
    path = os.path.join(str(directory), "c65536.txt")
    if not os.path.exists(path):
        open(path, "w").write("\n".join(f"{i} {2 * i}\n{i} {2 * i + 1}" for i in range(32768)))
    return path


def test_refusals_come_before_the_gpu(lib, codes, tmp_path_factory):
    """No GPU here: a call that reached the device would fail with another message, or not at all.  After every refusal a
    valid call is taken as before."""
    import libldpc_amd
    from libldpc_amd.binding import ldpc_hip_syndrome_decode as Spec
    d = codes.decoder("sd_small")
    llr = np.ones((2, d.nc), np.float64)
    syn = np.zeros((2, d.mc), np.uint8)
    bits, cnt, soft = np.zeros((2, (d.nc + 31) // 32), np.uint32), np.zeros(2, np.uint32), np.zeros((2, d.nc), np.float64)
    err = lib.ldpc_hip_last_error
    good = dict(iterations=5, early_term=1, q_bits=6, step=0.25, scale=0.8125, offset=0.0, flags=0)

    def run(n, spec=good, kind=F64, src=llr.ctypes.data, fmt=U8, s=syn.ctypes.data, ctx=None, outs=True):
        p = None if spec is None else ct.byref(Spec(*(spec[k] for k in ("iterations", "early_term", "q_bits", "step", "scale", "offset", "flags"))))
        o = [bits.ctypes.data, cnt.ctypes.data, cnt.ctypes.data, soft.ctypes.data] if outs else [None] * 4
        return lib.ldpc_hip_syndrome_decode_batch(ctx or d.ctx, p, n, src, kind, s, fmt, *o, None)

    def still_taken():
        assert run(0) == 0 and run(0, outs=False) == 0 and run(0, src=None, s=None) == 0

    still_taken()
    nan, inf = float("nan"), float("inf")
    bad = [None]
    bad += [dict(good, q_bits=v) for v in (-1, 0, 1, 9, 16)]
    bad += [dict(good, step=v) for v in (nan, 0.0, -0.25, 2.0**-21, 2.0**20 * 1.0000001, inf, -inf)]
    bad += [dict(good, scale=v) for v in (nan, 0.0, -0.5, 1.0000001, inf)]
    bad += [dict(good, offset=v) for v in (nan, -1e-9, 1e6 * 1.0000001, inf)]
    bad += [dict(good, early_term=v) for v in (-1, 2, 255)]
    bad += [dict(good, flags=v) for v in (2, 3, 4, -1, 1 << 30)]
    for spec in bad:
        for n in (0, 2):
            assert run(n, spec) == -1 and ENTRY in err(), (spec, n, err())
        still_taken()
    for n in (0, 2):
        for kind in (4, -1, 17):
            assert run(n, kind=kind) == -1 and ENTRY in err() and b"LLR type" in err(), (n, kind, err())
        for fmt in (2, -1, 9):
            assert run(n, fmt=fmt) == -1 and ENTRY in err(), (n, fmt, err())
        still_taken()
    assert run(2, src=None) == -1 and ENTRY in err() and b"null llr" in err()
    still_taken()
    # the edges of the ranges are taken: every type, both formats, the shared row, a null syndrome
    for spec in (dict(good, q_bits=2), dict(good, q_bits=8), dict(good, step=2.0**-20), dict(good, step=2.0**20), dict(good, scale=1.0),
                 dict(good, scale=5e-324), dict(good, offset=1e6), dict(good, early_term=0), dict(good, flags=1), dict(good, iterations=0),
                 dict(good, iterations=2**32 - 1)):
        for kind in (F64, F32, F16, I8):
            for fmt in (U8, PACKED):
                assert run(0, spec, kind, fmt=fmt) == 0 and run(0, spec, kind, fmt=fmt, s=None) == 0, (spec, kind, fmt, err())
    # a code the call does not take is refused before the GPU, frames or none
    big = libldpc_amd.HipDecoder(_big_code(tmp_path_factory.mktemp("sdbig")))
    assert big.nc == 65536 and big.syndrome_decode_lds_bytes() == -1 and lib.ldpc_hip_syndrome_decode_lds_bytes(big.ctx) == -1
    wide = np.ones((2, big.nc), np.int8)
    for n in (0, 2):
        assert run(n, kind=I8, src=wide.ctypes.data, s=None, ctx=big.ctx) == -1 and ENTRY in err() and b"65 535" in err(), err()
    with pytest.raises(RuntimeError, match="ldpc_hip_syndrome_decode_batch"):
        big.syndrome_decode_batch(wide[:0])
    still_taken()
    # the binding, n == 0
    for dt in (np.float64, np.float32, np.float16, np.int8):
        r = d.syndrome_decode_batch(np.zeros((0, d.nc), dt), want=sd.KEYS)
        assert set(r) == set(sd.KEYS) and r["hard_bits"].shape == (0, (d.nc + 31) // 32) and r["llr_out"].shape == (0, d.nc)
        assert r["llr_out"].dtype == np.float64 and all(r[k].dtype == np.uint32 for k in sd.KEYS if k != "llr_out")
    assert set(d.syndrome_decode_batch(np.zeros((0, d.nc)))) == {"hard_bits", "iters", "weight"}


def test_binding_refuses_other_dtypes_and_shapes(lib, codes):
    d = codes.decoder("sd_small")
    words, swords = (d.nc + 31) // 32, (d.mc + 31) // 32
    ok = np.zeros((0, d.nc), np.float32)
    for dt in (np.uint8, np.int16, np.int32, np.int64, np.uint32, np.bool_, np.complex64):
        with pytest.raises(TypeError, match="syndrome_decode_batch"):
            d.syndrome_decode_batch(np.zeros((1, d.nc), dt))
    for shape in ((1, d.nc + 1), (1, d.nc - 1), (d.nc,), (1, 1, d.nc), (1, words)):
        with pytest.raises(ValueError, match="syndrome_decode_batch"):
            d.syndrome_decode_batch(np.zeros(shape, np.float64))
    one = np.zeros((1, d.nc), np.float64)
    for dt in (np.int8, np.float32, np.uint16, np.int32, np.uint64):
        with pytest.raises(TypeError, match="syndrome_decode_batch"):
            d.syndrome_decode_batch(one, np.zeros((1, d.mc), dt))
    for s in (np.zeros((1, d.mc + 1), np.uint8), np.zeros((1, d.mc), np.uint32), np.zeros((1, swords + 1), np.uint32), np.zeros(d.mc, np.uint8),
              np.zeros((2, d.mc), np.uint8), np.zeros((0, swords), np.uint32)):
        with pytest.raises(ValueError, match="syndrome_decode_batch"):
            d.syndrome_decode_batch(one, s)
    # the shared row: [nc] or [1][nc], the frames counted by the syndrome
    for shape in ((2, d.nc), (d.nc + 1,), (1, 1, d.nc)):
        with pytest.raises(ValueError, match="shared"):
            d.syndrome_decode_batch(np.zeros(shape), np.zeros((0, d.mc), np.uint8), shared_llr=True)
    with pytest.raises(ValueError, match="shared"):
        d.syndrome_decode_batch(np.zeros(d.nc), None, shared_llr=True)
    for shape in ((d.nc,), (1, d.nc)):
        r = d.syndrome_decode_batch(np.zeros(shape), np.zeros((0, swords), np.uint32), shared_llr=True)
        assert r["iters"].shape == (0,)
    for iterations in (-1, 2**32):
        with pytest.raises(ValueError, match="iterations"):
            d.syndrome_decode_batch(ok, iterations=iterations)
    with pytest.raises(KeyError):
        d.syndrome_decode_batch(ok, want=("hard",))
    with pytest.raises(TypeError, match="llr_out"):
        d.syndrome_decode_batch(ok, want=(), out={"llr_out": np.zeros((0, d.nc), np.float32)})
    with pytest.raises(TypeError, match="weight"):
        d.syndrome_decode_batch(ok, want=(), out={"weight": np.zeros(0, np.int32)})
    with pytest.raises(ValueError, match="iters"):
        d.syndrome_decode_batch(ok, want=(), out={"iters": np.zeros(1, np.uint32)})
    with pytest.raises(ValueError, match="hard_bits"):
        d.syndrome_decode_batch(ok, want=(), out={"hard_bits": np.zeros((0, words + 1), np.uint32)})
    # what the library refuses comes back as an error that names the entry
    for kw in (dict(q_bits=9), dict(step=0.0), dict(scale=1.5), dict(offset=-1.0)):
        with pytest.raises(RuntimeError, match="ldpc_hip_syndrome_decode_batch"):
            d.syndrome_decode_batch(ok, **kw)


def _formula(code):
    """The formula of the header, restated; None where the header says -1."""
    def r16(v):
        return -(-v // 16) * 16
    degrees = np.bincount(code.h_rows, minlength=code.mc)
    if code.nc > 65535 or degrees.min() < 2:
        return None
    slots = int((-(-degrees // 4) * 4).sum())
    total = r16(slots) + r16(4 * code.nc) + 160 + r16(4 * -(-code.mc // 32)) + r16(code.nc)
    return total if total <= 160 * 1024 else None


def test_lds_bytes_formula(lib, codes, tmp_path_factory):
    import gf2_ref
    import libldpc_amd
    seen = {}
    for name in sd.NAMES:
        want = _formula(codes.gf2(name))
        seen[name] = codes.decoder(name).syndrome_decode_lds_bytes()
        assert want is not None and seen[name] == want == lib.ldpc_hip_syndrome_decode_lds_bytes(codes.decoder(name).ctx), (name, seen[name], want)
    assert seen["sd_r36"] == 288 * 8 + 4 * 576 + 160 + 48 + 576  # six messages in two words; nine syndrome words in 48 bytes
    assert seen["sd_small"] == 80 + 160 + 160 + 16 + 48
    assert seen["sd_wide"] == 120 * 20 + 3200 + 160 + 16 + 800
    golden = codes.gf2("golden")
    assert (golden.nc, golden.mc) == (1152, 1024) and seen["golden"] * 8 <= 160 * 1024  # eight frames a CU by the LDS
    big = _big_code(tmp_path_factory.mktemp("sdbig"))
    assert _formula(gf2_ref.Gf2Code(big)) is None and libldpc_amd.HipDecoder(big).syndrome_decode_lds_bytes() == -1
    # the augmented code of the route this call replaces takes more of every part
    for name in ("sd_r36", "golden"):
        aug = libldpc_amd.HipDecoder(codes.path(name + "+I"))
        assert aug.nc == codes.gf2(name).nc + codes.gf2(name).mc and aug.quantized_min_sum_lds_bytes() > seen[name]


def test_kernel_resources(lib):
    """kernels_syndrome_decode.hip: one kernel, no scratch, no spills, no static LDS, at most 128 registers."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_syndrome_decode.hip")
    assert res and len(res) == 1 and "syndrome_decode_kernel" in next(iter(res))
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] <= 128 and r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
    assert len(build.kernel_resources("kernels_qms.hip")) == 2  # (the neighbour is as it was)


# ---- the mirror ----
@pytest.mark.parametrize("name", ("sd_r36", "sd_mix", "sd_small"))
def test_toward_zero_the_mirror_is_quantized_min_sum(codes, name):
    f = codes.frames(name, n=64)
    new, old = codes.mirror(name), QuantizedMinSumMirror(sd.graph(codes.path(name)))
    # the LLRs of random words (never a codeword: such frames run to the end) and of the all-zero codeword (most stop)
    llr = np.concatenate((f["llr"][:16], sd.cr.bsc(codes.gf2(name), sd.POINTS[name][0], sd.NOISE_SEED, np.arange(48), None)[1]))
    f = {"llr": llr, "s": f["s"]}
    stopped = set()
    for (q, step, scale, offset), early, iterations in ((sd.SETTINGS[0], True, 50), (sd.SETTINGS[0], False, 7), (sd.SETTINGS[1], True, 1),
                                                        (sd.SETTINGS[2], True, 20), (sd.SETTINGS[3], True, 50)):
        a = new.decode_toward(f["llr"], None, q, step, scale, offset, early, iterations)
        b = old.decode(f["llr"], q, step, scale, offset, early, iterations)
        assert np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["hard"], b["hard"]) and np.array_equal(a["llr_out"], b["llr_out"])
        assert np.array_equal(a["total"].astype(np.float64) * step, b["llr_out"])
        assert np.array_equal(a["weight"] == 0, codes.gf2(name).syndrome(a["hard"])[1] == 0)
        stopped |= set((a["iters"] < iterations).tolist())
    assert stopped == {True, False}
    zero = new.decode_toward(f["llr"], f["s"], 6, 0.25, iterations=0)  # iterations == 0: the quantized input
    L = quantize(f["llr"], 6, 0.25)
    assert np.array_equal(zero["total"], L) and np.array_equal(zero["hard"], L <= 0) and not zero["iters"].any()
    assert np.array_equal(zero["weight"], (codes.gf2(name).syndrome(L <= 0)[0] != f["s"]).sum(1))


@pytest.mark.parametrize("name", ("sd_r36", "sd_mix", "sd_wide", "sd_small"))
def test_toward_a_syndrome_the_mirror_is_quantized_min_sum_on_the_augmented_code(codes, name):
    """[H | I] with 99999.9 (1 - 2 s) on the extra columns, decoded toward zero: the same messages always (the extra column has
    one edge, so what it sends is its own +-Qmax whatever it receives), hence the same totals and decisions on the first nc
    columns after any number of iterations.  The extra column's DECISION is s as long as its total is not zero: it receives
    +-lut[min], and with a scale below 1 lut[Qmax] < Qmax, so the total keeps the sign of +-Qmax, the decisions there are s in
    every iteration and the two stop in the same iteration.  With (scale, offset) = (1, 0) a check node whose other messages
    all sit at Qmax returns Qmax against the extra column, the total is 0, the tie decides 1 and the augmented route goes on
    where this decoder has stopped (at 2 bits, Qmax = 1, that happens in most frames): those settings are compared without
    early termination, and the extra decisions where their total is not zero."""
    f = codes.frames(name, n=64)
    code = codes.gf2(name)
    new, aug = codes.mirror(name), QuantizedMinSumMirror(sd.graph(codes.path(name + "+I")))
    assert (aug.nc, aug.mc, aug.nnz) == (code.nc + code.mc, code.mc, new.nnz + code.mc)
    s = np.random.default_rng(3).integers(0, 2, (64, code.mc), dtype=np.uint8)  # any syndrome, reachable or not
    for syn in (f["s"], s):
        wide = np.concatenate((f["llr"], sd.SHORTEN * (1.0 - 2.0 * syn)), axis=1)
        for (q, step, scale, offset), early, iterations in ((sd.SETTINGS[0], True, 50), (sd.SETTINGS[0], False, 3), (sd.SETTINGS[1], False, 5),
                                                            (sd.SETTINGS[2], False, 10), (sd.SETTINGS[3], True, 50)):
            assert scale < 1.0 or not early
            a = new.decode_toward(f["llr"], syn, q, step, scale, offset, early, iterations)
            b = aug.decode(wide, q, step, scale, offset, early, iterations)
            assert np.array_equal(a["iters"], b["iters"]), (name, q, early)
            assert np.array_equal(a["hard"], b["hard"][:, :code.nc]) and np.array_equal(a["llr_out"], b["llr_out"][:, :code.nc])
            extra, tie = b["hard"][:, code.nc:], b["llr_out"][:, code.nc:] == 0.0
            assert np.array_equal(extra == syn, ~tie | (syn == 1)) and (scale == 1.0 or not tie.any())
            assert np.array_equal(a["weight"], (code.syndrome(a["hard"])[0] != syn).sum(1))
    reached = new.decode_toward(f["llr"], f["s"], *sd.SETTINGS[0])["weight"] == 0
    assert 0 < reached.sum() < 64 or name == "sd_wide"


def test_an_int8_counts_steps():
    """clamp(k) is the quantizer applied to fl(k * step), for all 256 values."""
    k = np.arange(-128, 128).astype(np.int8)
    mirror = sd.SyndromeDecodeMirror.__new__(sd.SyndromeDecodeMirror)
    mirror.nc = 256
    for step in (2.0**-20, 0.25, 1.0, 3.7, 2.0**20):
        for bits in range(2, 9):
            q = qmax_of(bits)
            want = np.clip(k.astype(np.int64), -q, q)
            assert np.array_equal(quantize(k.astype(np.float64) * np.float64(step), bits, step), want), (step, bits)
            assert np.array_equal(mirror.input_values(k[None, :], bits, step)[0], want)
