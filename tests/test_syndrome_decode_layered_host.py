"""ldpc_hip_syndrome_decode_layered_batch and ldpc_hip_syndrome_decode_layered_lds_bytes (include/ldpc_amd.h) without a GPU:
the exported symbols and their prototypes, everything the call refuses before it touches a device, the binding's own checks,
the LDS formula, the compile-time resources of kernels_syndrome_decode_layered.hip, and the numpy mirror
(tests/syndrome_decode_layered_ref.py) by itself: toward the zero syndrome it IS the mirror of fixed-point layered min-sum,
toward any syndrome it is that mirror on the augmented code [H | I] where identity (b) of the header applies, one sweep by
hand, iterations == 0, and the operating points the GPU tests use."""
import ctypes as ct
import os

import numpy as np
import pytest

import orc
import syndrome_decode_layered_ref as sdl
import syndrome_decode_ref as sd
from layered_fixed_minsum_ref import LayeredFixedMinSumMirror
from minsum_common import write
from quantized_minsum_ref import qmax_of, quantize

F64, F32, F16, I8 = 0, 1, 2, 3
U8, PACKED = 0, 1
ENTRY = b"ldpc_hip_syndrome_decode_layered_batch"
FIELDS = ("iterations", "early_term", "msg_bits", "app_bits", "step", "scale", "offset", "flags")


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(lib):
    """Every test of this file, the mirror's included, is about the contract of one entry: without it none has a subject."""
    assert hasattr(lib, "ldpc_hip_syndrome_decode_layered_batch") and hasattr(lib, "ldpc_hip_syndrome_decode_layered_lds_bytes")


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return sdl.Codes(tmp_path_factory.mktemp("sdl"))


def test_symbols_and_signatures(lib):
    import libldpc_amd
    from libldpc_amd import binding
    vp, u64, i32 = ct.c_void_p, ct.c_uint64, ct.c_int
    f = lib.ldpc_hip_syndrome_decode_layered_batch
    assert f.argtypes == [vp, ct.POINTER(binding.ldpc_hip_syndrome_decode_layered), u64, vp, i32, vp, i32, vp, vp, vp, vp, vp] and f.restype == i32
    q = lib.ldpc_hip_syndrome_decode_layered_lds_bytes
    assert q.argtypes == [vp] and q.restype == ct.c_int64
    assert list(binding.ldpc_hip_syndrome_decode_layered._fields_) == [
        ("iterations", ct.c_uint32), ("early_term", ct.c_int), ("msg_bits", ct.c_int), ("app_bits", ct.c_int), ("step", ct.c_double),
        ("scale", ct.c_double), ("offset", ct.c_double), ("flags", ct.c_int)]
    assert ct.sizeof(binding.ldpc_hip_syndrome_decode_layered) == 48  # (16 bytes, three doubles, the flags, padding)
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_syndrome_decode_layered_batch(ldpc_hip_ctx *ctx, const ldpc_hip_syndrome_decode_layered *p, uint64_t n, "
            "const void *llr, int llr_type, const void *syndrome, int syndrome_format, uint32_t *hard_bits, uint32_t *iters, "
            "uint32_t *weight, double *llr_out, void *hip_stream);") in flat
    assert "int64_t ldpc_hip_syndrome_decode_layered_lds_bytes(const ldpc_hip_ctx *ctx);" in flat
    assert ("typedef struct { uint32_t iterations; int early_term; /* 0 / 1 */ int msg_bits; /* 2..8 */ int app_bits; /* msg_bits..16 */ "
            "double step; /* 2^-20 .. 2^20 */ double scale; /* (0, 1] */ double offset; /* [0, 1e6] */ int flags; "
            "/* LDPC_HIP_SYNDROME_SHARED_LLR or 0 */ } ldpc_hip_syndrome_decode_layered;") in flat
    # the flooding entry keeps its layout
    assert ct.sizeof(binding.ldpc_hip_syndrome_decode) == 48 and [n for n, _ in binding.ldpc_hip_syndrome_decode._fields_][2] == "q_bits"
    assert callable(libldpc_amd.HipDecoder.syndrome_decode_layered_batch) and callable(libldpc_amd.HipDecoder.syndrome_decode_layered_lds_bytes)


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
    from libldpc_amd.binding import ldpc_hip_syndrome_decode_layered as Spec
    d = codes.decoder("sd_small")
    llr = np.ones((2, d.nc), np.float64)
    syn = np.zeros((2, d.mc), np.uint8)
    bits, cnt, soft = np.zeros((2, (d.nc + 31) // 32), np.uint32), np.zeros(2, np.uint32), np.zeros((2, d.nc), np.float64)
    err = lib.ldpc_hip_last_error
    good = dict(iterations=5, early_term=1, msg_bits=6, app_bits=8, step=0.25, scale=0.8125, offset=0.0, flags=0)

    def run(n, spec=good, kind=F64, src=llr.ctypes.data, fmt=U8, s=syn.ctypes.data, ctx=None, outs=True):
        p = None if spec is None else ct.byref(Spec(*(spec[k] for k in FIELDS)))
        o = [bits.ctypes.data, cnt.ctypes.data, cnt.ctypes.data, soft.ctypes.data] if outs else [None] * 4
        return lib.ldpc_hip_syndrome_decode_layered_batch(ctx or d.ctx, p, n, src, kind, s, fmt, *o, None)

    def still_taken():
        assert run(0) == 0 and run(0, outs=False) == 0 and run(0, src=None, s=None) == 0

    still_taken()
    nan, inf = float("nan"), float("inf")
    bad = [None]
    bad += [dict(good, msg_bits=v) for v in (-1, 0, 1, 9, 16)]
    bad += [dict(good, app_bits=v) for v in (-1, 0, 5, 17, 32)] + [dict(good, msg_bits=8, app_bits=7)]
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
    for spec in (dict(good, msg_bits=2, app_bits=2), dict(good, msg_bits=8, app_bits=8), dict(good, app_bits=6), dict(good, app_bits=16),
                 dict(good, step=2.0**-20), dict(good, step=2.0**20), dict(good, scale=1.0), dict(good, scale=5e-324), dict(good, offset=1e6),
                 dict(good, early_term=0), dict(good, flags=1), dict(good, iterations=0), dict(good, iterations=2**32 - 1)):
        for kind in (F64, F32, F16, I8):
            for fmt in (U8, PACKED):
                assert run(0, spec, kind, fmt=fmt) == 0 and run(0, spec, kind, fmt=fmt, s=None) == 0, (spec, kind, fmt, err())
    # a code the layered plan does not take is refused before the GPU, frames or none: 65 536 columns; check nodes of degree 20
    big = libldpc_amd.HipDecoder(_big_code(tmp_path_factory.mktemp("sdlbig")))
    wide = codes.decoder("sd_wide")
    for other in (big, wide):
        assert other.syndrome_decode_layered_lds_bytes() == -1 and lib.ldpc_hip_syndrome_decode_layered_lds_bytes(other.ctx) == -1
        ones = np.ones((2, other.nc), np.int8)
        for n in (0, 2):
            assert run(n, kind=I8, src=ones.ctypes.data, s=None, ctx=other.ctx) == -1 and ENTRY in err() and b"65 535" in err(), err()
        with pytest.raises(RuntimeError, match="ldpc_hip_syndrome_decode_layered_batch"):
            other.syndrome_decode_layered_batch(ones[:0])
    assert big.nc == 65536 and wide.syndrome_decode_lds_bytes() > 0  # (the flooding call takes sd_wide)
    still_taken()
    # the binding, n == 0
    for dt in (np.float64, np.float32, np.float16, np.int8):
        r = d.syndrome_decode_layered_batch(np.zeros((0, d.nc), dt), want=sdl.KEYS)
        assert set(r) == set(sdl.KEYS) and r["hard_bits"].shape == (0, (d.nc + 31) // 32) and r["llr_out"].shape == (0, d.nc)
        assert r["llr_out"].dtype == np.float64 and all(r[k].dtype == np.uint32 for k in sdl.KEYS if k != "llr_out")
    assert set(d.syndrome_decode_layered_batch(np.zeros((0, d.nc)))) == {"hard_bits", "iters", "weight"}


def test_binding_refuses_other_dtypes_and_shapes(lib, codes):
    d = codes.decoder("sd_small")
    call = d.syndrome_decode_layered_batch
    words, swords = (d.nc + 31) // 32, (d.mc + 31) // 32
    ok = np.zeros((0, d.nc), np.float32)
    for dt in (np.uint8, np.int16, np.int32, np.int64, np.uint32, np.bool_, np.complex64):
        with pytest.raises(TypeError, match="syndrome_decode_layered_batch"):
            call(np.zeros((1, d.nc), dt))
    for shape in ((1, d.nc + 1), (1, d.nc - 1), (d.nc,), (1, 1, d.nc), (1, words)):
        with pytest.raises(ValueError, match="syndrome_decode_layered_batch"):
            call(np.zeros(shape, np.float64))
    one = np.zeros((1, d.nc), np.float64)
    for dt in (np.int8, np.float32, np.uint16, np.int32, np.uint64):
        with pytest.raises(TypeError, match="syndrome_decode_layered_batch"):
            call(one, np.zeros((1, d.mc), dt))
    for s in (np.zeros((1, d.mc + 1), np.uint8), np.zeros((1, d.mc), np.uint32), np.zeros((1, swords + 1), np.uint32), np.zeros(d.mc, np.uint8),
              np.zeros((2, d.mc), np.uint8), np.zeros((0, swords), np.uint32)):
        with pytest.raises(ValueError, match="syndrome_decode_layered_batch"):
            call(one, s)
    for shape in ((2, d.nc), (d.nc + 1,), (1, 1, d.nc)):
        with pytest.raises(ValueError, match="shared"):
            call(np.zeros(shape), np.zeros((0, d.mc), np.uint8), shared_llr=True)
    with pytest.raises(ValueError, match="shared"):
        call(np.zeros(d.nc), None, shared_llr=True)
    for shape in ((d.nc,), (1, d.nc)):
        assert call(np.zeros(shape), np.zeros((0, swords), np.uint32), shared_llr=True)["iters"].shape == (0,)
    for iterations in (-1, 2**32):
        with pytest.raises(ValueError, match="iterations"):
            call(ok, iterations=iterations)
    with pytest.raises(KeyError):
        call(ok, want=("hard",))
    with pytest.raises(TypeError, match="llr_out"):
        call(ok, want=(), out={"llr_out": np.zeros((0, d.nc), np.float32)})
    with pytest.raises(ValueError, match="hard_bits"):
        call(ok, want=(), out={"hard_bits": np.zeros((0, words + 1), np.uint32)})
    for kw in (dict(msg_bits=9), dict(app_bits=5), dict(app_bits=17), dict(step=0.0), dict(scale=1.5), dict(offset=-1.0)):
        with pytest.raises(RuntimeError, match="ldpc_hip_syndrome_decode_layered_batch"):
            call(ok, **kw)


def _formula(path):
    """The formula of the header from the oracle's restatement of the layered plan; None where the header says -1."""
    code = orc.Code(path)
    degrees, col_degrees = np.bincount(code.edge_row, minlength=code.mc), np.bincount(code.edge_col, minlength=code.nc)
    if degrees.min() < 2 or degrees.max() > 8 or code.nc > 65535 or col_degrees.min() == 0:
        return None
    n, step_of = code.layer_steps()  # (the oracle restates the packing, not what the plan refuses)
    slots = int(((np.bincount(step_of, minlength=n) + 1) // 2 * 2).sum())
    total = ((2 * code.nc + 3) // 4 * 4 + 4 * slots + 128 + 15) // 16 * 16
    return total if total <= 160 * 1024 else None


def test_lds_bytes_formula(lib, codes, h8k_file):
    import libldpc_amd
    seen = {}
    for name in sdl.NAMES:
        d = codes.decoder(name)
        seen[name] = d.syndrome_decode_layered_lds_bytes()
        assert seen[name] == _formula(codes.path(name)) == lib.ldpc_hip_syndrome_decode_layered_lds_bytes(d.ctx), (name, seen[name])
        assert seen[name] == lib.ldpc_hip_layered_fixed_direct_lds_bytes(d.ctx)  # the syndrome costs no byte
    assert seen["golden"] == 6528 and 25 * seen["golden"] <= 160 * 1024 < 26 * seen["golden"]
    assert seen["golden"] < codes.decoder("golden").syndrome_decode_lds_bytes() == 10144  # (the flooding call: 16 frames a CU)
    # sdl_odd: 63 totals in 126 bytes, rounded to 128; 27 check nodes of degree 7, at most 9 to a step (63 columns)
    n_steps, step_of = orc.Code(codes.path("sdl_odd")).layer_steps()
    per_step = np.bincount(step_of, minlength=n_steps)
    assert n_steps >= 3 and per_step.max() <= 9 and seen["sdl_odd"] == (128 + 4 * int(((per_step + 1) // 2 * 2).sum()) + 128 + 15) // 16 * 16
    d8 = libldpc_amd.HipDecoder(h8k_file)
    assert d8.syndrome_decode_layered_lds_bytes() == _formula(h8k_file) == 32896  # four frames a CU
    assert _formula(codes.path("sd_wide")) is None


def test_kernel_resources(lib):
    """kernels_syndrome_decode_layered.hip: one kernel, no scratch, no spills, no static LDS, at most 128 registers."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_syndrome_decode_layered.hip")
    assert res and len(res) == 1 and "syndrome_decode_layered_kernel" in next(iter(res))
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] <= 128 and r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
    # the neighbours are as they were: two instantiations each of the staged and the direct kernel, one flooding kernel
    assert len(build.kernel_resources("kernels_layered_fixed.hip")) == 2 and len(build.kernel_resources("kernels_layered_fixed_direct.hip")) == 2
    assert len(build.kernel_resources("kernels_syndrome_decode.hip")) == 1


# ---- the mirror ----
RUNS = ((sdl.SETTINGS[0], True, 50), (sdl.SETTINGS[0], False, 4), (sdl.SETTINGS[1], True, 1), (sdl.SETTINGS[2], True, 20),
        (sdl.SETTINGS[3], True, 50))


@pytest.mark.parametrize("name", ("sd_r36", "sd_mix", "sd_small", "sdl_odd"))
def test_toward_zero_the_mirror_is_fixed_point_layered_min_sum(codes, name):
    f = codes.frames(name, n=64)
    new, old = codes.mirror(name), LayeredFixedMinSumMirror(orc.Code(codes.path(name)))
    # the LLRs of random words (never a codeword: such frames run to the end) and of the all-zero codeword (most stop)
    llr = np.concatenate((f["llr"][:16], sd.cr.bsc(codes.gf2(name), sdl.POINTS[name][0], sd.NOISE_SEED, np.arange(48), None)[1]))
    stopped = set()
    for (q, p, step, scale, offset), early, iterations in RUNS:
        a = new.decode_toward(llr, None, q, p, step, scale, offset, early, iterations)
        b = old.decode(llr, q, p, step, scale, offset, early, iterations)
        assert np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["hard"], b["hard"]) and np.array_equal(a["llr_out"], b["llr_out"])
        assert np.array_equal(a["total"].astype(np.float64) * step, b["llr_out"])
        assert np.array_equal(a["weight"] == 0, codes.gf2(name).syndrome(a["hard"])[1] == 0)
        stopped |= set((a["iters"] < iterations).tolist())
    assert stopped == {True, False}


@pytest.mark.parametrize("name", ("sd_r36", "sd_small", "sdl_odd"))
def test_toward_a_syndrome_the_mirror_is_that_decoder_on_the_augmented_code(codes, name):
    """Identity (b): [H | I] with 99999.9 (1 - 2 s) on the extra columns, decoded toward zero without early termination, gives
    the same totals and decisions on the first nc columns after any number of sweeps — on a code whose check nodes all have
    degree <= 7 (the augmented plan has the same steps, every degree one larger) and with app_bits > msg_bits (the extra
    column's total, +-Qmax + m, is never clamped, so what it sends is exactly +-Qmax in every sweep)."""
    f = codes.frames(name, n=64)
    code = codes.gf2(name)
    assert np.bincount(code.h_rows).max() <= 7
    new, aug = codes.mirror(name), LayeredFixedMinSumMirror(orc.Code(codes.path(name + "+I")))
    assert (aug.nc, aug.mc, len(aug.steps)) == (code.nc + code.mc, code.mc, len(new.steps))
    assert all(np.array_equal(a[:, :-1], b) and np.array_equal(a[:, -1], code.nc + rows)
               for a, b, rows in zip(aug.steps, (np.sort(c, axis=1) for c in new.steps), new.step_rows))  # the same steps, one column more
    s = np.random.default_rng(3).integers(0, 2, (64, code.mc), dtype=np.uint8)  # any syndrome, reachable or not
    applies = [st for st in sdl.SETTINGS if st[1] > st[0]]
    assert len(applies) == 3 and sdl.SETTINGS[2][:2] == (2, 2)  # (2, 2): Pmax = Qmax, the extra column's total is clamped
    for syn in (f["s"], s):
        wide = np.concatenate((f["llr"], sd.SHORTEN * (1.0 - 2.0 * syn)), axis=1)
        for (q, p, step, scale, offset), iterations in ((applies[0], 1), (applies[0], 7), (applies[1], 5), (applies[2], 12)):
            a = new.decode_toward(f["llr"], syn, q, p, step, scale, offset, False, iterations)
            b = aug.decode(wide, q, p, step, scale, offset, False, iterations)
            assert np.array_equal(a["hard"], b["hard"][:, :code.nc]) and np.array_equal(a["llr_out"], b["llr_out"][:, :code.nc]), (name, q, p)
            assert np.array_equal(a["weight"], (code.syndrome(a["hard"])[0] != syn).sum(1))
    assert (new.decode_toward(f["llr"], s, *sdl.SETTINGS[0], False, 7)["hard"] != new.decode_toward(f["llr"], None, *sdl.SETTINGS[0], False, 7)["hard"]).any()


def test_identity_b_excludes_a_degree_8_check_node_by_rule(codes):
    """sd_mix has check nodes of degree 8: in [H | I] they have degree 9, which the layered plan refuses — the augmented route
    does not exist for such a code, while this entry takes it."""
    code = codes.gf2("sd_mix")
    assert np.bincount(code.h_rows).max() == 8
    assert np.bincount(codes.gf2("sd_mix+I").h_rows).max() == 9
    with pytest.raises(AssertionError):  # (the mirror of that decoder holds the same rule)
        LayeredFixedMinSumMirror(orc.Code(codes.path("sd_mix+I")))
    assert codes.decoder("sd_mix").syndrome_decode_layered_lds_bytes() > 0
    aug = codes.decoder("sd_mix+I")
    assert aug.layered_fixed_lds_bytes() == -1
    with pytest.raises(RuntimeError, match="ldpc_hip_set_min_sum_layered_fixed"):
        aug.set_min_sum_layered_fixed(6, 8, 0.25)
    # what is left to hold the mirror by on this code: the weight is the syndrome distance of the returned word
    f = codes.frames("sd_mix", n=8)
    r = codes.mirror("sd_mix").decode_toward(f["llr"], f["s"], *sdl.SETTINGS[0], False, 3)
    assert np.array_equal(r["weight"], (code.syndrome(r["hard"])[0] != f["s"]).sum(1))


def test_one_sweep_by_hand(tmp_path):
    """Two check nodes over four columns, rows {0, 1, 2} (s = 1) and {1, 2, 3} (s = 0), two steps; int8 input 5, -3, 2, 4 at
    (6, 8, 1.0, 1, 0), so the table is the identity.
    Row 0: t = 5, -3, 2; minima of the others 2, 2, 3; negative others 1, 0, 1, plus s = 1: +2, -2, +3; T = 7, -5, 5, 4.
    Row 1: t = -5, 5, 4; minima 4, 4, 5; negative others 0, 1, 1, plus s = 0: +4, -4, -5; T = 7, -1, 1, -1.
    Decisions 0 1 0 1: row 0 sums to 1 = s, row 1 to 0 = s: met after the first sweep."""
    m = sdl.SyndromeDecodeLayeredMirror(write(tmp_path / "two.txt", [[0, 1, 2], [1, 2, 3]]))
    assert [r.tolist() for r in m.step_rows] == [[0], [1]]
    k = np.array([[5, -3, 2, 4]], np.int8)
    r = m.decode_toward(k, np.array([[1, 0]], np.uint8), 6, 8, 1.0, early_term=True, iterations=50)
    assert r["total"].tolist() == [[7, -1, 1, -1]] and r["hard"].tolist() == [[0, 1, 0, 1]] and r["iters"].tolist() == [0] and r["weight"].tolist() == [0]
    r = m.decode_toward(k, np.array([[1, 0]], np.uint8), 6, 8, 1.0, early_term=False, iterations=1)
    assert r["total"].tolist() == [[7, -1, 1, -1]] and r["iters"].tolist() == [1] and r["llr_out"].tolist() == [[7.0, -1.0, 1.0, -1.0]]
    # toward zero row 0 sends the opposite signs, -2, +2, -3: T = 3, -1, -1, 4; row 1: t = -1, -1, 4 sends -1, -1, +1
    z = m.decode_toward(k, None, 6, 8, 1.0, early_term=False, iterations=1)
    assert z["total"].tolist() == [[3, -2, -2, 5]] and z["hard"].tolist() == [[0, 1, 1, 0]] and z["weight"].tolist() == [0]
    assert m.decode_toward(k, np.array([[1, 0]], np.uint8), 6, 8, 1.0, iterations=0)["weight"].tolist() == [1]  # (0 1 0 0: row 1 sums to 1)


@pytest.mark.parametrize("name", ("sd_small", "sdl_odd", "sd_mix"))
def test_no_iteration_returns_the_quantized_input(codes, name):
    f = codes.frames(name, n=32)
    code = codes.gf2(name)
    for q, p, step, scale, offset in sdl.SETTINGS:
        for early in (True, False):
            zero = codes.mirror(name).decode_toward(f["llr"], f["s"], q, p, step, scale, offset, early, 0)
            L = quantize(f["llr"], q, step)
            assert np.array_equal(zero["total"], L) and np.array_equal(zero["hard"], L <= 0) and not zero["iters"].any()
            assert np.array_equal(zero["llr_out"], L * step) and np.abs(L).max() <= qmax_of(q)
            assert np.array_equal(zero["weight"], (code.syndrome(L <= 0)[0] != f["s"]).sum(1))


@pytest.mark.parametrize("name", sdl.NAMES)
def test_operating_points(codes, name):
    """At POINTS[name] under SETTINGS[0] some frames reach their syndrome and some do not — among the first 64 as well, which
    the GPU tests run the variants on."""
    f = codes.frames(name)
    n = sdl.POINTS[name][1]
    r = codes.mirror(name).decode_toward(f["llr"], f["s"], *sdl.SETTINGS[0])
    reached = r["weight"] == 0
    assert f["llr"].shape[0] == n and int(reached.sum()) == sdl.REACHED[name] and 0 < sdl.REACHED[name] < n
    assert 0 < reached[:64].sum() < 64 and np.array_equal(reached, r["iters"] < 50)
    assert np.array_equal(r["weight"], (codes.gf2(name).syndrome(r["hard"])[0] != f["s"]).sum(1))
