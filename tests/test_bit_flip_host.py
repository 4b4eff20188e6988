"""ldpc_hip_bit_flip_batch and ldpc_hip_bit_flip_lds_bytes (include/ldpc_amd.h) without a GPU: the exported symbols and their
prototypes, everything the call refuses before it touches a device, the binding's own checks, the LDS formula, the
compile-time resources of kernels_bit_flip.hip, and the numpy mirror (tests/bit_flip_ref.py) by itself: one round by hand,
the translation identity, PGDBF's energy restated independently, words that meet their syndrome, prefixes, a threshold of
zero, splits of a batch, and the operating points the GPU tests use."""
import ctypes as ct
import os

import numpy as np
import pytest

import bit_flip_ref as bf
import orc
from minsum_common import write

F64, F32, F16, I8 = 0, 1, 2, 3
U8, PACKED = 0, 1
ENTRY = b"ldpc_hip_bit_flip_batch"
FIELDS = ("iterations", "q_bits", "step", "check_weight", "margin", "flip_threshold", "seed", "first_frame", "flags")


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(lib):
    """Every test of this file, the mirror's included, is about the contract of one entry: without it none has a subject."""
    assert hasattr(lib, "ldpc_hip_bit_flip_batch") and hasattr(lib, "ldpc_hip_bit_flip_lds_bytes")


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return bf.Codes(tmp_path_factory.mktemp("bf"))


def test_symbols_and_signatures(lib):
    import libldpc_amd
    from libldpc_amd import binding
    vp, u64, i32, u32 = ct.c_void_p, ct.c_uint64, ct.c_int, ct.c_uint32
    f = lib.ldpc_hip_bit_flip_batch
    assert f.argtypes == [vp, ct.POINTER(binding.ldpc_hip_bit_flip), u64, vp, i32, vp, i32, vp, vp, vp, vp] and f.restype == i32
    q = lib.ldpc_hip_bit_flip_lds_bytes
    assert q.argtypes == [vp] and q.restype == ct.c_int64
    assert list(binding.ldpc_hip_bit_flip._fields_) == [
        ("iterations", u32), ("q_bits", i32), ("step", ct.c_double), ("check_weight", u32), ("margin", u32), ("flip_threshold", u32),
        ("seed", u64), ("first_frame", u64), ("flags", i32)]
    assert ct.sizeof(binding.ldpc_hip_bit_flip) == 56  # (8, the step, 12 and 4 of padding, two of 8, the flags and padding)
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_bit_flip_batch(ldpc_hip_ctx *ctx, const ldpc_hip_bit_flip *p, uint64_t n, const void *llr, int llr_type, "
            "const void *syndrome, int syndrome_format, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight, void *hip_stream);") in flat
    assert "int64_t ldpc_hip_bit_flip_lds_bytes(const ldpc_hip_ctx *ctx);" in flat
    for field in ("uint32_t iterations;", "int q_bits;", "double step;", "uint32_t check_weight;", "uint32_t margin;",
                  "uint32_t flip_threshold;", "uint64_t seed;", "uint64_t first_frame;", "int flags;"):
        assert field in flat[flat.index("} ldpc_hip_syndrome_decode_layered;"):flat.index("} ldpc_hip_bit_flip;")]
    # the neighbours keep their layouts
    assert ct.sizeof(binding.ldpc_hip_syndrome_decode) == 48 and ct.sizeof(binding.ldpc_hip_syndrome_decode_layered) == 48
    assert callable(libldpc_amd.HipDecoder.bit_flip_batch) and callable(libldpc_amd.HipDecoder.bit_flip_lds_bytes)
    kernel = open(os.path.join(orc.ROOT, "libldpc_amd", "csrc", "device_philox.hpp")).read()
    assert "kTagFlip = 3" in kernel and bf.TAG_FLIP == 3


def _big_code(directory):
    """65 536 columns: check node i lists columns 2 i and 2 i + 1."""
    path = os.path.join(str(directory), "c65536.txt")
    if not os.path.exists(path):
        open(path, "w").write("\n".join(f"{i} {2 * i}\n{i} {2 * i + 1}" for i in range(32768)))
    return path


def test_refusals_come_before_the_gpu(lib, codes, tmp_path_factory):
    """No GPU here: a call that reached the device would fail with another message, or not at all.  After every refusal a
    valid call is taken as before, and no output is touched."""
    import libldpc_amd
    from libldpc_amd.binding import ldpc_hip_bit_flip as Spec
    d = codes.decoder("sd_small")
    llr = np.ones((2, d.nc), np.float64)
    syn = np.zeros((2, d.mc), np.uint8)
    bits, cnt = np.full((2, (d.nc + 31) // 32), 0xA5A5A5A5, np.uint32), np.full(2, 0xA5A5A5A5, np.uint32)
    err = lib.ldpc_hip_last_error
    good = dict(iterations=5, q_bits=2, step=1.0, check_weight=2, margin=0, flip_threshold=0xFFFFFFFF, seed=1, first_frame=0, flags=0)

    def run(n, spec=good, kind=F64, src=llr.ctypes.data, fmt=U8, s=syn.ctypes.data, ctx=None, outs=True):
        p = None if spec is None else ct.byref(Spec(*(spec[k] for k in FIELDS)))
        o = [bits.ctypes.data, cnt.ctypes.data, cnt.ctypes.data] if outs else [None] * 3
        return lib.ldpc_hip_bit_flip_batch(ctx or d.ctx, p, n, src, kind, s, fmt, *o, None)

    def still_taken():
        assert run(0) == 0 and run(0, outs=False) == 0 and run(0, src=None, s=None) == 0
        assert (bits == 0xA5A5A5A5).all() and (cnt == 0xA5A5A5A5).all()

    still_taken()
    nan, inf = float("nan"), float("inf")
    bad = [(None, b"null parameters")]
    bad += [(dict(good, iterations=v), b"iterations") for v in (65536, 100000, 2**32 - 1)]
    bad += [(dict(good, q_bits=v), b"q_bits") for v in (-1, 0, 1, 9, 16)]
    bad += [(dict(good, step=v), b"step") for v in (nan, 0.0, -0.25, 2.0**-21, 2.0**20 * 1.0000001, inf, -inf)]
    bad += [(dict(good, check_weight=v), b"check_weight") for v in (0, 256, 65536, 2**32 - 1)]
    bad += [(dict(good, margin=v), b"margin") for v in (65536, 2**31, 2**32 - 1)]
    bad += [(dict(good, flags=v), b"flag") for v in (2, 3, 4, -1, 1 << 30)]
    for spec, word in bad:
        for n in (0, 2):
            assert run(n, spec) == -1 and ENTRY in err() and word in err(), (spec, n, err())
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
    for spec in (dict(good, q_bits=8), dict(good, step=2.0**-20), dict(good, step=2.0**20), dict(good, check_weight=1),
                 dict(good, check_weight=255), dict(good, margin=65535), dict(good, flip_threshold=0), dict(good, flip_threshold=12345),
                 dict(good, seed=2**64 - 1, first_frame=2**64 - 1), dict(good, flags=1), dict(good, iterations=0),
                 dict(good, iterations=65535)):
        for kind in (F64, F32, F16, I8):
            for fmt in (U8, PACKED):
                assert run(0, spec, kind, fmt=fmt) == 0 and run(0, spec, kind, fmt=fmt, s=None) == 0, (spec, kind, fmt, err())
    # with every output null nothing is launched, frames or none
    assert run(2, outs=False) == 0
    # a code of 65 536 columns is refused before the GPU, frames or none
    big = libldpc_amd.HipDecoder(_big_code(tmp_path_factory.mktemp("bfbig")))
    assert big.nc == 65536 and big.bit_flip_lds_bytes() == -1 and lib.ldpc_hip_bit_flip_lds_bytes(big.ctx) == -1
    ones = np.ones((2, big.nc), np.int8)
    for n in (0, 2):
        assert run(n, kind=I8, src=ones.ctypes.data, s=None, ctx=big.ctx) == -1 and ENTRY in err() and b"65 535" in err(), err()
    with pytest.raises(RuntimeError, match="ldpc_hip_bit_flip_batch"):
        big.bit_flip_batch(ones[:0])
    still_taken()
    # the binding, n == 0
    for dt in (np.float64, np.float32, np.float16, np.int8):
        r = d.bit_flip_batch(np.zeros((0, d.nc), dt))
        assert set(r) == set(bf.KEYS) and r["hard_bits"].shape == (0, (d.nc + 31) // 32) and all(r[k].dtype == np.uint32 for k in bf.KEYS)
    assert set(d.bit_flip_batch(np.zeros((0, d.nc)), want=("iters",))) == {"iters"}


def test_binding_refuses_other_dtypes_and_shapes(lib, codes):
    d = codes.decoder("sd_small")
    call = d.bit_flip_batch
    words, swords = (d.nc + 31) // 32, (d.mc + 31) // 32
    ok = np.zeros((0, d.nc), np.float32)
    for dt in (np.uint8, np.int16, np.int32, np.int64, np.uint32, np.bool_, np.complex64):
        with pytest.raises(TypeError, match="bit_flip_batch"):
            call(np.zeros((1, d.nc), dt))
    for shape in ((1, d.nc + 1), (1, d.nc - 1), (d.nc,), (1, 1, d.nc), (1, words)):
        with pytest.raises(ValueError, match="bit_flip_batch"):
            call(np.zeros(shape, np.float64))
    one = np.zeros((1, d.nc), np.float64)
    for dt in (np.int8, np.float32, np.uint16, np.int32, np.uint64):
        with pytest.raises(TypeError, match="bit_flip_batch"):
            call(one, np.zeros((1, d.mc), dt))
    for s in (np.zeros((1, d.mc + 1), np.uint8), np.zeros((1, d.mc), np.uint32), np.zeros((1, swords + 1), np.uint32), np.zeros(d.mc, np.uint8),
              np.zeros((2, d.mc), np.uint8), np.zeros((0, swords), np.uint32)):
        with pytest.raises(ValueError, match="bit_flip_batch"):
            call(one, s)
    with pytest.raises(ValueError, match="shared"):
        call(np.zeros(d.nc), None, shared_llr=True)
    for shape in ((d.nc,), (1, d.nc)):
        assert call(np.zeros(shape), np.zeros((0, swords), np.uint32), shared_llr=True)["iters"].shape == (0,)
    for kw in (dict(iterations=-1), dict(iterations=2**32), dict(flip_prob=-0.1), dict(flip_prob=1.5), dict(check_weight=-1), dict(margin=2**32),
               dict(seed=-1), dict(seed=2**64), dict(first_frame=2**64), dict(want=("llr_out",))):
        with pytest.raises(ValueError, match="bit_flip_batch"):
            call(ok, **kw)
    with pytest.raises(KeyError):
        call(ok, want=("hard",))
    with pytest.raises(ValueError, match="hard_bits"):
        call(ok, want=(), out={"hard_bits": np.zeros((0, words + 1), np.uint32)})
    with pytest.raises(TypeError):
        call(ok, None, 5)  # (the settings are keyword-only)
    for kw in (dict(q_bits=9), dict(q_bits=1), dict(step=0.0), dict(check_weight=0), dict(check_weight=256), dict(margin=65536),
               dict(iterations=65536)):
        with pytest.raises(RuntimeError, match="ldpc_hip_bit_flip_batch"):
            call(ok, **kw)
    assert bf.threshold_of(1.0) == 0xFFFFFFFF and bf.threshold_of(0.0) == 0 and bf.threshold_of(0.5) == 2**31
    assert bf.threshold_of(0.7) == int(0.7 * 2.0**32) == 3006477107


def _formula(path):
    """The formula of the header from the code file alone; None where the header says -1."""
    rows, cols = [], []
    for line in open(path).read().split("\n"):
        parts = line.split()
        if ":" not in line and len(parts) >= 2:
            rows.append(int(parts[0])), cols.append(int(parts[1]))
    mc, nc = max(rows) + 1, max(cols) + 1
    if nc > 65535 or mc > 65535:
        return None
    r16 = lambda v: (v + 15) // 16 * 16
    total = r16(nc) + r16(4 * ((nc + 31) // 32)) + 2 * r16(4 * ((mc + 31) // 32))
    return total if total <= 160 * 1024 else None


def test_lds_bytes_formula(lib, codes, h8k_file, tmp_path):
    import libldpc_amd
    seen = {}
    for name in bf.NAMES:
        d = codes.decoder(name)
        seen[name] = d.bit_flip_lds_bytes()
        assert seen[name] == _formula(codes.path(name)) == lib.ldpc_hip_bit_flip_lds_bytes(d.ctx), (name, seen[name])
    assert seen["golden"] == 1152 + 144 + 2 * 128 and seen["sd_small"] == 48 + 16 + 2 * 16
    assert seen["golden"] < codes.decoder("golden").syndrome_decode_layered_lds_bytes() == 6528
    d8 = libldpc_amd.HipDecoder(h8k_file)
    assert d8.bit_flip_lds_bytes() == _formula(h8k_file) == 8192 + 1024 + 2 * 512
    assert _formula(_big_code(tmp_path)) is None and libldpc_amd.HipDecoder(_big_code(tmp_path)).bit_flip_lds_bytes() == -1
    # 65 535 columns and as many check nodes are taken: 65 536 + 8 192 + 2 * 8 192 bytes
    edge = os.path.join(str(tmp_path), "c65535.txt")
    open(edge, "w").write("\n".join(f"{i} {i}\n{i} {(i + 1) % 65535}" for i in range(65535)))
    assert libldpc_amd.HipDecoder(edge).bit_flip_lds_bytes() == _formula(edge) == 65536 + 8192 + 2 * 8192


def test_kernel_resources(lib):
    """kernels_bit_flip.hip: one kernel, no scratch, no spills, no static LDS, and registers for eight waves a SIMD."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_bit_flip.hip")
    assert res and len(res) == 1 and "bit_flip_kernel" in next(iter(res))
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] <= 64 and r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
    assert len(build.kernel_resources("kernels_syndrome_decode_layered.hip")) == 1 and len(build.kernel_resources("kernels_syndrome_decode.hip")) == 1


# ---- the mirror ----
def test_one_round_by_hand(tmp_path):
    """Three check nodes over five columns: rows {0, 1, 2}, {1, 2, 3}, {3, 4}; column 4's entry in row 2 is listed twice more
    below.  int8 input 3, -1, 2, -2, 1 at q_bits = 3 (Qmax = 3), w = 4: y = 0 1 0 1 0, r = 3 1 2 2 1.
    s = 0 0 0: u = (1, 0, 1); U = 1 1 1 1 1; P = 4 - 3, 4 - 1, 4 - 2, 4 - 2, 4 - 1 = 1 3 2 2 3: columns 1 and 4 flip
    (margin 0) -> x = 0 0 0 1 1: u = (0, 1, 0); U = 0 1 1 1 0; P = -3, 4 + 1, 4 - 2, 4 - 2, 0 + 1 = -3 5 2 2 1: column 1 flips
    back: a cycle of period two.  With margin 1 in round 0 columns 1, 2, 3, 4 flip -> x = 0 0 1 0 1: u = (1, 1, 1)."""
    m = bf.BitFlipMirror(write(tmp_path / "three.txt", [[0, 1, 2], [1, 2, 3], [3, 4]]))
    k = np.array([[3, -1, 2, -2, 1]], np.int8)
    trace = []
    r = m.decode(k, None, 2, 3, 1.0, 4, 0, trace=trace)
    assert trace[0][2].tolist() == [[1, 3, 2, 2, 3]] and trace[0][3].astype(int).tolist() == [[0, 1, 0, 0, 1]]
    assert trace[1][2].tolist() == [[-3, 5, 2, 2, 1]] and trace[1][3].astype(int).tolist() == [[0, 1, 0, 0, 0]]
    assert r["hard"].tolist() == [[0, 1, 0, 1, 1]] and r["iters"].tolist() == [2] and r["weight"].tolist() == [1]
    r = m.decode(k, None, 1, 3, 1.0, 4, 1)
    assert r["hard"].tolist() == [[0, 0, 1, 0, 1]] and r["weight"].tolist() == [3] and r["iters"].tolist() == [1]
    # toward s = 1 0 1 the input's decisions are a solution: nothing runs
    r = m.decode(k, np.array([[1, 0, 1]], np.uint8), 50, 3, 1.0, 4, 0)
    assert r["hard"].tolist() == [[0, 1, 0, 1, 0]] and r["iters"].tolist() == [0] and r["weight"].tolist() == [0]
    # the clamp of item 1: at q_bits = 2 every magnitude is 1
    trace = []
    m.decode(k, None, 1, 2, 1.0, 4, 0, trace=trace)
    assert trace[0][2].tolist() == [[3, 3, 3, 3, 3]]
    # an entry listed twice counts twice in u (it cancels) and adds twice in U
    dup = bf.BitFlipMirror(write(tmp_path / "dup.txt", [[0, 1, 2], [1, 2, 3], [3, 4, 4, 4]]))
    trace = []
    dup.decode(k, None, 1, 3, 1.0, 4, 0, trace=trace)
    assert trace[0][2].tolist() == [[1, 3, 2, 2, 11]]  # u = (1, 0, 1) as before (three times = once), U[4] = 3


def _random_case(code, n, qmax, seed):
    rng = np.random.default_rng(seed)
    k = (rng.integers(1, qmax + 1, (n, code.nc)) * (1 - 2 * rng.integers(0, 2, (n, code.nc)))).astype(np.int8)
    noise = (rng.random((n, code.nc)) < 0.03).astype(np.uint8)
    return k, noise


@pytest.mark.parametrize("name", ("sd_r36", "sd_mix", "sd_small", "s40x60_hdup"))
def test_translation(codes, name):
    """(a): on frames without a quantized zero, decoding L (1 - 2 x0) toward s XOR H x0 returns the word of (L, s) XOR x0,
    with the same iters and weight, in both modes: the draws depend on (frame, round, column) alone."""
    code, m = codes.gf2(name), codes.mirror(name)
    n = 24
    rng = np.random.default_rng(11)
    x0 = rng.integers(0, 2, (n, code.nc), dtype=np.uint8)
    for q_bits, w, margin, thr in ((2, 2, 0, bf.EVERY_CANDIDATE), (2, 2, 0, bf.threshold_of(0.7)), (6, 16, 4, bf.EVERY_CANDIDATE),
                                   (4, 5, 2, bf.threshold_of(0.4))):
        k, noise = _random_case(code, n, (1 << (q_bits - 1)) - 1, 5)
        assert (k != 0).all()
        # the frame: the all-zero word with `noise` flipped, read through reliabilities |k|, toward s = 0
        L = (np.abs(k).astype(np.int64) * (1 - 2 * noise.astype(np.int64))).astype(np.int8)
        a = m.decode(L, None, 30, q_bits, 1.0, w, margin, thr, bf.SEED, 100)
        moved = (L.astype(np.int64) * (1 - 2 * x0.astype(np.int64))).astype(np.int8)
        b = m.decode(moved, code.syndrome(x0)[0], 30, q_bits, 1.0, w, margin, thr, bf.SEED, 100)
        assert np.array_equal(b["hard"], a["hard"] ^ x0) and np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["weight"], b["weight"])
        assert (a["iters"] > 0).any()


@pytest.mark.parametrize("name", ("sd_r36", "sd_small", "s40x60_hdup"))
def test_flip_sets_are_pgdbf(codes, name):
    """(b): with +-1 inputs, w = 2 and margin 0 the flips of every round are the columns of the largest energy "unsatisfied
    neighbours + disagreement with the channel", restated here entry by entry."""
    code, m = codes.gf2(name), codes.mirror(name)
    f = codes.hard_frames(name)
    n = 12
    trace = []
    m.decode(f["k"][:n], f["s"][:n], 6, 2, 1.0, 2, 0, trace=trace)
    y = (f["k"][:n] <= 0).astype(int)
    x = y.copy()
    assert len(trace) >= 3
    for t, active, _, flips in trace:
        for i, frame in enumerate(active):
            unsat = [0] * code.mc
            for r, c in zip(code.h_rows, code.h_cols):
                unsat[r] ^= x[frame][c]
            unsat = [int(u ^ s) for u, s in zip(unsat, f["s"][frame])]
            energy = [int(x[frame][c] != y[frame][c]) for c in range(code.nc)]
            for r, c in zip(code.h_rows, code.h_cols):
                energy[c] += unsat[r]
            assert np.array_equal(flips[i], np.asarray(energy) == max(energy)), (t, frame)
            x[frame] ^= flips[i]


@pytest.mark.parametrize("name", ("sd_mix", "golden"))
def test_a_word_that_meets_s_returns_unchanged(codes, name):
    """(c): whatever `iterations` is, and whatever the settings are."""
    code, m = codes.gf2(name), codes.mirror(name)
    x = codes.frames(name, 0.01, 16)["x"]
    k = (1 - 2 * x.astype(np.int64)).astype(np.int8)
    for iterations in (0, 1, 50, 65535):
        for thr in (bf.EVERY_CANDIDATE, bf.threshold_of(0.7)):
            r = m.decode(k, code.syndrome(x)[0], iterations, 2, 1.0, 2, 3, thr, bf.SEED)
            assert np.array_equal(r["hard"], x) and not r["iters"].any() and not r["weight"].any()


@pytest.mark.parametrize("name", ("sd_r36", "sd_wide", "golden"))
def test_prefix(codes, name):
    """(d): a run of k rounds agrees with a longer one on every frame that finished within k; on the others iters = k.  And
    item 7: no round returns the quantized input's decisions."""
    code, m = codes.gf2(name), codes.mirror(name)
    f = codes.hard_frames(name, 48)
    for margin, thr in ((bf.POINTS[name][1], bf.EVERY_CANDIDATE), (0, bf.threshold_of(0.7))):
        full = m.decode(f["llr"], f["s"], 40, 2, f["step"], 2, margin, thr, bf.SEED)
        for k in (0, 1, 7, 20):
            part = m.decode(f["llr"], f["s"], k, 2, f["step"], 2, margin, thr, bf.SEED)
            within = full["iters"] <= k
            assert np.array_equal(part["hard"][within], full["hard"][within]) and not full["weight"][within].any()
            assert np.array_equal(part["iters"][within], full["iters"][within]) and (part["iters"][~within] == k).all()
            assert np.array_equal(part["weight"], (code.syndrome(part["hard"])[0] != f["s"]).sum(1))
            if k == 0:
                assert np.array_equal(part["hard"], f["llr"] <= 0) and not part["iters"].any()
        assert 0 < (full["iters"] <= 7).sum() < 48 or name == "golden"


def test_a_threshold_of_zero_flips_nothing(codes):
    """(e): every round counts, none flips."""
    m = codes.mirror("sd_r36")
    f = codes.hard_frames("sd_r36", 16)
    r = m.decode(f["k"], f["s"], 9, 2, 1.0, 2, 0, 0, bf.SEED)
    zero = m.decode(f["k"], f["s"], 0, 2, 1.0, 2, 0)
    assert np.array_equal(r["hard"], zero["hard"]) and np.array_equal(r["weight"], zero["weight"])
    assert np.array_equal(r["iters"], np.where(zero["weight"] == 0, 0, 9)) and (zero["weight"] > 0).any()
    one = m.decode(f["k"], f["s"], 9, 2, 1.0, 2, 0, 1, bf.SEED)  # (a draw below 1 is a draw of 0)
    assert np.array_equal(one["hard"], zero["hard"])


@pytest.mark.parametrize("name", ("sd_r36", "s40x60_hdup"))
def test_a_split_with_first_frame_reproduces_the_batch(codes, name):
    """(f), and what it rests on: the draws are the tag-3 words of (seed, frame, block), and another first_frame or seed
    gives other words."""
    m = codes.mirror(name)
    f = codes.hard_frames(name, 40)
    args = (30, 2, 1.0, 2, 0, bf.threshold_of(0.7), bf.SEED)
    whole = m.decode(f["k"], f["s"], *args, 1000)
    for cut in (1, 17, 39):
        a, b = m.decode(f["k"][:cut], f["s"][:cut], *args, 1000), m.decode(f["k"][cut:], f["s"][cut:], *args, 1000 + cut)
        for key in ("hard", "iters", "weight"):
            assert np.array_equal(np.concatenate((a[key], b[key])), whole[key]), (cut, key)
    assert (m.decode(f["k"], f["s"], *args, 0)["hard"] != whole["hard"]).any()
    assert (m.decode(f["k"], f["s"], *args[:-1], bf.SEED + 1, 1000)["hard"] != whole["hard"]).any()
    w = bf.draws(bf.SEED, [1000, 2**40 + 3], 2, m.nc)
    per_round = (m.nc + 3) // 4
    ref = bf.philox_ref.blocks(bf.SEED, 3, [1000, 2**40 + 3], 2 * per_round + np.arange(per_round))
    assert w.shape == (2, m.nc) and all(w[i, v] == ref[i, v >> 2, v & 3] for i in range(2) for v in (0, 1, 5, m.nc - 1))


@pytest.mark.parametrize("name", bf.NAMES)
def test_operating_points(codes, name):
    """Both kinds of frame occur under every setting of the GPU tests — among the first 67 frames too — except under
    margin 0 on "golden", the degenerate case: its punctured columns tie and flip together, and no frame reaches s."""
    code, m = codes.gf2(name), codes.mirror(name)
    eps, margin, reached = bf.POINTS[name]
    f = codes.hard_frames(name)
    assert f["llr"].shape[0] == bf.N and np.array_equal(np.abs(f["k"]), np.abs(f["llr"]) > 0)

    def both(frames, r, count=None):
        ok = r["weight"] == 0
        assert np.array_equal(r["weight"], (code.syndrome(r["hard"])[0] != frames["s"]).sum(1))
        assert (count is None or int(ok.sum()) == count) and 0 < ok.sum() < bf.N and 0 < ok[:67].sum() < 67, int(ok.sum())
        assert (r["iters"][~ok] == bf.ROUNDS).all() and (r["iters"][ok] > 0).any()

    both(f, m.decode(f["llr"], f["s"], bf.ROUNDS, 2, f["step"], 2, margin), reached)
    if name == "golden":
        none = m.decode(f["llr"], f["s"], bf.ROUNDS, 2, f["step"], 2, 0)
        assert (none["weight"] > 0).all() and (none["iters"] == bf.ROUNDS).all() and len(code.puncture) == 128
    g = codes.hard_frames(name, eps=bf.PROB_POINTS[name])
    both(g, m.decode(g["llr"], g["s"], bf.ROUNDS, 2, g["step"], 2, 0, bf.threshold_of(0.7), bf.SEED))
    a = codes.soft_frames(name)
    w, margin, _, q_bits, step = bf.SOFT_SETTING
    both(a, m.decode(a["llr"], a["s"], bf.ROUNDS, q_bits, step, w, margin), bf.SOFT_REACHED[name])
