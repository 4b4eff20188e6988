"""ldpc_hip_erasure_solve_batch and ldpc_hip_erasure_solve_lds_bytes (include/ldpc_amd.h) without a GPU: the exported symbols
and their prototypes, everything the call refuses before it touches a device, the binding's own checks, the LDS formula, the
numpy mirror (tests/erasure_ml_ref.py) against enumeration from the definition, the mirror against peeling, and the
compile-time resources of kernels_erasure_solve.hip."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

import erasure_ml_ref as ml
import erasure_ref as er
import generator_codes as gc
import gf2_ref
import orc

U8, PACKED32 = 0, 1
SOLVE = b"ldpc_hip_erasure_solve_batch"
KEYS = ("word", "erased", "unresolved", "rank", "status")


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(lib):
    """Every test of this file, the mirror's included, is about the contract of one entry: without it none has a subject."""
    assert hasattr(lib, "ldpc_hip_erasure_solve_batch") and hasattr(lib, "ldpc_hip_erasure_solve_lds_bytes")


def _regular(directory, nc, seed=1):
    sys.path.insert(0, os.path.join(orc.ROOT, "tools"))
    import gen_regular_code
    path = os.path.join(str(directory), f"r{nc}.h.txt")
    if not os.path.exists(path):
        open(path, "w").write(gen_regular_code.generate(nc, 3, 6, seed))
    return path, ""


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("erasure_solve")
    out = {"golden": (orc.H_TXT, orc.G_TXT), "r240": _regular(d, 240), "r14000": _regular(d, 14000)}
    for name in ("s40x60", "s129x150t5", "s800x100"):
        out[name] = gc.write_pair(d, name)
    out["s40x60_hdup"] = (er.repeat_entries(out["s40x60"][0], os.path.join(str(d), "s40x60_hdup.h.txt")), "")  # parallel edges in H
    return out


def test_symbols_and_signatures(lib):
    vp, u64, u32, i32 = ct.c_void_p, ct.c_uint64, ct.c_uint32, ct.c_int
    assert lib.ldpc_hip_erasure_solve_batch.argtypes == [vp, u32, u64, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    assert lib.ldpc_hip_erasure_solve_batch.restype == i32
    assert lib.ldpc_hip_erasure_solve_lds_bytes.argtypes == [vp, u32] and lib.ldpc_hip_erasure_solve_lds_bytes.restype == ct.c_int64
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_erasure_solve_batch(ldpc_hip_ctx *ctx, uint32_t max_unknowns, uint64_t n, const void *word, "
            "const void *erased, int format, uint32_t *word_out, uint32_t *erased_out, uint32_t *unresolved, uint32_t *rank, "
            "uint32_t *status, void *hip_stream);") in flat
    assert "int64_t ldpc_hip_erasure_solve_lds_bytes(const ldpc_hip_ctx *ctx, uint32_t max_unknowns);" in flat
    assert ("LDPC_HIP_ERASURE_SOLVED = 0, LDPC_HIP_ERASURE_PARTIAL = 1, LDPC_HIP_ERASURE_INCONSISTENT = 2, "
            "LDPC_HIP_ERASURE_TOO_LARGE = 3") in flat
    import libldpc_amd
    d = libldpc_amd.HipDecoder
    assert (d.ERASURE_SOLVED, d.ERASURE_PARTIAL, d.ERASURE_INCONSISTENT, d.ERASURE_TOO_LARGE) == (ml.SOLVED, ml.PARTIAL, ml.INCONSISTENT, ml.TOO_LARGE)


def test_refusals_come_before_the_gpu(lib, files):
    """No GPU here: a call that reached the device would fail with another message, or not at all."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(*files["s129x150t5"])
    words = (d.nc + 31) // 32
    a, b = np.zeros((2, words), np.uint32), np.zeros((2, words), np.uint32)
    cnt = np.zeros(2, np.uint32)
    err = lib.ldpc_hip_last_error

    def solve(n, cap=64, fmt=PACKED32, word=a.ctypes.data, erased=b.ctypes.data, ctx=None, outs=True):
        o = [a.ctypes.data, b.ctypes.data, cnt.ctypes.data, cnt.ctypes.data, cnt.ctypes.data] if outs else [None] * 5
        return lib.ldpc_hip_erasure_solve_batch(ctx or d.ctx, cap, n, word, erased, fmt, *o, None)

    for n in (0, 2):
        for what, kw in {"format 2": dict(fmt=2), "format -1": dict(fmt=-1), "cap 0": dict(cap=0), "cap 0, bytes": dict(cap=0, fmt=U8)}.items():
            assert solve(n, **kw) == -1 and SOLVE in err(), (n, what, err())
    assert solve(2, word=None) == -1 and SOLVE in err() and solve(2, erased=None) == -1 and SOLVE in err()
    # after the checks n == 0 returns 0 (no GPU needed): every format, a cap above nc, with and without buffers
    for fmt in (U8, PACKED32):
        for cap in (1, 64, d.nc, d.nc + 1, 2**32 - 1):
            assert solve(0, cap, fmt) == 0 and solve(0, cap, fmt, None, None) == 0 and solve(0, cap, fmt, outs=False) == 0
    # a code and cap whose frame does not fit is refused before the GPU, frames or none; a small cap on the same code is taken
    big = libldpc_amd.HipDecoder(*files["r14000"])
    assert big.erasure_solve_lds_bytes(14000) == -1 and big.erasure_solve_lds_bytes(64) > 0
    wide = np.zeros((2, (14000 + 31) // 32), np.uint32)
    for n in (0, 2):
        assert solve(n, 14000, word=wide.ctypes.data, erased=wide.ctypes.data, ctx=big.ctx) == -1 and SOLVE in err() and b"LDS" in err()
    assert solve(0, 64, ctx=big.ctx) == 0
    with pytest.raises(RuntimeError, match="ldpc_hip_erasure_solve_batch"):
        big.erasure_solve_batch(wide[:0], wide[:0], max_unknowns=14000)
    with pytest.raises(RuntimeError, match="max_unknowns"):
        d.erasure_solve_batch(a[:0], b[:0], max_unknowns=0)
    # the binding, n == 0: the default cap is the largest that fits
    assert d.erasure_solve_max_unknowns() == d.nc
    cap = big.erasure_solve_max_unknowns()
    assert 0 < cap < 14000 and big.erasure_solve_lds_bytes(cap) > 0 and big.erasure_solve_lds_bytes(cap + 1) == -1
    for dec, rows in ((d, np.zeros((0, d.nc), np.uint8)), (big, wide[:0])):
        r = dec.erasure_solve_batch(rows, rows)
        assert set(r) == set(KEYS) and r["word"].shape == (0, (dec.nc + 31) // 32) and r["status"].shape == (0,)
        assert all(v.dtype == np.uint32 for v in r.values())


def test_binding_refuses_other_dtypes_and_shapes(lib, files):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(*files["s40x60"])
    words = (d.nc + 31) // 32
    u8, pk = np.zeros((1, d.nc), np.uint8), np.zeros((1, words), np.uint32)
    for dt in (np.int8, np.int32, np.uint16, np.float32, np.bool_):
        with pytest.raises(TypeError, match="erasure_solve_batch"):
            d.erasure_solve_batch(np.zeros((1, d.nc), dt), u8)
        with pytest.raises(TypeError, match="erasure_solve_batch"):
            d.erasure_solve_batch(u8, np.zeros((1, d.nc), dt))
    with pytest.raises(ValueError, match="erasure_solve_batch"):
        d.erasure_solve_batch(u8, pk)  # both operands in one format
    with pytest.raises(ValueError, match="erasure_solve_batch"):
        d.erasure_solve_batch(pk, np.zeros((2, words), np.uint32))
    with pytest.raises(ValueError, match="erasure_solve_batch"):
        d.erasure_solve_batch(np.zeros((1, d.nc + 1), np.uint8), np.zeros((1, d.nc + 1), np.uint8))
    with pytest.raises(ValueError, match="erasure_solve_batch"):
        d.erasure_solve_batch(np.zeros((1, d.nc), np.uint32), np.zeros((1, d.nc), np.uint32))  # packed rows are ceil(nc / 32) words
    with pytest.raises(ValueError, match="max_unknowns"):
        d.erasure_solve_batch(pk[:0], pk[:0], max_unknowns=-1)
    with pytest.raises(KeyError):
        d.erasure_solve_batch(pk[:0], pk[:0], want=("iters",))
    with pytest.raises(TypeError, match="rank"):
        d.erasure_solve_batch(pk[:0], pk[:0], want=(), out={"rank": np.zeros(0, np.int64)})
    with pytest.raises(ValueError, match="status"):
        d.erasure_solve_batch(pk[:0], pk[:0], want=(), out={"status": np.zeros(1, np.uint32)})
    with pytest.raises(ValueError, match="erased"):
        d.erasure_solve_batch(u8, u8, want=(), out={"erased": np.zeros((2, words), np.uint32)})


def _formula(code, max_unknowns):
    """The formula of the header, restated; None where the header says -1."""
    if max_unknowns == 0:
        return None
    u = min(max_unknowns, code.nc)
    d = int(np.bincount(code.h_cols).max())
    r = min(code.mc, u * d)
    s = -(-(u + 1) // 64) | 1
    w = -(-code.nc // 32)
    total = -(-(8 * r * s + 12 * -(-code.mc // 64) + 4 * (3 * w + 1) + 4 * u + 64) // 16) * 16
    return total if total <= 160 * 1024 else None


def test_lds_bytes_formula(lib, files):
    import libldpc_amd
    golden = gf2_ref.Gf2Code(*files["golden"])
    dec = libldpc_amd.HipDecoder(*files["golden"])
    assert (golden.nc, golden.mc) == (1152, 1024) and int(np.bincount(golden.h_cols).max()) == 15
    assert _formula(golden, 1024) == 144064 == dec.erasure_solve_lds_bytes(1024)  # 8 * 1024 * 17 + 192 + 436 + 4096 + 64, rounded up
    assert dec.erasure_solve_lds_bytes(0) == -1
    assert dec.erasure_solve_lds_bytes(1152) == dec.erasure_solve_lds_bytes(5000) == dec.erasure_solve_lds_bytes(2**32 - 1) == _formula(golden, 1152)
    caps = {"golden": (1, 2, 63, 64, 68, 69, 127, 128, 1023, 1024, 1025, 1151, 1152, 1153), "s40x60": (1, 13, 14, 20, 21, 63, 64, 100, 101),
            "s40x60_hdup": (1, 11, 12, 13, 100), "s129x150t5": (1, 49, 50, 51, 284), "s800x100": (1, 33, 34, 900),
            "r240": (1, 16, 39, 40, 41, 240), "r14000": (1, 16, 63, 64, 127, 128, 191, 192, 400, 2333, 2334, 7000, 14000)}
    refused = 0
    for name, points in caps.items():
        code, d = gf2_ref.Gf2Code(*files[name]), libldpc_amd.HipDecoder(*files[name])
        for cap in points:
            want = _formula(code, cap)
            assert d.erasure_solve_lds_bytes(cap) == (-1 if want is None else want), (name, cap)
            refused += want is None
        sizes = [_formula(code, cap) for cap in range(1, code.nc + 1, 1 if code.nc < 2000 else 37)]
        fits = [s for s in sizes if s is not None]
        assert fits == sorted(fits) and all(s is None for s in sizes[len(fits):]), name  # monotone; once refused, refused
    assert refused >= 3  # (r14000 at the larger caps)
    # the bound on the rows keeps a sparse code of many check nodes in range: 7000 check nodes, 64 unknowns, 192 rows
    big = gf2_ref.Gf2Code(*files["r14000"])
    assert _formula(big, 14000) is None and _formula(big, 7000) is None and _formula(big, 192) is not None
    assert _formula(big, 64) == -(-(8 * 192 * 3 + 12 * 110 + 4 * (3 * 438 + 1) + 4 * 64 + 64) // 16) * 16 < 16 * 1024


CASES = ("s40x60", "s40x60_hdup", "s129x150t5")


def _small_frames(code, seed, eps):
    """60 frames with |E| <= 14: erasures of a codeword (the all-zero one, or an encoded one), of random words, on random
    columns and on the columns of single check nodes (dependent columns: undetermined bits); one frame without erasures that
    is a codeword and one that is none; ten frames that peeling could not finish."""
    rng = np.random.default_rng(seed)
    n = 60
    w = np.zeros((n, code.nc), np.uint8)
    if code.has_g:
        w[:20] = code.encode(rng.integers(0, 2, (20, code.kc), dtype=np.uint8))
    w[20:] = rng.integers(0, 2, (n - 20, code.nc))
    w[40:50] = 0
    e = np.zeros((n, code.nc), np.uint8)
    for f in range(n):
        if f % 3 == 2:  # the columns of a check node, and some more
            cols = code.h_cols[code.h_rows == rng.integers(code.mc)]
            cols = np.union1d(cols[:12], rng.choice(code.nc, 2, replace=False))
        else:
            cols = rng.choice(code.nc, rng.integers(1, 15), replace=False)
        e[f, cols] = 1 + rng.integers(0, 255)
    # what peeling leaves of a codeword with erasures: stopping sets, where a codeword hides among the erased columns
    cw = code.encode(rng.integers(0, 2, (200, code.kc), dtype=np.uint8)) if code.has_g else None
    left = er.decode(code, *er.channel(code, eps, 31, np.arange(200), cw), 50, er.EARLY_TERM | er.STOP_STALLED)
    keep = np.flatnonzero((left["unresolved"] > 0) & (left["unresolved"] <= 14))[:10]
    assert keep.size == 10
    w[48:58], e[48:58] = left["word"][keep], left["erased"][keep]
    e[58:] = 0
    w[58] = 0
    w[59, 0] ^= 1
    assert e.astype(bool).sum(1).max() <= 14
    return w, e


@pytest.mark.parametrize("name", CASES)
def test_mirror_equals_enumeration(files, name):
    code = gf2_ref.Gf2Code(*files[name])
    seen = set()
    for cap in (14, 9):
        w, e = _small_frames(code, 11, {"s40x60": 0.4, "s40x60_hdup": 0.4, "s129x150t5": 0.35}[name])
        got, want = ml.solve(code, w, e, cap), ml.solve_by_enumeration(code, w, e, cap)
        for key in KEYS:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (name, cap, key)
        seen |= set(got["status"].tolist())
        status, ne = got["status"], (e != 0).sum(1)
        assert np.array_equal(status == ml.TOO_LARGE, ne > cap)
        back = (status == ml.INCONSISTENT) | (status == ml.TOO_LARGE)  # returned as they came
        assert np.array_equal(got["erased"][back], gf2_ref.pack(e)[back]) and np.array_equal(got["word"][back], gf2_ref.pack((w != 0) & (e == 0))[back])
        assert not got["rank"][status == ml.TOO_LARGE].any() and np.array_equal(got["unresolved"][back], ne[back])
        assert (got["unresolved"][status == ml.SOLVED] == 0).all() and (got["unresolved"][status == ml.PARTIAL] > 0).all()
        assert not (got["word"] & got["erased"]).any() and not gf2_ref.high_bits(got["word"] | got["erased"], code.nc).any()
        assert (got["status"][58], got["rank"][58]) == (ml.SOLVED, 0) and (got["status"][59], got["rank"][59]) == (ml.INCONSISTENT, 0)
    assert seen == {ml.SOLVED, ml.PARTIAL, ml.INCONSISTENT, ml.TOO_LARGE}, (name, seen)


def test_an_entry_listed_twice_cancels(files):
    """The one place where the solver and the peeling decoder read H differently."""
    plain, dup = gf2_ref.Gf2Code(*files["s40x60"]), gf2_ref.Gf2Code(*files["s40x60_hdup"])
    twice = np.argwhere(er.incidence(dup) == 2)
    assert twice.shape == (1, 2) and er.incidence(dup).max() == 3
    r, c = twice[0]
    assert ml.matrix(dup)[r, c] == 0 and ml.matrix(plain)[r, c] == 1 and (ml.matrix(dup) != ml.matrix(plain)).sum() == 1


@pytest.mark.parametrize("name", ("s40x60", "s40x60_hdup", "s129x150t5", "s800x100", "r240"))
def test_the_mirror_recovers_every_bit_peeling_does(files, name):
    """A bit that peeling recovers is a determined bit: solving the channel's output and solving what peeling leaves of it
    give the same frames; only the rank differs."""
    code = gf2_ref.Gf2Code(*files[name])
    n = 40
    eps = {"s40x60": 0.4, "s40x60_hdup": 0.4, "s129x150t5": 0.35, "s800x100": 0.03, "r240": 0.45}[name]
    cw = code.encode(np.random.default_rng(2).integers(0, 2, (n, code.kc), dtype=np.uint8)) if code.has_g else None
    w, e = er.channel(code, eps, 31, np.arange(n), cw)
    peeled = er.decode(code, w, e, 50, er.EARLY_TERM | er.STOP_STALLED)
    raw, after = ml.solve(code, w, e, code.nc), ml.solve(code, peeled["word"], peeled["erased"], code.nc)
    for key in ("word", "erased", "unresolved", "status"):
        assert np.array_equal(raw[key], after[key]), (name, key)
    moved = peeled["unresolved"] < e.sum(1)
    assert moved.any() and (after["rank"][moved] < raw["rank"][moved]).all()
    assert not (gf2_ref.unpack(raw["erased"], code.nc) & ~peeled["erased"]).any()  # nothing peeling filled is erased again
    assert (gf2_ref.unpack(raw["word"], code.nc)[peeled["erased"] == 0] == peeled["word"][peeled["erased"] == 0]).all()
    assert (raw["unresolved"] <= peeled["unresolved"]).all()
    if name == "r240":
        assert (raw["unresolved"] < peeled["unresolved"]).any()


def test_kernel_resources(lib):
    """kernels_erasure_solve.hip: one kernel, no scratch, no spills, no static LDS beside the frame's, and registers that let a
    workgroup of 1024 threads run (at most 128)."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_erasure_solve.hip")
    assert res and len(res) == 1 and "erasure_solve_kernel" in next(iter(res))
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] <= 128 and r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
    assert len(build.kernel_resources("kernels_erasure.hip")) == 2  # (the peeling kernels are as they were)
