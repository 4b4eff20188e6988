"""ldpc_hip_erasure_channel_batch and ldpc_hip_erasure_decode_batch (include/ldpc_amd.h) without a GPU: the exported symbols
and their prototypes, everything the calls refuse before they touch a device, the binding's own checks, the LDS formula of
ldpc_hip_erasure_lds_bytes, the numpy mirror (tests/erasure_ref.py) against an independent message-passing decoder pass by
pass, the stalled-stop property of the mirror, and the compile-time resources of kernels_erasure.hip."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

import erasure_ref as er
import generator_codes as gc
import gf2_ref
import orc

U8, PACKED32 = 0, 1
CHANNEL, DECODE = b"ldpc_hip_erasure_channel_batch", b"ldpc_hip_erasure_decode_batch"


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


def _regular(directory, nc, seed=1):
    sys.path.insert(0, os.path.join(orc.ROOT, "tools"))
    import gen_regular_code
    path = os.path.join(str(directory), f"r{nc}.h.txt")
    if not os.path.exists(path):
        open(path, "w").write(gen_regular_code.generate(nc, 3, 6, seed))
    return path, ""


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("erasure")
    out = {"golden": (orc.H_TXT, orc.G_TXT), "r240": _regular(d, 240), "r14000": _regular(d, 14000)}
    for name in ("s40x60", "s129x150t5", "s40x60_dup", "s800x100"):
        out[name] = gc.write_pair(d, name)
    out["s40x60_hdup"] = (er.repeat_entries(out["s40x60"][0], os.path.join(str(d), "s40x60_hdup.h.txt")), "")  # parallel edges in H
    return out


def test_symbols_and_signatures(lib):
    vp, u64, u32, i32, f64 = ct.c_void_p, ct.c_uint64, ct.c_uint32, ct.c_int, ct.c_double
    assert lib.ldpc_hip_erasure_channel_batch.argtypes == [vp, f64, u64, u64, u64, vp, i32, vp, vp, vp]
    assert lib.ldpc_hip_erasure_channel_batch.restype == i32
    assert lib.ldpc_hip_erasure_decode_batch.argtypes == [vp, u32, i32, u64, vp, vp, i32, vp, vp, vp, vp, vp]
    assert lib.ldpc_hip_erasure_decode_batch.restype == i32
    assert lib.ldpc_hip_erasure_lds_bytes.argtypes == [vp] and lib.ldpc_hip_erasure_lds_bytes.restype == ct.c_int64
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_erasure_channel_batch(ldpc_hip_ctx *ctx, double eps, uint64_t seed, uint64_t first_frame, uint64_t n, "
            "const void *codeword, int codeword_format, uint32_t *word_bits, uint32_t *erased_bits, void *hip_stream);") in flat
    assert ("int ldpc_hip_erasure_decode_batch(ldpc_hip_ctx *ctx, uint32_t iterations, int flags, uint64_t n, const void *word, "
            "const void *erased, int format, uint32_t *word_out, uint32_t *erased_out, uint32_t *iters, uint32_t *unresolved, "
            "void *hip_stream);") in flat
    assert "int64_t ldpc_hip_erasure_lds_bytes(const ldpc_hip_ctx *ctx);" in flat
    assert "LDPC_HIP_ERASURE_EARLY_TERM = 1, LDPC_HIP_ERASURE_STOP_STALLED = 2" in flat
    assert "ldpc_hip_encode_batch -> ldpc_hip_erasure_channel_batch -> ldpc_hip_erasure_decode_batch -> ldpc_hip_syndrome_batch" in flat
    import libldpc_amd
    assert (libldpc_amd.HipDecoder.ERASURE_EARLY_TERM, libldpc_amd.HipDecoder.ERASURE_STOP_STALLED) == (er.EARLY_TERM, er.STOP_STALLED)


def test_refusals_come_before_the_gpu(lib, files):
    """No GPU here: a call that reached the device would fail with another message, or not at all."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(*files["s129x150t5"])
    words = (d.nc + 31) // 32
    cw = np.zeros((2, d.nc), np.uint8)
    a, b = np.zeros((2, words), np.uint32), np.zeros((2, words), np.uint32)
    cnt = np.zeros(2, np.uint32)
    err = lib.ldpc_hip_last_error
    nan = float("nan")

    def channel(n, eps=0.1, fmt=U8, src=cw.ctypes.data, word=a.ctypes.data, erased=b.ctypes.data):
        return lib.ldpc_hip_erasure_channel_batch(d.ctx, eps, 5, 0, n, src, fmt, word, erased, None)

    def decode(n, flags=1, fmt=PACKED32, word=a.ctypes.data, erased=b.ctypes.data, ctx=None):
        return lib.ldpc_hip_erasure_decode_batch(ctx or d.ctx, 50, flags, n, word, erased, fmt, a.ctypes.data, b.ctypes.data,
                                                 cnt.ctypes.data, cnt.ctypes.data, None)

    for n in (0, 2):
        for what, kw in {"format 2": dict(fmt=2), "format -1": dict(fmt=-1), "eps 0": dict(eps=0.0), "eps 1": dict(eps=1.0),
                         "eps nan": dict(eps=nan), "eps -0.1": dict(eps=-0.1), "eps 1.5": dict(eps=1.5)}.items():
            assert channel(n, **kw) == -1 and CHANNEL in err(), (n, what, err())
        for what, kw in {"format 2": dict(fmt=2), "format -1": dict(fmt=-1), "flags 4": dict(flags=4), "flags 7": dict(flags=7),
                         "flags -1": dict(flags=-1), "flags 8": dict(flags=8)}.items():
            assert decode(n, **kw) == -1 and DECODE in err(), (n, what, err())
    assert channel(2, word=None, erased=None) == -1 and CHANNEL in err()  # both outputs NULL: with frames to work on only
    assert channel(0, word=None, erased=None) == 0
    assert decode(2, word=None) == -1 and DECODE in err() and decode(2, erased=None) == -1 and DECODE in err()
    # after the checks n == 0 returns 0 (no GPU needed): every format and flag combination, with and without buffers
    for fmt in (U8, PACKED32):
        assert channel(0, fmt=fmt) == 0 and channel(0, fmt=fmt, src=None) == 0 and channel(0, eps=0.999, fmt=fmt, word=None) == 0
        for flags in (0, 1, 2, 3):
            assert decode(0, flags, fmt) == 0 and decode(0, flags, fmt, None, None) == 0
    # a code whose group does not fit is refused by the decoder alone, before the GPU, frames or none
    big = libldpc_amd.HipDecoder(*files["r14000"])
    assert big.erasure_lds_bytes() == -1
    for n in (0, 2):
        assert decode(n, ctx=big.ctx) == -1 and DECODE in err() and b"LDS" in err()
    with pytest.raises(RuntimeError, match="ldpc_hip_erasure_decode_batch"):
        big.erasure_decode_batch(np.zeros((0, (14000 + 31) // 32), np.uint32), np.zeros((0, (14000 + 31) // 32), np.uint32))
    assert big.erasure_channel_batch(None, 0.3, frames=0)["erased"].shape == (0, (14000 + 31) // 32)
    # the binding, n == 0
    r = d.erasure_channel_batch(np.zeros((0, d.nc), np.uint8), 0.3)
    assert set(r) == {"word", "erased"} and all(v.shape == (0, words) and v.dtype == np.uint32 for v in r.values())
    r = d.erasure_decode_batch(np.zeros((0, d.nc), np.uint8), np.zeros((0, d.nc), np.uint8), stop_stalled=True)
    assert set(r) == {"word", "erased", "iters", "unresolved"} and r["iters"].shape == (0,) and r["word"].shape == (0, words)


def test_binding_refuses_other_dtypes_and_shapes(lib, files):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(*files["s40x60"])
    words = (d.nc + 31) // 32
    u8, pk = np.zeros((1, d.nc), np.uint8), np.zeros((1, words), np.uint32)
    for dt in (np.int8, np.int32, np.uint16, np.float32, np.bool_):
        with pytest.raises(TypeError, match="erasure_channel_batch"):
            d.erasure_channel_batch(np.zeros((1, d.nc), dt), 0.3)
        with pytest.raises(TypeError, match="erasure_decode_batch"):
            d.erasure_decode_batch(np.zeros((1, d.nc), dt), u8)
    with pytest.raises(ValueError, match="erasure_channel_batch"):
        d.erasure_channel_batch(np.zeros((1, d.nc + 1), np.uint8), 0.3)
    with pytest.raises(ValueError, match="frames"):
        d.erasure_channel_batch(None, 0.3)
    with pytest.raises(ValueError, match="frames"):
        d.erasure_channel_batch(np.zeros((0, d.nc), np.uint8), 0.3, frames=3)
    with pytest.raises(ValueError, match="erasure_decode_batch"):
        d.erasure_decode_batch(u8, pk)  # both operands in one format
    with pytest.raises(ValueError, match="erasure_decode_batch"):
        d.erasure_decode_batch(pk, np.zeros((2, words), np.uint32))
    with pytest.raises(ValueError, match="erasure_decode_batch"):
        d.erasure_decode_batch(np.zeros((1, d.nc), np.uint32), np.zeros((1, d.nc), np.uint32))  # packed rows are ceil(nc / 32) words
    with pytest.raises(KeyError):
        d.erasure_decode_batch(pk[:0], pk[:0], want=("hard",))
    with pytest.raises(TypeError, match="iters"):
        d.erasure_decode_batch(pk[:0], pk[:0], want=(), out={"iters": np.zeros(0, np.int64)})
    with pytest.raises(ValueError, match="erased"):
        d.erasure_channel_batch(u8, 0.3, want=(), out={"erased": np.zeros((2, words), np.uint32)})


def _formula(code):
    degree = np.bincount(code.h_cols, minlength=code.nc)
    n8 = int((degree >= 8).sum())
    chunks = -(-code.mc // 64) + -(-n8 // 16) + -(-(code.nc - n8) // 64)
    return -(-(4 * (2 * (code.nc + 1) + 2 * (code.mc + 1)) + 8 * chunks + 144) // 16) * 16


def test_lds_bytes_formula(lib, files):
    """The formula of the header on h.txt (128 columns of degree 15: wide chunks), s40x60 (none) and a code that is refused."""
    import libldpc_amd
    golden = gf2_ref.Gf2Code(*files["golden"])
    assert (golden.nc, golden.mc) == (1152, 1024) and int((np.bincount(golden.h_cols) >= 8).sum()) == 128
    assert _formula(golden) == 17888 and libldpc_amd.HipDecoder(*files["golden"]).erasure_lds_bytes() == 17888
    assert 4 * 17888 <= 160 * 1024  # four groups of 512 threads: the 32 waves of a CU
    small = gf2_ref.Gf2Code(*files["s40x60"])
    assert _formula(small) == 1472  # 4 (202 + 122) + 8 * 3 + 144 = 1464, rounded up
    assert libldpc_amd.HipDecoder(*files["s40x60"]).erasure_lds_bytes() == _formula(small)
    wide = gf2_ref.Gf2Code(*files["s800x100"])
    assert libldpc_amd.HipDecoder(*files["s800x100"]).erasure_lds_bytes() == _formula(wide)
    big = gf2_ref.Gf2Code(*files["r14000"])
    assert _formula(big) > 160 * 1024 and libldpc_amd.HipDecoder(*files["r14000"]).erasure_lds_bytes() == -1


# (code, erasure probabilities): below, near and beyond where peeling stops resolving whole frames
POINTS = {"golden": (0.3, 0.82, 0.85), "s40x60": (0.1, 0.2, 0.4), "s129x150t5": (0.1, 0.2, 0.35), "s40x60_dup": (0.2, 0.4),
          "s800x100": (0.01, 0.03), "r240": (0.3, 0.42, 0.5), "s40x60_hdup": (0.1, 0.2, 0.4)}
# ... and one at which some of 32 frames resolve and some stall
STALL_POINTS = {"golden": 0.84, "s40x60": 0.3, "s129x150t5": 0.25, "s40x60_dup": 0.3, "s800x100": 0.02, "r240": 0.42,
                "s40x60_hdup": 0.3}


def _codeword(code, n, seed):
    if not code.has_g:
        return np.zeros((n, code.nc), np.uint8)
    return code.encode(np.random.default_rng(seed).integers(0, 2, (n, code.kc), dtype=np.uint8))


@pytest.mark.parametrize("name", sorted(POINTS))
def test_mirror_equals_message_passing_pass_by_pass(files, name):
    """The claim the kernel rests on: the node-value iteration of the contract resolves exactly the columns of the
    message-passing decoder, to the same values, after every pass — on codewords with erasures (consistent input)."""
    code = gf2_ref.Gf2Code(*files[name])
    passes, n = 30, 12
    for k, eps in enumerate(POINTS[name]):
        word, erased = er.channel(code, eps, 40 + k, np.arange(n), _codeword(code, n, k))
        trace = []
        er.decode(code, word, erased, passes, 0, trace)
        mp = er.message_passing(code, word, erased, passes)
        assert len(trace) == len(mp) == passes
        for i, ((e, v), (me, mv)) in enumerate(zip(trace, mp)):
            assert np.array_equal(e, me) and np.array_equal(v, mv), (name, eps, i)


def test_mirror_channel_rules(files):
    code = gf2_ref.Gf2Code(*files["s129x150t5"])
    cw = _codeword(code, 6, 3)
    word, erased = er.channel(code, 0.5, 9, np.arange(6), cw)
    assert len(code.shorten) == 5 and not erased[:, code.shorten].any()  # shortened: known, the codeword's own bit
    assert np.array_equal(word[:, code.shorten], cw[:, code.shorten] != 0)
    assert np.array_equal(word, (cw != 0) & ~erased)
    golden = gf2_ref.Gf2Code(*files["golden"])
    word, erased = er.channel(golden, 0.5, 9, np.arange(40))
    assert erased[:, golden.puncture].all() and not word.any()
    rate = erased[:, golden.bit_pos].mean()
    assert abs(rate - 0.5) < 5 * np.sqrt(0.25 / (40 * golden.nct))


@pytest.mark.parametrize("name", sorted(POINTS))
def test_stalled_stop_changes_nothing_but_iters(files, name):
    """A pass that removed nothing from E is followed by passes that remove nothing: stopping there leaves word, erased and
    unresolved as they are.  iters follows item 4 of the contract."""
    code = gf2_ref.Gf2Code(*files[name])
    n, iterations = 32, 50
    rng = np.random.default_rng(5)
    word, erased = er.channel(code, STALL_POINTS[name], 8, np.arange(n), _codeword(code, n, 1))
    word[n // 2:] = rng.integers(0, 2, (n - n // 2, code.nc)) != 0  # (not codewords)
    for early in (0, er.EARLY_TERM):
        base = er.decode(code, word, erased, iterations, early)
        stop = er.decode(code, word, erased, iterations, early | er.STOP_STALLED)
        for key in ("word", "erased", "unresolved"):
            assert np.array_equal(base[key], stop[key]), (name, early, key)
        trace = []
        er.decode(code, word, erased, iterations, 0, trace)
        left = np.stack([e.sum(1) for e, _ in trace], 1)                          # [n][iterations]: |E| after every pass
        before = np.concatenate([erased.sum(1)[:, None], left[:, :-1]], 1)
        # the first pass that removed nothing (a frame still moving at the limit runs every pass)
        stall = np.where((left == before).any(1), np.argmax(left == before, 1), iterations - 1)
        assert ((left == before).any(1) & (left[:, -1] > 0)).any(), name  # (some frame does stall with erasures left)
        resolved = (left == 0).any(1)
        assert 0 < resolved.sum() < n, name
        # early: a resolved frame stopped at its resolving pass I with iters = I; a stalled one after pass `stall`: stall + 1
        first_empty = np.argmax(left == 0, 1)
        want = np.where(resolved, first_empty, stall + 1) if early else stall + 1
        assert np.array_equal(stop["iters"], want.astype(np.uint32)), (name, early)
        assert np.array_equal(base["iters"], np.where(resolved, first_empty, iterations) if early else np.full(n, iterations))


def test_kernel_resources(lib):
    """kernels_erasure.hip: no scratch, no spills, at most 64 VGPRs (eight waves per SIMD), no static LDS beside the group's."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_erasure.hip")
    assert res and len(res) == 2
    assert sorted(k.split("erasure_")[1].split("_kernel")[0] for k in res) == ["channel", "decode"]
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8 and r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
    assert len(build.kernel_resources("kernels_channel.hip")) == 20  # (the channel_kernel instantiations are as they were)
