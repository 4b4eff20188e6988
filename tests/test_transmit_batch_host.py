"""The batch calls on frames of bits (include/ldpc_amd.h: ldpc_hip_encode_batch, ldpc_hip_syndrome_batch,
ldpc_hip_bit_errors_batch) without a GPU: the numpy mirror of tests/gf2_ref.py pinned against encode() and syndrome() of Part 1
(host code both, independent of the new kernels), every generator pair's rows in the null space of its H, the exported
symbols, what the calls refuse before they touch a device, and the kernels' compile-time resources."""
import ctypes as ct
import os

import numpy as np
import pytest

import generator_codes as gc
import gf2_ref
import orc

U8, PACKED32 = 0, 1
ENTRIES = (b"ldpc_hip_encode_batch", b"ldpc_hip_syndrome_batch", b"ldpc_hip_bit_errors_batch")
PART1_PAIRS = ("golden", "s129x150t5", "s40x60_dup")  # g.txt; a tail (G.cols < nc, G.rows < kc); a repeated entry


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module")
def pair_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs")
    out = {"golden": (orc.H_TXT, orc.G_TXT)}
    for name in list(gc.SYSTEMATIC) + list(gc.NULL_SPACE):
        out[name] = gc.write_pair(d, name)
    return out


def _setup(lib, h, g):
    n, m, nct, mct = (ct.c_int(0) for _ in range(4))
    lib.ldpc_setup(h.encode(), g.encode(), ct.byref(n), ct.byref(m), ct.byref(nct), ct.byref(mct))
    return n.value, m.value, nct.value, mct.value


@pytest.mark.parametrize("name", PART1_PAIRS)
def test_mirror_encoder_against_part1(lib, pair_files, name):
    """For information whose bits from kct on are 0, encode() returns the mirror's codeword[bit_pos[i]] at position i."""
    h, g = pair_files[name]
    code = gf2_ref.Gf2Code(h, g)
    assert _setup(lib, h, g) == (code.nc, code.mc, code.nct, code.mc - len(code.puncture))
    rng = np.random.default_rng(3)
    info = np.zeros((40, code.kc), np.uint8)
    info[:, :code.kct] = rng.integers(0, 2, (40, code.kct))
    info[0] = 0
    info[1, :code.kct] = 1
    info[2, :code.kct] = rng.integers(0, 256, code.kct) | 2  # any non-zero byte is a 1 ...
    want = code.encode(info)
    assert np.array_equal(want[2], code.encode((info[2:3] != 0))[0]) and want.any(1).sum() >= 38
    assert not want[:, code.g_cols:].any()
    lib.encode.argtypes, lib.encode.restype = [ct.c_void_p, ct.c_void_p], None
    for f in range(info.shape[0]):
        u = np.ascontiguousarray(info[f, :code.kct])
        cw = np.full(code.nct, 7, np.uint8)
        lib.encode(u.ctypes.data, cw.ctypes.data)
        assert np.array_equal(cw, want[f, code.bit_pos]), (name, f)


@pytest.mark.parametrize("name", PART1_PAIRS + ("n7200",))
def test_mirror_syndrome_against_part1(lib, pair_files, name):
    h, g = pair_files[name]
    code = gf2_ref.Gf2Code(h, g)
    _setup(lib, h, g)
    rng = np.random.default_rng(4)
    words = rng.integers(0, 2, (12, code.nc), dtype=np.uint8)
    words[0] = 0
    words[1] = 1
    want, weight = code.syndrome(words)
    assert np.array_equal(weight, want.sum(1)) and weight[2:].min() > 0
    lib.syndrome.argtypes, lib.syndrome.restype = [ct.c_void_p, ct.c_void_p], None
    for f in range(words.shape[0]):
        s = np.full(code.mc, 7, np.uint8)
        lib.syndrome(words[f].ctypes.data, s.ctypes.data)
        assert np.array_equal(s, want[f]), (name, f)


def test_every_row_of_every_generator_is_a_codeword(pair_files):
    for name, (h, g) in pair_files.items():
        code = gf2_ref.Gf2Code(h, g)
        assert code.g_rows <= code.kc, name
        for first in range(0, code.kc, 1024):
            rows = np.arange(first, min(first + 1024, code.kc))
            info = np.zeros((rows.size, code.kc), np.uint8)
            info[np.arange(rows.size), rows] = 1
            cw = code.encode(info)
            s, weight = code.syndrome(cw)
            assert not s.any() and not weight.any(), (name, first)
            assert first > 0 or cw.any(1).sum() >= 1, name


def test_packed_layout_of_the_mirror():
    rng = np.random.default_rng(5)
    for length in (1, 31, 32, 33, 64, 100, 2049):
        bits = rng.integers(0, 2, (3, length), dtype=np.uint8)
        w = gf2_ref.pack(bits * 5)
        assert w.shape == (3, (length + 31) // 32) and w.dtype == np.uint32
        for i in (0, length // 2, length - 1):
            assert np.array_equal((w[:, i >> 5] >> np.uint32(i & 31)) & 1, bits[:, i])
        assert not gf2_ref.high_bits(w, length).any() and np.array_equal(gf2_ref.unpack(w, length), bits)


def test_symbols_and_signatures(lib):
    vp, u64, i32 = ct.c_void_p, ct.c_uint64, ct.c_int
    assert lib.ldpc_hip_encode_batch.argtypes == [vp, u64, vp, i32, vp, vp, vp]
    assert lib.ldpc_hip_syndrome_batch.argtypes == [vp, u64, vp, i32, vp, vp, vp, vp]
    assert lib.ldpc_hip_bit_errors_batch.argtypes == [vp, u64, vp, i32, vp, i32, vp, vp]
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_encode_batch(ldpc_hip_ctx *ctx, uint64_t n, const void *info, int info_format, uint8_t *codeword, "
            "uint32_t *codeword_bits, void *hip_stream);") in flat
    assert ("int ldpc_hip_syndrome_batch(ldpc_hip_ctx *ctx, uint64_t n, const void *word, int word_format, uint8_t *syndrome, "
            "uint32_t *syndrome_bits, uint32_t *weight, void *hip_stream);") in flat
    assert ("int ldpc_hip_bit_errors_batch(ldpc_hip_ctx *ctx, uint64_t n, const void *a, int a_format, const void *b, "
            "int b_format, uint32_t *bit_errors, void *hip_stream);") in flat
    assert "LDPC_HIP_BITS_U8 = 0" in flat and "LDPC_HIP_BITS_PACKED32 = 1" in flat


def test_refusals_come_before_the_gpu(lib, pair_files):
    """No GPU here: a call that reached the device would fail with another message, or not at all."""
    import libldpc_amd
    h, g = pair_files["s129x150t5"]
    with_g, without_g = libldpc_amd.HipDecoder(h, g), libldpc_amd.HipDecoder(h)
    info = np.zeros((2, with_g.kc), np.uint8)
    word = np.zeros((2, with_g.nc), np.uint8)
    cw = np.zeros((2, with_g.nc), np.uint8)
    weight = np.zeros(2, np.uint32)
    err = lib.ldpc_hip_last_error

    def encode(d, n, fmt, src=info.ctypes.data):
        return lib.ldpc_hip_encode_batch(d.ctx, n, src, fmt, cw.ctypes.data, None, None)

    def syndrome(d, n, fmt, src=word.ctypes.data):
        return lib.ldpc_hip_syndrome_batch(d.ctx, n, src, fmt, None, None, weight.ctypes.data, None)

    def bit_errors(d, n, fa, fb, a=word.ctypes.data, b=cw.ctypes.data):
        return lib.ldpc_hip_bit_errors_batch(d.ctx, n, a, fa, b, fb, weight.ctypes.data, None)

    for n in (0, 2):
        # a context created without a generator
        for fmt in (U8, PACKED32):
            assert encode(without_g, n, fmt) == -1 and ENTRIES[0] in err() and b"generator" in err(), (n, fmt)
        # an unknown format value, on each entry and each operand
        for fmt in (2, -1, 1000):
            assert encode(with_g, n, fmt) == -1 and ENTRIES[0] in err() and b"format" in err(), (n, fmt)
            assert syndrome(with_g, n, fmt) == -1 and ENTRIES[1] in err() and b"format" in err(), (n, fmt)
            assert bit_errors(with_g, n, fmt, U8) == -1 and ENTRIES[2] in err() and b"format" in err(), (n, fmt)
            assert bit_errors(with_g, n, PACKED32, fmt) == -1 and ENTRIES[2] in err() and b"format" in err(), (n, fmt)
    # a missing input with frames to work on is an error, not a crash
    assert encode(with_g, 2, U8, None) == -1 and ENTRIES[0] in err()
    assert syndrome(with_g, 2, PACKED32, None) == -1 and ENTRIES[1] in err()
    assert bit_errors(with_g, 2, U8, U8, None) == -1 and ENTRIES[2] in err()
    assert bit_errors(with_g, 2, U8, U8, word.ctypes.data, None) == -1 and ENTRIES[2] in err()
    # after the checks n == 0 returns 0 (no GPU needed): every format, with and without buffers
    for fmt in (U8, PACKED32):
        assert encode(with_g, 0, fmt) == 0 and encode(with_g, 0, fmt, None) == 0
        assert syndrome(with_g, 0, fmt) == 0 and syndrome(without_g, 0, fmt, None) == 0
        for fb in (U8, PACKED32):
            assert bit_errors(without_g, 0, fmt, fb) == 0 and bit_errors(with_g, 0, fmt, fb, None, None) == 0
    assert with_g.encode_batch(np.zeros((0, with_g.kc), np.uint8), want=("codeword", "codeword_bits"))["codeword_bits"].shape == (0, 9)
    assert with_g.syndrome_batch(np.zeros((0, 9), np.uint32))["weight"].shape == (0,)
    assert with_g.bit_errors_batch(np.zeros((0, 9), np.uint32), np.zeros((0, with_g.nc), np.uint8)).shape == (0,)


def test_generator_with_more_rows_than_kc_is_refused(lib, tmp_path):
    """G.rows > kc: the rule of the stream encoder (Engine::encoder_prologue)."""
    import libldpc_amd
    from minsum_common import write
    h = write(tmp_path / "h.txt", [[0, 1, 2], [2, 3, 4], [4, 5, 0], [1, 3, 5]])  # 4 x 6: kc = 2
    g = tmp_path / "g.txt"
    g.write_text("0 0\n1 1\n2 2")
    d = libldpc_amd.HipDecoder(h, str(g))
    assert d.kc == 2
    info = np.zeros((1, 2), np.uint8)
    for n in (0, 1):
        assert lib.ldpc_hip_encode_batch(d.ctx, n, info.ctypes.data, U8, None, None, None) == -1
        assert ENTRIES[0] in lib.ldpc_hip_last_error() and b"rows" in lib.ldpc_hip_last_error()


def test_binding_refuses_other_dtypes_and_shapes(lib, pair_files):
    import libldpc_amd
    h, g = pair_files["s40x60"]
    d = libldpc_amd.HipDecoder(h, g)
    for dt in (np.int8, np.int32, np.uint16, np.uint64, np.float32, np.bool_):
        with pytest.raises(TypeError, match="encode_batch"):
            d.encode_batch(np.zeros((1, d.kc), dt))
        with pytest.raises(TypeError, match="syndrome_batch"):
            d.syndrome_batch(np.zeros((1, d.nc), dt))
        with pytest.raises(TypeError, match="bit_errors_batch"):
            d.bit_errors_batch(np.zeros((1, d.nc), np.uint8), np.zeros((1, d.nc), dt))
    with pytest.raises(ValueError, match="encode_batch"):
        d.encode_batch(np.zeros((1, d.kc + 1), np.uint8))
    with pytest.raises(ValueError, match="syndrome_batch"):
        d.syndrome_batch(np.zeros((1, d.nc), np.uint32))  # packed rows are ceil(nc / 32) words
    with pytest.raises(ValueError, match="bit_errors_batch"):
        d.bit_errors_batch(np.zeros((2, d.nc), np.uint8), np.zeros((1, d.nc), np.uint8))
    with pytest.raises(KeyError):
        d.encode_batch(np.zeros((0, d.kc), np.uint8), want=("hard",))


def test_chunk_words_and_kernel_resources(lib):
    """No kernel of kernels_gf2.hip uses scratch; the encoder's instantiations are the six chunk sizes."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_gf2.hip")
    assert res
    enc = [k for k in res if "gf2_encode_kernel" in k]
    assert len(enc) == 6 and len([k for k in res if "gf2_syndrome_kernel" in k]) == 4
    assert len([k for k in res if "gf2_bit_errors_kernel" in k]) == 4 and len(res) == 14
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r["VGPRs"] <= 64, (name, r)
