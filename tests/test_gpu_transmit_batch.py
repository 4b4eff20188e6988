"""Frames of bits that stay on the device: ldpc_hip_encode_batch, ldpc_hip_syndrome_batch and ldpc_hip_bit_errors_batch
(include/ldpc_amd.h; libldpc_amd/csrc/kernels_gf2.hip) against the numpy mirror of tests/gf2_ref.py, which
test_transmit_batch_host.py pins against encode() and syndrome() of Part 1.  Pure GF(2): every comparison is np.array_equal.

The encoder keeps T words of a column's mask in registers, T = the largest power of two <= min(ceil(kc / 32), 32)
(kernels.hpp, gf2_encode_chunk_words), and walks a longer information word in windows of T, the last one moved back to end
at the row's end.  The largest T is 32 words = 1024 bits: of the three larger pairs s800x100 (kc = 800) lies below it and
runs T = 16 with a moved window, n7200 (kc = 3600) and s6000x3600 (kc = 6000) lie above it and walk 4 and 6 windows.  The
pairs of EXTRA fill in what generator_codes.py leaves out: T = 1, and a word of exactly T = 16 and T = 32 words."""
import numpy as np
import pytest

import generator_codes as gc
import gf2_ref
import orc

pytestmark = pytest.mark.gpu
FRAME_COUNTS = (1, 33, 70)  # no tile of the kernels (16 frames, 4 frames, 64 frames per workgroup) divides them
EXTRA = {"s20x30": dict(k=20, mc=30, col_weight=3), "s512x96": dict(k=512, mc=96, col_weight=3),
         "s1024x64": dict(k=1024, mc=64, col_weight=3)}
ENCODE_CODES = ("golden",) + gc.ENCODER_PAIRS + ("s800x100", "n7200", "s6000x3600") + tuple(EXTRA)
# name: (information words, T, windows): what each code asks of the kernel
ENCODE_SHAPES = {"golden": (4, 4, 1), "s40x60": (2, 2, 1), "s64x100": (2, 2, 1), "s129x150t5": (5, 4, 2), "s256x1792": (8, 8, 1),
                 "s200x1849": (7, 4, 2), "s257x200": (9, 8, 2), "s300x250t3": (10, 8, 2), "s40x60_dup": (2, 2, 1),
                 "s800x100": (25, 16, 2), "n7200": (113, 32, 4), "s6000x3600": (188, 32, 6), "s20x30": (1, 1, 1),
                 "s512x96": (16, 16, 1), "s1024x64": (32, 32, 1)}
SYNDROME_CODES = ("golden", "s200x1849", "n7200", "np_mix")  # np_mix: mc = 535, punctured and shortened columns, no generator


def chunk_words(words):
    t = 1
    while t < 32 and 2 * t <= words:
        t *= 2
    return t


class Codes:
    """The files, mirrors and decoders of the codes the tests use, each made once."""

    def __init__(self, directory):
        import non_parity_codes
        self.files = {"golden": (orc.H_TXT, orc.G_TXT), "np_mix": (non_parity_codes.write_code("np_mix", directory), "")}
        for name in list(gc.SYSTEMATIC) + list(gc.NULL_SPACE):
            self.files[name] = gc.write_pair(directory, name)
        for name, kw in EXTRA.items():
            self.files[name] = gc.write_systematic(directory, name, **kw)
        self.mirrors, self.decoders = {}, {}

    def mirror(self, name):
        if name not in self.mirrors:
            self.mirrors[name] = gf2_ref.Gf2Code(*self.files[name])
        return self.mirrors[name]

    def decoder(self, name):
        import libldpc_amd
        if name not in self.decoders:
            self.decoders[name] = libldpc_amd.HipDecoder(*self.files[name])
        return self.decoders[name]


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return Codes(tmp_path_factory.mktemp("transmit"))


def _garbage_high_bits(words, length, rng):
    """The packed rows with random bits put into each row's last word from `length` on: input the calls must ignore."""
    w = words.copy()
    if length % 32:
        w[:, -1] |= rng.integers(0, 2**32, w.shape[0], dtype=np.uint64).astype(np.uint32) << np.uint32(length % 32)
    return w


def test_shapes_cover_the_encoder():
    for name, (words, t, windows) in ENCODE_SHAPES.items():
        assert chunk_words(words) == t and -(-words // t) == windows, name
    kinds = {(t, words == t, words % t != 0) for words, t, _ in ENCODE_SHAPES.values()}
    assert {t for t, _, _ in kinds} == {1, 2, 4, 8, 16, 32}            # every instantiation
    assert {(16, True, False), (32, True, False), (16, False, True), (32, False, True)} <= kinds  # whole words and moved windows
    assert set(ENCODE_CODES) == set(ENCODE_SHAPES)


# ---- 1. the encoder against the mirror ----
@pytest.mark.parametrize("name", ENCODE_CODES)
def test_encode_batch_equals_the_mirror(codes, name):
    code, dec = codes.mirror(name), codes.decoder(name)
    assert (code.kc + 31) // 32 == ENCODE_SHAPES[name][0] and dec.kc == code.kc and dec.nc == code.nc
    rng = np.random.default_rng(11)
    words = (code.nc + 31) // 32
    cases = [("zero", np.zeros((1, code.kc), np.uint8)), ("one", np.ones((1, code.kc), np.uint8))]
    for n in FRAME_COUNTS:
        info = rng.integers(0, 2, (n, code.kc), dtype=np.uint8)
        if n > 2:
            info[n // 2], info[n - 1] = 0, 1
        cases.append((f"random{n}", info))
    for what, info in cases:
        want = code.encode(info)
        assert what == "zero" or want.any()
        assert not want[:, code.g_cols:].any()
        n = info.shape[0]
        inputs = {"bytes": info * rng.integers(1, 256, info.shape, dtype=np.uint8),  # (a non-zero byte is 1)
                  "packed": _garbage_high_bits(gf2_ref.pack(info), code.kc, rng)}
        for fmt, src in inputs.items():
            out = {"codeword": np.full((n, code.nc), 0xAB, np.uint8), "codeword_bits": np.full((n, words), 0xDEADBEEF, np.uint32)}
            got = dec.encode_batch(src, want=(), out=out)
            assert np.array_equal(got["codeword"], want), (name, what, fmt)
            assert np.array_equal(got["codeword_bits"], gf2_ref.pack(want)), (name, what, fmt)
            assert not gf2_ref.high_bits(got["codeword_bits"], code.nc).any(), (name, what, fmt)
    # each output by itself
    info = cases[-1][1]
    want = code.encode(info)
    assert np.array_equal(dec.encode_batch(info)["codeword"], want)
    assert np.array_equal(dec.encode_batch(gf2_ref.pack(info), want=("codeword_bits",))["codeword_bits"], gf2_ref.pack(want))


# ---- 2. the encoder against the stream's counter mode ----
@pytest.mark.parametrize("name", ("s129x150t5", "s257x200"))
def test_encode_batch_returns_the_counter_streams_codewords(codes, name):
    import libldpc_amd
    code = codes.mirror(name)
    dec = libldpc_amd.HipDecoder(*codes.files[name])
    n, seed, first = 70, 21, 5
    dec.set_noise("counter")
    dec.stream_begin("AWGN", seed, 1.0)
    dec.stream_skip(first)
    stream = dec.stream_decode(n, iterations=0, want=("codeword",))["codeword"]
    assert stream.any(1).mean() > 0.9
    # info bit j of frame f = bit j % 32 of word (j / 32) % 4 of block j / 128 of Philox tag 2: the words in order are the packed row
    kw = (code.kc + 31) // 32
    packed = np.stack([dec.philox(seed, 2, first + f, 0, (code.kc + 127) // 128).reshape(-1)[:kw] for f in range(n)])
    assert gf2_ref.high_bits(packed, code.kc).any()  # (the generator's bits from kc on are there, and ignored)
    assert np.array_equal(dec.encode_batch(packed)["codeword"], stream)
    assert np.array_equal(dec.encode_batch(gf2_ref.unpack(packed, code.kc))["codeword"], stream)
    assert np.array_equal(code.encode(gf2_ref.unpack(packed, code.kc)), stream)


# ---- 3. the syndrome against the mirror ----
@pytest.mark.parametrize("name", SYNDROME_CODES)
def test_syndrome_batch_equals_the_mirror(codes, name):
    code, dec = codes.mirror(name), codes.decoder(name)
    assert dec.mc == code.mc and (name != "np_mix" or (code.mc % 64 and code.mc % 32 and not code.has_g))
    rng = np.random.default_rng(12)
    sw = (code.mc + 31) // 32
    cases = [(f"random{n}", rng.integers(0, 2, (n, code.nc), dtype=np.uint8)) for n in FRAME_COUNTS]
    cols = np.unique(np.r_[0, 31, 32, 63, 64, code.nc - 1, rng.integers(0, code.nc, 27)])
    single = np.zeros((cols.size, code.nc), np.uint8)
    single[np.arange(cols.size), cols] = 1
    cases.append(("one bit", single))
    if code.has_g:
        cases.append(("codewords", code.encode(rng.integers(0, 2, (70, code.kc), dtype=np.uint8))))
    for what, word in cases:
        n = word.shape[0]
        want, weight = code.syndrome(word)
        if what == "one bit":
            assert np.array_equal(weight, [code.column_degree(c) for c in cols]) and weight.min() >= 1
        if what == "codewords":
            assert word.any() and not want.any() and not weight.any()
        inputs = {"bytes": word * rng.integers(1, 256, word.shape, dtype=np.uint8),
                  "packed": _garbage_high_bits(gf2_ref.pack(word), code.nc, rng)}
        for fmt, src in inputs.items():
            out = {"syndrome": np.full((n, code.mc), 0xAB, np.uint8), "syndrome_bits": np.full((n, sw), 0xDEADBEEF, np.uint32),
                   "weight": np.full(n, 0xDEADBEEF, np.uint32)}
            got = dec.syndrome_batch(src, want=(), out=out)
            assert np.array_equal(got["syndrome"], want), (name, what, fmt)
            assert np.array_equal(got["syndrome_bits"], gf2_ref.pack(want)), (name, what, fmt)
            assert not gf2_ref.high_bits(got["syndrome_bits"], code.mc).any(), (name, what, fmt)
            assert np.array_equal(got["weight"], weight), (name, what, fmt)
            # ... and one at a time
            assert np.array_equal(dec.syndrome_batch(src, want=("syndrome",))["syndrome"], want), (name, what, fmt)
            assert np.array_equal(dec.syndrome_batch(src, want=("syndrome_bits",))["syndrome_bits"], gf2_ref.pack(want)), (name, what, fmt)
            assert np.array_equal(dec.syndrome_batch(src)["weight"], weight), (name, what, fmt)


# ---- 4. / 5. chained on the device; bit errors ----
@pytest.fixture(scope="module")
def lds_frames(codes):
    """The 8 frames of DECODERS["lds"], case min_sum, as the stream delivers them (generator_codes.py: SEED, SKIP, FRAMES)."""
    import libldpc_amd
    name = gc.DECODERS["lds"][0]
    ch, decoding, early, iterations, _ = gc.CASES["min_sum"]
    dec = libldpc_amd.HipDecoder(*codes.files[name])
    dec.stream_begin(ch, gc.SEED, gc.POINTS["lds"]["min_sum"])
    dec.stream_skip(gc.SKIP)
    r = dec.stream_decode(gc.FRAMES, early_term=early, iterations=iterations, decoding=decoding,
                          want=("iters", "bit_errors", "hard", "llr_in", "codeword"))
    gc.check_mixed(r["iters"], r["bit_errors"], r["codeword"], early, iterations, "the stream's frames")
    return dict(r, dec=dec, name=name, early=early, iterations=iterations, decoding=decoding)


def test_chained_on_the_device(codes, lds_frames):
    import torch
    dev = torch.device("cuda", 0)
    f = lds_frames
    dec, code = f["dec"], codes.mirror(f["name"])
    n, words = 70, (code.nc + 31) // 32
    # encode -> syndrome, packed words passing from one call to the next
    rng = np.random.default_rng(13)
    info = torch.from_numpy(rng.integers(0, 2, (n, code.kc), dtype=np.uint8)).to(dev)
    bits = torch.full((n, words), -1, dtype=torch.int32, device=dev).view(torch.uint32)
    weight = torch.full((n,), -1, dtype=torch.int32, device=dev).view(torch.uint32)
    dec.encode_batch(info, want=(), out={"codeword_bits": bits})
    dec.syndrome_batch(bits, want=(), out={"weight": weight})
    torch.cuda.synchronize()
    assert np.array_equal(bits.cpu().numpy(), gf2_ref.pack(code.encode(info.cpu().numpy()))) and bits.cpu().numpy().any()
    assert not weight.cpu().numpy().any()
    # the stream's LLRs -> decode_batch_typed -> hard_bits -> syndrome
    m = gc.FRAMES
    llr = torch.from_numpy(f["llr_in"]).to(dev)
    hard_bits = torch.full((m, words), -1, dtype=torch.int32, device=dev).view(torch.uint32)
    iters = torch.zeros(m, dtype=torch.int32, device=dev)
    weight = torch.full((m,), -1, dtype=torch.int32, device=dev).view(torch.uint32)
    dec.decode_batch_typed(llr, early_term=f["early"], iterations=f["iterations"], decoding=f["decoding"], want=(),
                           out={"iters": iters, "hard_bits": hard_bits})
    dec.syndrome_batch(hard_bits, want=(), out={"weight": weight})
    errors = torch.full((m,), -1, dtype=torch.int32, device=dev).view(torch.uint32)
    dec.bit_errors_batch(hard_bits, torch.from_numpy(f["codeword"]).to(dev), out=errors)
    torch.cuda.synchronize()
    it, w = iters.cpu().numpy().astype(np.uint32), weight.cpu().numpy()
    assert np.array_equal(it, f["iters"]) and np.array_equal(hard_bits.cpu().numpy(), gf2_ref.pack(f["hard"]))
    stopped = it < f["iterations"]
    assert stopped.any() and not stopped.all()  # frames that stop early and frames that do not
    assert not w[stopped].any()
    assert np.array_equal(w, code.syndrome(f["hard"])[1])
    assert np.array_equal(errors.cpu().numpy(), f["bit_errors"])
    gc.check_mixed(it, errors.cpu().numpy(), f["codeword"], f["early"], f["iterations"], "chained")


def test_bit_errors_batch(codes, lds_frames):
    f = lds_frames
    dec, code = f["dec"], codes.mirror(f["name"])
    assert np.array_equal(code.bit_errors(f["hard"], f["codeword"]), f["bit_errors"]) and f["bit_errors"].any()
    rng = np.random.default_rng(14)
    forms = lambda rows: {"bytes": rows * rng.integers(1, 256, rows.shape, dtype=np.uint8),  # noqa: E731
                          "packed": _garbage_high_bits(gf2_ref.pack(rows), code.nc, rng)}
    for fa, a in forms(f["hard"]).items():
        for fb, b in forms(f["codeword"]).items():
            assert np.array_equal(dec.bit_errors_batch(a, b), f["bit_errors"]), (fa, fb)
    # h.txt has punctured columns: they do not count
    code, dec = codes.mirror("golden"), codes.decoder("golden")
    assert len(code.puncture) == 128 and code.nct == code.nc - 128
    for n in FRAME_COUNTS:
        a = rng.integers(0, 2, (n, code.nc), dtype=np.uint8)
        b = a.copy()
        base = dec.bit_errors_batch(a, gf2_ref.pack(b))
        assert not base.any()
        b[:, code.puncture] ^= 1
        assert not dec.bit_errors_batch(gf2_ref.pack(a), b).any()  # every punctured column flipped: nothing
        want = np.zeros(n, np.uint32)
        for i, c in enumerate((0, 255, 384, 1151)):  # transmitted columns around the punctured range and at both ends
            assert c in code.bit_pos
            b[i % n:, c] ^= 1
            want[i % n:] += 1
        for fa, aa in forms(a).items():
            for fb, bb in forms(b).items():
                assert np.array_equal(dec.bit_errors_batch(aa, bb), want) and np.array_equal(code.bit_errors(a, b), want), (n, fa, fb)
        c = rng.integers(0, 2, (n, code.nc), dtype=np.uint8)
        assert np.array_equal(dec.bit_errors_batch(a, c), code.bit_errors(a, c)) and dec.bit_errors_batch(a, c).min() > 100


# ---- 6. host and device buffers, another stream, and the stream interface left alone ----
def test_host_and_device_buffers_and_a_stream(codes):
    import torch
    dev = torch.device("cuda", 0)
    name = "s129x150t5"
    code, dec = codes.mirror(name), codes.decoder(name)
    rng = np.random.default_rng(15)
    n = 70
    info = rng.integers(0, 2, (n, code.kc), dtype=np.uint8)
    cw = code.encode(info)
    noisy = cw ^ (rng.random(cw.shape) < 0.02).astype(np.uint8)
    synd, weight = code.syndrome(noisy)
    errors = code.bit_errors(noisy, cw)
    assert weight.any() and errors.any()

    def u32(*shape):
        return torch.full(shape, -1, dtype=torch.int32, device=dev).view(torch.uint32)

    side = torch.cuda.Stream(device=dev)
    for stream in (None, side.cuda_stream):
        for on_device in (False, True):
            put = (lambda a: torch.from_numpy(a).to(dev)) if on_device else (lambda a: a)
            get = (lambda t: t.cpu().numpy()) if on_device else (lambda a: a)
            new8 = (lambda *s: torch.full(s, 0xAB, dtype=torch.uint8, device=dev)) if on_device else (lambda *s: np.full(s, 0xAB, np.uint8))
            new32 = u32 if on_device else (lambda *s: np.full(s, 0xDEADBEEF, np.uint32))
            ins = [put(gf2_ref.pack(info)), put(noisy), put(gf2_ref.pack(noisy))]
            e = {"codeword": new8(n, code.nc), "codeword_bits": new32(n, (code.nc + 31) // 32)}
            s = {"syndrome": new8(n, code.mc), "syndrome_bits": new32(n, (code.mc + 31) // 32), "weight": new32(n)}
            b = new32(n)
            torch.cuda.synchronize()  # (the buffers were filled on torch's stream; the calls run on `stream`)
            dec.encode_batch(ins[0], want=(), stream=stream, out=e)
            dec.syndrome_batch(ins[1], want=(), stream=stream, out=s)
            dec.bit_errors_batch(ins[2], e["codeword"], out=b, stream=stream)
            dec.synchronize(stream)
            what = (stream is not None, on_device)
            assert np.array_equal(get(e["codeword"]), cw) and np.array_equal(get(e["codeword_bits"]), gf2_ref.pack(cw)), what
            assert np.array_equal(get(s["syndrome"]), synd) and np.array_equal(get(s["syndrome_bits"]), gf2_ref.pack(synd)), what
            assert np.array_equal(get(s["weight"]), weight) and np.array_equal(get(b), errors), what


def test_the_stream_interface_is_left_alone(codes):
    """A stream_decode sequence on the reference noise stream, a generator loaded (the encoder's running codeword and its
    information-word stream are state), with and without the three calls between its batches."""
    import libldpc_amd
    code = codes.mirror("golden")
    rng = np.random.default_rng(16)
    info = rng.integers(0, 2, (33, code.kc), dtype=np.uint8)
    runs = []
    for between in (False, True):
        dec = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
        dec.stream_begin("AWGN", 9, 2.0)
        got = []
        for batch in (5, 33, 1, 70):
            if between:
                cw = dec.encode_batch(info, want=("codeword", "codeword_bits"))
                assert np.array_equal(cw["codeword"], code.encode(info))
                assert not dec.syndrome_batch(cw["codeword_bits"])["weight"].any()
                assert not dec.bit_errors_batch(cw["codeword"], cw["codeword_bits"]).any()
            got.append(dec.stream_decode(batch, iterations=10, decoding="BP_MS", want=("iters", "bit_errors", "codeword")))
        runs.append(got)
    for plain, mixed in zip(*runs):
        for k in ("iters", "bit_errors", "codeword"):
            assert np.array_equal(plain[k], mixed[k]), k
    assert all(r["codeword"].any() for r in runs[0])
