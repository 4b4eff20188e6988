"""ldpc_hip_channel_batch (include/ldpc_amd.h; libldpc_amd/csrc/kernels_channel.hip) on the GPU: against the stream's counter
noise mode (binary signalling: bit for bit), against the numpy mirror of tests/channel_ref.py (the BSC exactly; the AWGN's
received values within the bound the counter mode's normals are held to; the demapper, the conversions and the quantizer
exactly, applied to the device's own received values), over the input formats, splits and buffer kinds, chained between the
encoder and the typed decoder on device tensors, and between the batches of a running stream.

The codes: tests/golden/h.txt (128 punctured columns, nct = 1024), s129x150t5 (5 shortened columns, nct = 279), s257x200
(nct = 457) and s40x60 (nct = 100): nct % 4 = 0, 3, 1, 0; padding symbols at m = 2 (279, 457), m = 3 (1024, 457, 100) and
m = 4 (279, 457); a last Philox block with 1, 2, 3 and 4 symbols."""
import numpy as np
import pytest

import channel_ref as cr
import generator_codes as gc
import gf2_ref
import orc
import philox_ref

pytestmark = pytest.mark.gpu
NAMES = ("golden", "s129x150t5", "s257x200", "s40x60")
N = 70  # frames of most calls: with a code's lanes per frame no multiple of the 256 lanes of a workgroup


class Codes:
    def __init__(self, directory):
        self.files = {"golden": (orc.H_TXT, orc.G_TXT)}
        for name in NAMES[1:]:
            self.files[name] = gc.write_pair(directory, name)
        self.mirrors, self.decoders = {}, {}

    def mirror(self, name):
        if name not in self.mirrors:
            self.mirrors[name] = gf2_ref.Gf2Code(*self.files[name])
        return self.mirrors[name]

    def decoder(self, name, generator=True):
        import libldpc_amd
        if (name, generator) not in self.decoders:
            h, g = self.files[name]
            self.decoders[(name, generator)] = libldpc_amd.HipDecoder(h, g if generator else "")
        return self.decoders[(name, generator)]


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return Codes(tmp_path_factory.mktemp("channel"))


def _random_words(code, n, seed):
    """Random codewords of the pair's generator, then a frame of zeros and a frame of ones."""
    rng = np.random.default_rng(seed)
    cw = code.encode(rng.integers(0, 2, (n, code.kc), dtype=np.uint8))
    cw[n // 2], cw[n - 1] = 0, 1
    return cw


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(cr.raw(a), cr.raw(b))


def test_the_codes_cover_the_paths(codes):
    ncts = [codes.mirror(name).nct for name in NAMES]
    assert ncts == [1024, 279, 457, 100] and [t % 4 for t in ncts] == [0, 3, 1, 0]
    assert len(codes.mirror("golden").puncture) == 128 and len(codes.mirror("s129x150t5").shorten) == 5
    for m in (2, 3, 4):
        assert any(t % m for t in ncts)
    assert {cr.symbols(m, t) % 4 for m in (1, 2, 3, 4) for t in ncts} == {0, 1, 2, 3}


# ---- 1. binary signalling is the stream's counter noise mode ----
@pytest.mark.parametrize("channel, x", [("AWGN", 3.0), ("AWGN", -4.0), ("BSC", 0.02), ("BSC", 0.24)])
@pytest.mark.parametrize("name", NAMES)
def test_stream_identity(codes, name, channel, x):
    seed, skip = 31, 9
    for generator in (True, False):
        dec = codes.decoder(name, generator)
        dec.set_noise("counter")
        dec.stream_begin(channel, seed, x)
        one = dec.stream_decode(N, early_term=False, iterations=1, decoding="BP_MS", want=("llr_in", "codeword"))
        dec.stream_begin(channel, seed, x)
        dec.stream_skip(skip)
        late = dec.stream_decode(20, early_term=False, iterations=1, decoding="BP_MS", want=("llr_in", "codeword"))
        dec.set_noise("reference")
        assert one["codeword"].any() == generator and _same(late["llr_in"], one["llr_in"][skip:skip + 20])
        cw = one["codeword"] if generator else None
        got = dec.channel_batch(cw, channel, x, seed=seed, frames=N)["llr"]
        assert _same(got, one["llr_in"]), (name, channel, x, generator)
        got = dec.channel_batch(cw[skip:skip + 20] if generator else None, channel, x, seed=seed, first_frame=skip, frames=20)["llr"]
        assert _same(got, late["llr_in"]), (name, channel, x, generator)


def test_first_frame_beyond_32_bits(codes):
    """The frame index is a 64-bit counter (two Philox counter words): the BSC is exact against the mirror."""
    name, x, seed, first = "s129x150t5", 0.24, 77, 2**32 + 3
    code, dec = codes.mirror(name), codes.decoder(name)
    cw = _random_words(code, 4, 1)
    frames = np.arange(first, first + 4, dtype=np.uint64)
    want_r, want_l = cr.bsc(code, x, seed, frames, cw)
    got = dec.channel_batch(cw, "BSC", x, seed=seed, first_frame=first, want=("llr", "received"))
    assert _same(got["llr"], want_l) and _same(got["received"], want_r)
    row = dec.channel_batch(cw[2:3], "BSC", x, seed=seed, first_frame=first + 2, want=("llr", "received"))
    assert _same(row["llr"], want_l[2:3]) and _same(row["received"], want_r[2:3])
    low = cr.bsc(code, x, seed, frames & np.uint64(0xFFFFFFFF), cw)[0]
    assert not np.array_equal(low, want_r)  # (the high word counts)


# ---- 2. the BSC against the mirror ----
@pytest.mark.parametrize("name", NAMES)
def test_bsc_equals_the_mirror(codes, name):
    code, dec = codes.mirror(name), codes.decoder(name)
    cw = _random_words(code, N, 2)
    for x, seed, first in ((0.02, 5, 0), (0.24, 6, 1000)):
        want_r, want_l = cr.bsc(code, x, seed, np.arange(first, first + N), cw)
        got = dec.channel_batch(cw, "BSC", x, seed=seed, first_frame=first, want=("llr", "received"))
        assert _same(got["received"], want_r) and _same(got["llr"], want_l), (name, x)
        flips = (want_r < 0) != (cw[:, code.bit_pos] != 0)
        assert abs(flips.mean() - x) < 5 * np.sqrt(x * (1 - x) / flips.size)


# ---- 3. the AWGN's received values against the mirror's normals ----
@pytest.mark.parametrize("m", (1, 2, 3, 4))
@pytest.mark.parametrize("name", NAMES)
def test_awgn_received_against_the_mirror(codes, name, m):
    code, dec = codes.mirror(name), codes.decoder(name)
    cw = _random_words(code, N, 3)
    for x, seed, first in ((3.0, 8, 0), (-4.0, 9, 123)):
        _, sigma = cr.awgn_params(x)
        want, radius = cr.awgn_received(code, m, x, seed, np.arange(first, first + N), cw)
        got = dec.channel_batch(cw, "AWGN", x, seed=seed, first_frame=first, bits_per_symbol=m, want=("received",))["received"]
        assert got.shape == (N, cr.symbols(m, code.nct)) == want.shape
        err = np.abs(got - want)
        assert np.all(err <= sigma * (2e-5 + 2e-7 / radius) + 1e-12), (name, m, x, float(err.max()))
        sent = cr.awgn_transmit(code, m, cw, N)
        assert len(np.unique(sent)) == 1 << m and abs(float((sent * sent).mean()) - 1.0) < 0.1


# ---- 4. the demapper, exactly, on the device's own received values ----
@pytest.mark.parametrize("m", (1, 2, 3, 4))
@pytest.mark.parametrize("name", NAMES)
def test_demapper_is_exact(codes, name, m):
    code, dec = codes.mirror(name), codes.decoder(name)
    cw = _random_words(code, N, 4)
    for x, seed in ((3.0, 10), (-4.0, 11), (14.0, 12)):
        got = dec.channel_batch(cw, "AWGN", x, seed=seed, bits_per_symbol=m, want=("llr", "received"))
        want = cr.awgn_llr(code, m, x, got["received"])
        assert _same(got["llr"], want), (name, m, x)
        assert np.array_equal(got["llr"][:, code.shorten], np.full((N, len(code.shorten)), cr.SHORTEN_AWGN))
        assert not cr.raw(got["llr"][:, code.puncture]).any()  # +0.0
        # the signs of the LLRs follow the bits sent (a negative LLR is a 1), and not all of them at -4 dB per dimension
        wrong = ((got["llr"][:, code.bit_pos] < 0) != (cw[:, code.bit_pos] != 0)).mean()
        assert wrong < (0.25 if x == 14.0 else 0.5) and (x > 0 or wrong > 0.01), (name, m, x, wrong)


# ---- 5. the element types ----
@pytest.mark.parametrize("channel, x, m", [("AWGN", 2.0, 1), ("AWGN", 6.0, 3), ("AWGN", 9.0, 4), ("BSC", 0.05, 1)])
@pytest.mark.parametrize("name", ("s129x150t5", "golden"))
def test_element_types(codes, name, channel, x, m):
    code, dec = codes.mirror(name), codes.decoder(name)
    cw = _random_words(code, N, 5)
    kw = dict(seed=13, first_frame=7, bits_per_symbol=m)
    f64 = dec.channel_batch(cw, channel, x, **kw)["llr"]
    assert f64.dtype == np.float64 and np.isfinite(f64).all()
    f32 = dec.channel_batch(cw, channel, x, llr="float32", **kw)["llr"]
    assert _same(f32, f64.astype(np.float32))
    f16 = dec.channel_batch(cw, channel, x, llr="float16", **kw)["llr"]
    with np.errstate(over="ignore"):
        assert _same(f16, f64.astype(np.float32).astype(np.float16))
    if channel == "AWGN" and code.shorten:
        assert np.isposinf(f16[:, code.shorten]).all() and np.isfinite(f16[:, code.bit_pos]).all()
    for q_bits, step in ((6, 0.25), (4, 1.0)):
        i8 = dec.channel_batch(cw, channel, x, llr="int8", q_bits=q_bits, step=step, **kw)["llr"]
        assert _same(i8, cr.quantize(f64, q_bits, step)), (q_bits, step)
        qmax = 2 ** (q_bits - 1) - 1
        if channel == "AWGN":  # (both ends saturate; the BSC's two values +-delta / step lie inside)
            assert i8.min() == -qmax and i8.max() == qmax
            assert (i8[:, code.shorten] == qmax).all()
        else:
            assert set(np.unique(i8[:, code.bit_pos])) == {-int(np.rint(cr.bsc_delta(x) / step)), int(np.rint(cr.bsc_delta(x) / step))}


# ---- 6. formats, splits, buffers ----
@pytest.mark.parametrize("channel, x, m", [("AWGN", 1.0, 1), ("AWGN", 5.0, 2), ("AWGN", 9.0, 4), ("BSC", 0.1, 1)])
def test_formats_and_splits(codes, channel, x, m):
    name = "s129x150t5"
    code, dec = codes.mirror(name), codes.decoder(name)
    assert code.nc % 32  # (a row's last word has unused high bits)
    rng = np.random.default_rng(6)
    cw = _random_words(code, N, 6)
    kw = dict(seed=14, bits_per_symbol=m, want=("llr", "received"))
    base = dec.channel_batch(cw, channel, x, first_frame=40, **kw)
    # packed input, garbage in the unused bits of a row's last word; bytes of 2 and 255
    packed = gf2_ref.pack(cw)
    packed[:, -1] |= rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32) << np.uint32(code.nc % 32)
    odd = cw * rng.choice(np.array([1, 2, 255], np.uint8), cw.shape)
    assert (odd == 2).any() and (odd == 255).any()
    for what, src in (("packed", packed), ("bytes", odd)):
        got = dec.channel_batch(src, channel, x, first_frame=40, **kw)
        assert _same(got["llr"], base["llr"]) and _same(got["received"], base["received"]), what
    # None is the all-zero codeword
    zero = dec.channel_batch(np.zeros_like(cw), channel, x, first_frame=40, **kw)
    none = dec.channel_batch(None, channel, x, first_frame=40, frames=N, **kw)
    assert _same(none["llr"], zero["llr"]) and _same(none["received"], zero["received"])
    assert not _same(zero["llr"], base["llr"])
    # one call of N frames = three calls of unequal pieces
    parts, first = [], 40
    for k in (1, 46, 23):
        lo = first - 40
        parts.append(dec.channel_batch(cw[lo:lo + k], channel, x, first_frame=first, **kw))
        first += k
    assert first == 40 + N
    for key in ("llr", "received"):
        assert _same(np.concatenate([p[key] for p in parts]), base[key]), key
    # each output by itself
    assert _same(dec.channel_batch(cw, channel, x, seed=14, first_frame=40, bits_per_symbol=m)["llr"], base["llr"])
    assert _same(dec.channel_batch(cw, channel, x, seed=14, first_frame=40, bits_per_symbol=m, want=("received",))["received"], base["received"])


def test_device_tensors_and_prefilled_buffers(codes):
    import torch
    dev = torch.device("cuda", 0)
    name = "s129x150t5"
    code, dec = codes.mirror(name), codes.decoder(name)
    cw = _random_words(code, N, 7)
    side = torch.cuda.Stream(device=dev)
    for channel, x, m in (("AWGN", 4.0, 3), ("BSC", 0.1, 1)):
        S = cr.symbols(m, code.nct)
        for llr, dt, tdt in (("float64", np.float64, torch.float64), ("float32", np.float32, torch.float32),
                             ("float16", np.float16, torch.float16), ("int8", np.int8, torch.int8)):
            kw = dict(seed=15, first_frame=3, bits_per_symbol=m, llr=llr, q_bits=5, step=0.5)
            base = dec.channel_batch(cw, channel, x, want=("llr", "received"), **kw)
            assert base["llr"].dtype == dt
            # host buffers filled with 0x7F bytes end fully overwritten
            out = {"llr": np.full((N, code.nc), 0x7F, np.uint8).repeat(np.dtype(dt).itemsize, 1).view(dt),
                   "received": np.full((N, 8 * S), 0x7F, np.uint8).view(np.float64)}
            assert out["llr"].shape == (N, code.nc) and (cr.raw(out["llr"]) & 0xFF == 0x7F).all()
            got = dec.channel_batch(cw, channel, x, want=(), out=out, **kw)
            assert got["llr"] is out["llr"] and _same(out["llr"], base["llr"]) and _same(out["received"], base["received"]), (channel, llr)
            # device tensors in and out, on torch's stream and on another
            for stream, source in ((None, torch.from_numpy(cw).to(dev)), (side.cuda_stream, torch.from_numpy(gf2_ref.pack(cw)).to(dev))):
                t_llr = torch.full((N, code.nc * np.dtype(dt).itemsize), 0x7F, dtype=torch.uint8, device=dev).view(tdt)
                t_rec = torch.full((N, 8 * S), 0x7F, dtype=torch.uint8, device=dev).view(torch.float64)
                assert tuple(t_llr.shape) == (N, code.nc) and tuple(t_rec.shape) == (N, S)
                torch.cuda.synchronize()  # (the buffers were filled on torch's stream; the call runs on `stream`)
                dec.channel_batch(source, channel, x, want=(), out={"llr": t_llr, "received": t_rec}, stream=stream, **kw)
                dec.synchronize(stream)
                assert _same(t_llr.cpu().numpy(), base["llr"]) and _same(t_rec.cpu().numpy(), base["received"]), (channel, llr, stream)


# ---- 7. the chain on device tensors ----
def test_the_chain_on_device_tensors(codes):
    import libldpc_amd
    import torch
    dev = torch.device("cuda", 0)
    code = codes.mirror("golden")
    dec = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
    n, x, seed, iterations = 200, 3.0, 16, 30
    words = (code.nc + 31) // 32
    rng = np.random.default_rng(8)
    info_np = rng.integers(0, 2, (n, code.kc), dtype=np.uint8)
    info = torch.from_numpy(info_np).to(dev)

    def u32(*shape):
        return torch.full(shape, -1, dtype=torch.int32, device=dev).view(torch.uint32)

    cw_bits = u32(n, words)
    dec.encode_batch(info, want=(), out={"codeword_bits": cw_bits})
    dec.set_min_sum_layered_fixed(6, 8, 0.25)
    runs = {}
    for kind, tdt in (("int8", torch.int8), ("float64", torch.float64)):
        llr = torch.full((n, code.nc), 99, dtype=tdt, device=dev)
        dec.channel_batch(cw_bits, "AWGN", x, seed=seed, llr=kind, q_bits=6, step=0.25, want=(), out={"llr": llr})
        out = {"iters": torch.zeros(n, dtype=torch.int32, device=dev), "bit_errors": torch.zeros(n, dtype=torch.int32, device=dev),
               "hard": torch.zeros((n, code.nc), dtype=torch.uint8, device=dev),
               "llr_out": torch.zeros((n, code.nc), dtype=torch.float64, device=dev)}
        errors, ones = u32(n), u32(n)
        zeros = torch.zeros((n, words), dtype=torch.int32, device=dev).view(torch.uint32)
        if kind == "int8":  # packed words pass from one call to the next
            out["hard_bits"] = u32(n, words)
            dec.decode_batch_typed(llr, early_term=True, iterations=iterations, decoding="BP_MS", want=(), out=out)
            dec.bit_errors_batch(out["hard_bits"], cw_bits, out=errors)
            dec.bit_errors_batch(out["hard_bits"], zeros, out=ones)
        else:
            dec.decode_batch(llr, early_term=True, iterations=iterations, decoding="BP_MS", want=(), out=out)
            dec.bit_errors_batch(out["hard"], cw_bits, out=errors)
            dec.bit_errors_batch(out["hard"], zeros, out=ones)
        torch.cuda.synchronize()
        runs[kind] = {k: v.cpu().numpy() for k, v in dict(out, errors=errors, ones=ones, llr=llr).items()}
    dec.set_min_sum_layered_fixed(0)
    a, b = runs["int8"], runs["float64"]
    cw = code.encode(info_np)
    assert np.array_equal(cw_bits.cpu().numpy(), gf2_ref.pack(cw)) and cw.any(1).all()
    assert _same(a["llr"], cr.quantize(b["llr"], 6, 0.25))
    for k in ("iters", "bit_errors", "hard", "llr_out", "errors", "ones"):
        assert _same(a[k], b[k]), k
    assert np.array_equal(a["hard_bits"], gf2_ref.pack(b["hard"]))
    # bit_errors_batch against the encoder's words is the count over the transmitted positions; against zeros it is what a
    # decode of given LLRs (no codeword of its own: the all-zero one) reports as bit_errors
    assert np.array_equal(a["errors"], code.bit_errors(a["hard"], cw))
    assert np.array_equal(a["ones"], a["bit_errors"].astype(np.uint32))
    good = (a["errors"] == 0) & (a["iters"] < iterations)
    print("chain: frames decoded without error", int(good.sum()), "of", n, "with errors", int((a["errors"] > 0).sum()))
    assert good.any()


# ---- 8. no state ----
@pytest.mark.parametrize("noise", ("reference", "counter"))
def test_the_stream_interface_is_left_alone(codes, noise):
    import libldpc_amd
    code = codes.mirror("golden")
    cw = _random_words(code, 33, 9)
    runs = []
    for between in (False, True):
        dec = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
        dec.set_noise(noise)
        dec.set_min_sum_correction(0.8125, 0.0)
        dec.stream_begin("AWGN", 9, 2.0)
        got = []
        for batch in (40, 33):
            if between:
                r = dec.channel_batch(cw, "BSC", 0.07, seed=9, want=("llr", "received"))
                assert _same(r["llr"], cr.bsc(code, 0.07, 9, np.arange(33), cw)[1])
                dec.channel_batch(cw, "AWGN", 7.0, seed=1234, first_frame=5, bits_per_symbol=4, llr="int8", q_bits=6, step=0.25)
                dec.channel_batch(None, "AWGN", -1.0, seed=9, frames=3, want=("received",))
            got.append(dec.stream_decode(batch, iterations=10, decoding="BP_MS", want=("iters", "bit_errors", "llr_in", "codeword")))
        assert dec.stream_frame == 73 and dec.min_sum_layered_fixed[0] == 0
        runs.append(got)
    for plain, mixed in zip(*runs):
        for k in ("iters", "bit_errors", "llr_in", "codeword"):
            assert _same(plain[k], mixed[k]), (noise, k)
    assert all(r["codeword"].any() for r in runs[0])
