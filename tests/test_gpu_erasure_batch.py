"""ldpc_hip_erasure_channel_batch and ldpc_hip_erasure_decode_batch (include/ldpc_amd.h; libldpc_amd/csrc/kernels_erasure.hip)
on the GPU: the channel and the decoder against the stream's BEC under counter noise (bit for bit, iteration counts
included), all four outputs of the decoder against the numpy mirror of tests/erasure_ref.py on words that are no codewords,
over the input formats, splits and buffer kinds, chained between the encoder and the syndrome on device tensors, the
stalled stop, and between the batches of a running stream.

The codes: tests/golden/h.txt (128 punctured columns, column degrees 1 / 2 / 15: the four-lane column chunks; 36 words),
s40x60 (nc = 100: a last word of 4 bits), s129x150t5 (nc = 284, 5 shortened columns), s40x60_dup (entries of G listed twice),
s40x60_hdup (entries of H listed twice and three times: parallel edges), s800x100 (check nodes of degree 9..20, uneven
inside a chunk) and a (3,6)-regular code of 240 columns.  70 frames are two groups and six frames; 1, 31, 32 and 33 frames
are a partial group, exactly one, and one frame into a second."""
import os
import sys

import numpy as np
import pytest

import erasure_ref as er
import generator_codes as gc
import gf2_ref
import orc

pytestmark = pytest.mark.gpu
NAMES = ("golden", "s40x60", "s129x150t5", "s40x60_dup", "s800x100", "r240", "s40x60_hdup")
N = 70
SEED = 31
# two erasure probabilities per code at which, by the mirror, some of the 70 frames resolve and some do not (asserted below)
POINTS = {"golden": (0.82, 0.85), "s40x60": (0.2, 0.4), "s129x150t5": (0.2, 0.35), "s40x60_dup": (0.2, 0.4),
          "s800x100": (0.01, 0.03), "r240": (0.4, 0.45), "s40x60_hdup": (0.2, 0.4)}
STREAM_NAMES = ("golden", "s40x60", "r240")  # no shortened columns: the stream's channel is the contract's
FLAGS = (0, er.EARLY_TERM, er.STOP_STALLED, er.EARLY_TERM | er.STOP_STALLED)
KEYS = ("word", "erased", "iters", "unresolved")


class Codes:
    def __init__(self, directory):
        sys.path.insert(0, os.path.join(orc.ROOT, "tools"))
        import gen_regular_code
        regular = os.path.join(str(directory), "r240.h.txt")
        open(regular, "w").write(gen_regular_code.generate(240, 3, 6, 1))
        self.files = {"golden": (orc.H_TXT, orc.G_TXT), "r240": (regular, "")}
        for name in NAMES[1:5]:
            self.files[name] = gc.write_pair(directory, name)
        self.files["s40x60_hdup"] = (er.repeat_entries(self.files["s40x60"][0], os.path.join(str(directory), "s40x60_hdup.h.txt")), "")
        self.mirrors, self.decoders, self.inputs, self.expected = {}, {}, {}, {}

    def mirror(self, name):
        if name not in self.mirrors:
            self.mirrors[name] = gf2_ref.Gf2Code(*self.files[name])
        return self.mirrors[name]

    def decoder(self, name, generator=True):
        import libldpc_amd
        generator = generator and bool(self.files[name][1])
        if (name, generator) not in self.decoders:
            h, g = self.files[name]
            self.decoders[(name, generator)] = libldpc_amd.HipDecoder(h, g if generator else "")
        return self.decoders[(name, generator)]

    def words(self, name):
        """word[N][nc], erased[N][nc] bytes that are no codewords with erasures: the channel's erasures of a codeword for the
        first rows, then random erasures, random bits, value bits under erased bits, bytes other than 0 and 1; one row
        without erasures and one all erased.  Computed once per code, never changed."""
        if name not in self.inputs:
            code = self.mirror(name)
            rng = np.random.default_rng(len(name))
            cw = code.encode(rng.integers(0, 2, (N, code.kc), dtype=np.uint8)) if code.has_g else np.zeros((N, code.nc), np.uint8)
            w, e = er.channel(code, POINTS[name][0], SEED, np.arange(N), cw)
            w, e = w.astype(np.uint8), e.astype(np.uint8)
            e[20:45] = rng.random((25, code.nc)) < rng.uniform(0.0, 2 * POINTS[name][1], (25, 1))
            w[30:] = rng.integers(0, 2, (N - 30, code.nc))           # (value bits under erased bits among them)
            w[10:20] |= e[10:20]
            w[50:60] *= rng.integers(1, 256, (10, code.nc), dtype=np.uint8)
            e[50:60] *= rng.integers(1, 256, (10, code.nc), dtype=np.uint8)
            e[68], e[69] = 0, 1
            w.setflags(write=False), e.setflags(write=False)
            self.inputs[name] = (w, e)
        return self.inputs[name]

    def want(self, name, iterations, flags):
        if (name, iterations, flags) not in self.expected:
            self.expected[(name, iterations, flags)] = er.decode_packed(self.mirror(name), *self.words(name), iterations, flags)
        return self.expected[(name, iterations, flags)]


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return Codes(tmp_path_factory.mktemp("erasure"))


def _same(got, want):
    return all(got[k].dtype == np.uint32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)


def _garbage(packed, nc, rng):
    """The packed rows with random bits from nc on in every row's last word."""
    out = packed.copy()
    if nc % 32:
        out[:, -1] |= rng.integers(0, 2**32, out.shape[0], dtype=np.uint64).astype(np.uint32) << np.uint32(nc % 32)
    return out


def test_the_codes_cover_the_paths(codes):
    golden = codes.mirror("golden")
    degree = np.bincount(golden.h_cols, minlength=golden.nc)
    assert len(golden.puncture) == 128 and sorted(set(degree)) == [1, 2, 15] and (golden.nc + 31) // 32 == 36
    assert codes.mirror("s40x60").nc == 100 and len(codes.mirror("s129x150t5").shorten) == 5 and codes.mirror("s129x150t5").nc == 284
    dup = codes.mirror("s40x60_hdup")
    assert er.incidence(dup).max() == 3 and (er.incidence(dup) == 2).sum() == 1 and er.incidence(codes.mirror("s40x60")).max() == 1
    wide = np.bincount(codes.mirror("s800x100").h_rows)
    assert wide.min() > 8 and wide.max() >= 19 and np.unique(wide).size >= 4  # (uneven trip counts inside a chunk)
    r = codes.mirror("r240")
    assert set(np.bincount(r.h_cols)) == {3} and set(np.bincount(r.h_rows)) == {6}
    for name in NAMES:  # both classes of frames at both points, on the mirror
        code = codes.mirror(name)
        for eps in POINTS[name]:
            w, e = er.channel(code, eps, SEED, np.arange(N))
            left = er.decode(code, w, e, 50, er.EARLY_TERM)["unresolved"]
            assert 0 < (left > 0).sum() < N, (name, eps)


# ---- 1. and 2. the stream's BEC under counter noise: its channel, and its decoder without the genie ----
def _stream(dec, eps, count, skip, iterations, early):
    dec.set_noise("counter")
    dec.stream_begin("BEC", SEED, eps)
    if skip:
        dec.stream_skip(skip)
    out = dec.stream_decode(count, early_term=early, iterations=iterations, decoding="BP", want=("iters", "llr_in", "llr_out", "codeword"))
    dec.set_noise("reference")
    return out


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_channel_is_the_streams(codes, name):
    code = codes.mirror(name)
    skip = 9
    for generator in ((True, False) if code.has_g else (False,)):
        dec = codes.decoder(name, generator)
        for eps in POINTS[name]:
            one = _stream(dec, eps, N, 0, 1, False)
            late = _stream(dec, eps, 20, skip, 1, False)
            assert one["codeword"].any() == generator and np.array_equal(late["llr_in"], one["llr_in"][skip:skip + 20])
            for ref, first, count in ((one, 0, N), (late, skip, 20)):
                cw = ref["codeword"] if generator else None
                got = dec.erasure_channel_batch(cw, eps, seed=SEED, first_frame=first, frames=count)
                assert np.array_equal(got["erased"], gf2_ref.pack(ref["llr_in"] == 69)), (name, eps, generator, first)
                assert np.array_equal(got["word"], gf2_ref.pack(ref["llr_in"] == 1)), (name, eps, generator, first)
                m = er.channel(code, eps, SEED, np.arange(first, first + count), cw)
                assert np.array_equal(got["word"], gf2_ref.pack(m[0])) and np.array_equal(got["erased"], gf2_ref.pack(m[1]))


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_decoder_is_the_streams_without_the_genie(codes, name):
    code = codes.mirror(name)
    for generator in ((True, False) if code.has_g else (False,)):
        dec = codes.decoder(name, generator)
        for eps in POINTS[name]:
            for iterations in (1, 3, 50):
                for early in (True, False):
                    ref = _stream(dec, eps, N, 0, iterations, early)
                    cw = ref["codeword"] if generator else None
                    if iterations == 50 and early:
                        w, e = er.channel(code, eps, SEED, np.arange(N), cw)
                        left = er.decode(code, w, e, 50, er.EARLY_TERM)["unresolved"]
                        assert 0 < (left > 0).sum() < N, (name, eps)  # frames that resolve and frames that do not
                    ch = dec.erasure_channel_batch(cw, eps, seed=SEED, frames=N)
                    got = dec.erasure_decode_batch(ch["word"], ch["erased"], iterations=iterations, early_term=early)
                    what = (name, eps, generator, iterations, early)
                    assert np.array_equal(got["iters"], ref["iters"].astype(np.uint32)), what
                    assert np.array_equal(got["erased"], gf2_ref.pack(ref["llr_out"] == 69)), what
                    assert np.array_equal(got["word"], gf2_ref.pack(ref["llr_out"] == 1)), what
                    assert np.array_equal(got["unresolved"], (ref["llr_out"] == 69).sum(1)), what


# ---- 3. the mirror, on words that are no codewords ----
@pytest.mark.parametrize("name", NAMES)
def test_decoder_equals_the_mirror(codes, name):
    code, dec = codes.mirror(name), codes.decoder(name)
    w, e = codes.words(name)
    rng = np.random.default_rng(3)
    pw, pe = _garbage(gf2_ref.pack(w), code.nc, rng), _garbage(gf2_ref.pack(e), code.nc, rng)
    if code.nc % 32:
        assert gf2_ref.high_bits(pw, code.nc).any() and gf2_ref.high_bits(pe, code.nc).any()
    for flags in FLAGS:
        kw = dict(early_term=bool(flags & er.EARLY_TERM), stop_stalled=bool(flags & er.STOP_STALLED))
        for iterations in (0, 1, 50):
            want = codes.want(name, iterations, flags)
            assert _same(dec.erasure_decode_batch(pw, pe, iterations=iterations, **kw), want), (name, flags, iterations, "packed")
            assert _same(dec.erasure_decode_batch(w, e, iterations=iterations, **kw), want), (name, flags, iterations, "bytes")
            assert not gf2_ref.high_bits(want["word"], code.nc).any() and not (want["word"] & want["erased"]).any()
    full = codes.want(name, 50, er.EARLY_TERM)
    assert (full["unresolved"] == 0).any() and (full["unresolved"] > 0).any() and full["iters"].max() > 1
    zero = codes.want(name, 0, 0)
    assert np.array_equal(zero["erased"], gf2_ref.pack(e)) and np.array_equal(zero["word"], gf2_ref.pack((w != 0) & (e == 0)))
    assert not zero["iters"].any() and np.array_equal(zero["unresolved"], (e != 0).sum(1))


@pytest.mark.parametrize("name", ("golden", "s129x150t5", "s40x60"))
def test_channel_equals_the_mirror(codes, name):
    """Shortened columns carry their own bit; a 64-bit frame index; padding bits 0."""
    code, dec = codes.mirror(name), codes.decoder(name)
    rng = np.random.default_rng(4)
    cw = code.encode(rng.integers(0, 2, (N, code.kc), dtype=np.uint8))
    cw[N - 1] = 1
    for eps, seed, first in ((POINTS[name][0], 5, 0), (0.5, 2**40 + 6, 2**32 + 3)):
        w, e = er.channel(code, eps, seed, np.arange(first, first + N, dtype=np.uint64), cw)
        want = {"word": gf2_ref.pack(w), "erased": gf2_ref.pack(e)}
        assert _same(dec.erasure_channel_batch(cw, eps, seed=seed, first_frame=first), want), (name, eps, "bytes")
        assert _same(dec.erasure_channel_batch(_garbage(gf2_ref.pack(cw), code.nc, rng), eps, seed=seed, first_frame=first), want), (name, eps)
        none = dec.erasure_channel_batch(None, eps, seed=seed, first_frame=first, frames=N)
        assert np.array_equal(none["erased"], want["erased"]) and not none["word"].any()
        only = dec.erasure_channel_batch(cw, eps, seed=seed, first_frame=first, want=("erased",))
        assert set(only) == {"erased"} and np.array_equal(only["erased"], want["erased"])
        only = dec.erasure_channel_batch(cw, eps, seed=seed, first_frame=first, want=("word",))
        assert set(only) == {"word"} and np.array_equal(only["word"], want["word"])
    if code.shorten:
        assert cw[:, code.shorten].any() and np.array_equal(w[:, code.shorten], cw[:, code.shorten] != 0)


# ---- 4. buffers, formats, splits ----
@pytest.mark.parametrize("name", ("golden", "s40x60"))
def test_rows_of_a_call_are_the_call_on_the_rows(codes, name):
    code, dec = codes.mirror(name), codes.decoder(name)
    w, e = codes.words(name)
    pw, pe = gf2_ref.pack(w), gf2_ref.pack(e)
    kw = dict(iterations=50, early_term=True, stop_stalled=False)
    want = codes.want(name, 50, er.EARLY_TERM)
    for a, b in ((0, 1), (0, 31), (0, 32), (0, 33), (5, 47), (37, 70), (69, 70)):
        got = dec.erasure_decode_batch(pw[a:b], pe[a:b], **kw)
        assert _same(got, {k: want[k][a:b] for k in KEYS}), (name, a, b)
        ch = dec.erasure_channel_batch(w[a:b], 0.3, seed=2, first_frame=100 + a)
        assert _same(ch, {k: v[a:b] for k, v in dec.erasure_channel_batch(w, 0.3, seed=2, first_frame=100).items()})
    # n == 0, and every subset of the outputs
    empty = dec.erasure_decode_batch(pw[:0], pe[:0], **kw)
    assert empty["word"].shape == (0, pw.shape[1]) and empty["iters"].shape == (0,)
    for key in KEYS:
        got = dec.erasure_decode_batch(pw, pe, want=(key,), **kw)
        assert set(got) == {key} and np.array_equal(got[key], want[key]), key
    assert dec.erasure_decode_batch(pw, pe, want=(), **kw) == {}


def test_device_tensors_and_prefilled_buffers(codes):
    import torch
    dev = torch.device("cuda", 0)
    name = "s129x150t5"
    code, dec = codes.mirror(name), codes.decoder(name)
    w, e = codes.words(name)
    words = (code.nc + 31) // 32
    want = codes.want(name, 50, er.EARLY_TERM | er.STOP_STALLED)
    ch_want = dec.erasure_channel_batch(w, 0.3, seed=15, first_frame=3)
    side = torch.cuda.Stream(device=dev)

    def filled(*shape):
        return torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device=dev).view(torch.uint32)

    # host buffers filled with 0x7F bytes end fully overwritten
    out = {k: np.full(want[k].shape, 0x7F7F7F7F, np.uint32) for k in KEYS}
    got = dec.erasure_decode_batch(w, e, stop_stalled=True, want=(), out=out)
    assert got["word"] is out["word"] and _same(out, want)
    for stream, fmt in ((None, "bytes"), (side.cuda_stream, "packed")):
        tw, te = (torch.from_numpy(x.copy() if fmt == "bytes" else gf2_ref.pack(x).view(np.int32)).to(dev) for x in (w, e))
        if fmt == "packed":
            tw, te = tw.view(torch.uint32), te.view(torch.uint32)
        out = {"word": filled(N, words), "erased": filled(N, words), "iters": filled(N), "unresolved": filled(N)}
        ch = {"word": filled(N, words), "erased": filled(N, words)}
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream; the calls run on `stream`)
        dec.erasure_decode_batch(tw, te, stop_stalled=True, want=(), out=out, stream=stream)
        dec.erasure_channel_batch(tw, 0.3, seed=15, first_frame=3, want=(), out=ch, stream=stream)
        dec.synchronize(stream)
        assert _same({k: v.view(torch.int32).cpu().numpy().view(np.uint32) for k, v in out.items()}, want), fmt
        assert _same({k: v.view(torch.int32).cpu().numpy().view(np.uint32) for k, v in ch.items()}, ch_want), fmt


# ---- 5. the pipeline on device tensors ----
@pytest.mark.parametrize("name", ("golden", "s129x150t5"))
def test_the_pipeline_on_device_tensors(codes, name):
    import torch
    dev = torch.device("cuda", 0)
    code, dec = codes.mirror(name), codes.decoder(name)
    n, words = 200, (code.nc + 31) // 32
    info_np = np.random.default_rng(8).integers(0, 2, (n, code.kc), dtype=np.uint8)
    info = torch.from_numpy(info_np).to(dev)

    def u32(*shape):
        return torch.full(shape, -1, dtype=torch.int32, device=dev).view(torch.uint32)

    cw, word, erased, word_out, erased_out = (u32(n, words) for _ in range(5))
    iters, left, weight, errors = (u32(n) for _ in range(4))
    eps = POINTS[name][1]
    dec.encode_batch(info, want=(), out={"codeword_bits": cw})
    dec.erasure_channel_batch(cw, eps, seed=16, want=(), out={"word": word, "erased": erased})
    dec.erasure_decode_batch(word, erased, iterations=50, want=(),
                             out={"word": word_out, "erased": erased_out, "iters": iters, "unresolved": left})
    dec.syndrome_batch(word_out, want=(), out={"weight": weight})
    dec.bit_errors_batch(word_out, cw, out=errors)
    torch.cuda.synchronize()
    host = {k: v.view(torch.int32).cpu().numpy().view(np.uint32) for k, v in
            dict(cw=cw, word=word, erased=erased, word_out=word_out, erased_out=erased_out, iters=iters, left=left, weight=weight,
                 errors=errors).items()}
    truth = code.encode(info_np)
    assert np.array_equal(host["cw"], gf2_ref.pack(truth)) and truth.any(1).all()
    done = host["left"] == 0
    assert 0 < done.sum() < n
    assert not host["weight"][done].any() and not host["errors"][done].any() and (host["errors"] <= host["left"]).all()
    assert np.array_equal(host["word_out"][done], host["cw"][done]) and not host["erased_out"][done].any()
    assert (host["errors"] > 0).any()  # an erased 1 that stays erased counts: word_out holds 0 there
    want = er.decode_packed(code, gf2_ref.unpack(host["word"], code.nc), gf2_ref.unpack(host["erased"], code.nc), 50, er.EARLY_TERM)
    assert _same({"word": host["word_out"], "erased": host["erased_out"], "iters": host["iters"], "unresolved": host["left"]}, want)


# ---- 6. the stalled stop ----
@pytest.mark.parametrize("name", NAMES)
def test_stalled_stop_changes_nothing_but_iters(codes, name):
    dec = codes.decoder(name)
    w, e = codes.words(name)
    for early in (False, True):
        base = dec.erasure_decode_batch(w, e, iterations=50, early_term=early)
        stop = dec.erasure_decode_batch(w, e, iterations=50, early_term=early, stop_stalled=True)
        for key in ("word", "erased", "unresolved"):
            assert np.array_equal(base[key], stop[key]), (name, early, key)
        assert (stop["iters"] <= base["iters"]).all() and (stop["iters"] < base["iters"]).any()
        flags = er.EARLY_TERM if early else 0
        assert np.array_equal(stop["iters"], codes.want(name, 50, flags | er.STOP_STALLED)["iters"])
        assert np.array_equal(base["iters"], codes.want(name, 50, flags)["iters"])
        if not early:
            assert (base["iters"] == 50).all()


# ---- no state ----
def test_the_stream_interface_is_left_alone(codes):
    import libldpc_amd
    w, e = codes.words("golden")
    runs = []
    for between in (False, True):
        dec = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
        dec.set_noise("counter")
        dec.stream_begin("BEC", 9, 0.8)
        got = []
        for batch in (40, 33):
            if between:
                dec.erasure_channel_batch(w, 0.2, seed=9, first_frame=7)
                r = dec.erasure_decode_batch(w, e, iterations=50, stop_stalled=True)
                assert _same(r, codes.want("golden", 50, er.EARLY_TERM | er.STOP_STALLED))
            got.append(dec.stream_decode(batch, iterations=10, decoding="BP", want=("iters", "bit_errors", "llr_in", "llr_out", "codeword")))
        assert dec.stream_frame == 73
        runs.append(got)
    for plain, mixed in zip(*runs):
        for k in ("iters", "bit_errors", "llr_in", "llr_out", "codeword"):
            assert plain[k].dtype == mixed[k].dtype and np.array_equal(plain[k], mixed[k]), k
    assert all(r["codeword"].any() for r in runs[0])
