"""ldpc_hip_erasure_solve_batch (include/ldpc_amd.h; libldpc_amd/csrc/kernels_erasure_solve.hip) on the GPU: all five outputs
against the numpy mirror of tests/erasure_ml_ref.py bit for bit — on what the erasure channel delivers and on what peeling
leaves of it, on words that are no codewords, under a cap —, the identity between solving the raw frames and solving the
peeled ones, formats, splits and buffer kinds, the chain encode -> erasure channel -> peeling -> solve -> syndrome on device
tensors, and between the batches of a running stream.

The codes, the two erasure probabilities of each, the 70 frames, the noise seed and the words() recipe are those of
test_gpu_erasure_batch.py.  The largest system is 1023 unknowns over 1020 check nodes (h.txt at 0.85 after peeling); h.txt
runs at max_unknowns = 1024, every other code at its number of columns."""
import itertools

import numpy as np
import pytest

import erasure_ml_ref as ml
import erasure_ref as er
import gf2_ref
import orc
import test_gpu_erasure_batch as peel

pytestmark = pytest.mark.gpu
NAMES, N, SEED, POINTS = peel.NAMES, peel.N, peel.SEED, peel.POINTS
KEYS = ("word", "erased", "unresolved", "rank", "status")
STALLED = er.EARLY_TERM | er.STOP_STALLED


class Frames:
    """The inputs and what the mirror makes of them, computed once and never changed."""

    def __init__(self, codes):
        self.codes, self.raw_frames, self.peeled_frames, self.solved = codes, {}, {}, {}

    def cap(self, name):
        return 1024 if name == "golden" else self.codes.mirror(name).nc

    def raw(self, name, eps):
        """What the erasure channel delivers of N codewords (the all-zero one where the code has no generator), as bytes."""
        if (name, eps) not in self.raw_frames:
            code = self.codes.mirror(name)
            cw = code.encode(np.random.default_rng(7).integers(0, 2, (N, code.kc), dtype=np.uint8)) if code.has_g else None
            w, e = er.channel(code, eps, SEED, np.arange(N), cw)
            self.raw_frames[(name, eps)] = self._frozen(w, e)
        return self.raw_frames[(name, eps)]

    def peeled(self, name, eps):
        """What the mirror of the peeling decoder, stopped when stalled, leaves of raw()."""
        if (name, eps) not in self.peeled_frames:
            r = er.decode(self.codes.mirror(name), *self.raw(name, eps), 50, STALLED)
            self.peeled_frames[(name, eps)] = self._frozen(r["word"], r["erased"])
        return self.peeled_frames[(name, eps)]

    @staticmethod
    def _frozen(w, e):
        w, e = np.ascontiguousarray(w, np.uint8), np.ascontiguousarray(e, np.uint8)
        w.setflags(write=False), e.setflags(write=False)
        return w, e

    def want(self, name, kind, eps=None, cap=None):
        """The mirror's solve() of raw / peeled frames at eps, or of the words() of the peeling tests."""
        cap = cap or self.cap(name)
        if (name, kind, eps, cap) not in self.solved:
            w, e = self.codes.words(name) if kind == "words" else getattr(self, kind)(name, eps)
            r = ml.solve(self.codes.mirror(name), w, e, cap)
            for v in r.values():
                v.setflags(write=False)
            self.solved[(name, kind, eps, cap)] = r
        return self.solved[(name, kind, eps, cap)]


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return peel.Codes(tmp_path_factory.mktemp("erasure_solve"))


@pytest.fixture(scope="module")
def frames(codes):
    return Frames(codes)


def _same(got, want):
    return all(got[k].dtype == np.uint32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)


def _differing(got, want):
    return {k: np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1)).tolist() for k in want if not np.array_equal(got[k], want[k])}


def _both_formats(codes, name, w, e, cap, want, what):
    code, dec = codes.mirror(name), codes.decoder(name)
    rng = np.random.default_rng(3)
    pw, pe = peel._garbage(gf2_ref.pack(w), code.nc, rng), peel._garbage(gf2_ref.pack(e), code.nc, rng)
    if code.nc % 32:
        assert gf2_ref.high_bits(pw, code.nc).any() and gf2_ref.high_bits(pe, code.nc).any()
    got = dec.erasure_solve_batch(w, e, max_unknowns=cap)
    assert _same(got, want), (what, "bytes", _differing(got, want))
    got = dec.erasure_solve_batch(pw, pe, max_unknowns=cap)
    assert _same(got, want), (what, "packed", _differing(got, want))
    assert not gf2_ref.high_bits(want["word"] | want["erased"], code.nc).any() and not (want["word"] & want["erased"]).any()


# ---- 1. the mirror, on the channel's frames and on what peeling leaves of them ----
def test_the_mirror_shows_every_class(frames):
    """Before any kernel runs: the frames hold what the tests below are about."""
    for name, eps in (("golden", 0.85), ("r240", 0.45)):
        stuck = (frames.peeled(name, eps)[1] != 0).any(1)
        status = frames.want(name, "peeled", eps)["status"][stuck]
        assert (status == ml.SOLVED).sum() >= 10 and (status == ml.PARTIAL).sum() >= 2 and set(status) == {ml.SOLVED, ml.PARTIAL}, (name, eps)
    left = (frames.peeled("golden", 0.85)[1] != 0).sum(1)
    assert left.max() == 1023 and (frames.raw("golden", 0.85)[1] != 0).sum(1).max() > 1024  # the largest system; frames over the cap
    assert (frames.want("golden", "raw", 0.85)["status"] == ml.TOO_LARGE).any()
    stuck = (frames.peeled("s40x60", 0.4)[1] != 0).sum(1)
    after = frames.want("s40x60", "peeled", 0.4)["unresolved"]
    assert ((stuck > 0) & (after == stuck)).any() and (after <= stuck).all()  # frames with nothing recovered


@pytest.mark.parametrize("name", NAMES)
def test_solver_equals_the_mirror(codes, frames, name):
    for eps in POINTS[name]:
        for kind in ("raw", "peeled"):
            w, e = getattr(frames, kind)(name, eps)
            _both_formats(codes, name, w, e, frames.cap(name), frames.want(name, kind, eps), (name, eps, kind))


# ---- 2. words that are no codewords ----
@pytest.mark.parametrize("name", NAMES)
def test_words_that_are_no_codewords(codes, frames, name):
    code = codes.mirror(name)
    w, e = codes.words(name)
    want = frames.want(name, "words")
    bad = want["status"] == ml.INCONSISTENT
    assert bad.any() and (want["status"] == ml.SOLVED).any() and (want["status"] != ml.INCONSISTENT).sum() >= 10, name
    assert want["status"][68] in (ml.SOLVED, ml.INCONSISTENT) and want["rank"][68] == 0 and want["unresolved"][68] == 0  # no erasures
    assert want["status"][69] == (ml.TOO_LARGE if name == "golden" else ml.PARTIAL) and want["unresolved"][69] == code.nc  # all erased
    _both_formats(codes, name, w, e, frames.cap(name), want, (name, "words"))
    got = codes.decoder(name).erasure_solve_batch(w, e, max_unknowns=frames.cap(name))
    assert np.array_equal(got["erased"][bad], gf2_ref.pack(e)[bad]) and np.array_equal(got["word"][bad], gf2_ref.pack((w != 0) & (e == 0))[bad])
    assert np.array_equal(got["unresolved"][bad], (e != 0).sum(1)[bad])


# ---- 3. the cap ----
def test_the_cap(codes, frames):
    """The words() of the peeling tests (mostly inconsistent) and, behind them, the all-zero codeword through a channel that
    erases about 14 columns a frame: frames on both sides of 16 unknowns, solvable ones among those within."""
    name, cap = "r240", 16
    code, dec = codes.mirror(name), codes.decoder(name)
    few = er.channel(code, 0.06, SEED, np.arange(N))
    w, e = (np.concatenate([a, b.astype(np.uint8)]) for a, b in zip(codes.words(name), few))
    ne = (e != 0).sum(1)
    over = ne > cap
    full, want = ml.solve(code, w, e, code.nc), ml.solve(code, w, e, cap)
    assert over.sum() >= 20 and (ne == cap).any() and (ne == cap + 1).any()
    assert set(full["status"][~over]) == {ml.SOLVED, ml.INCONSISTENT} and (full["status"][~over & (ne > 0)] == ml.SOLVED).sum() >= 10
    got = dec.erasure_solve_batch(w, e, max_unknowns=cap)
    assert _same(got, want), _differing(got, want)
    assert (got["status"][over] == ml.TOO_LARGE).all() and not got["rank"][over].any() and (got["status"][~over] != ml.TOO_LARGE).all()
    assert np.array_equal(got["erased"][over], gf2_ref.pack(e)[over]) and np.array_equal(got["word"][over], gf2_ref.pack((w != 0) & (e == 0))[over])
    assert np.array_equal(got["unresolved"][over], ne[over])
    uncapped = dec.erasure_solve_batch(w, e)
    assert _same(uncapped, full), _differing(uncapped, full)
    for key in KEYS:
        assert np.array_equal(got[key][~over], uncapped[key][~over]), key
    assert _same(dec.erasure_solve_batch(w, e, max_unknowns=code.nc + 1000), full)  # above nc counts as nc


# ---- 4. solving the raw frames and solving the peeled frames ----
@pytest.mark.parametrize("name,eps", (("r240", 0.45), ("r240", 0.4), ("s129x150t5", 0.35), ("golden", 0.82)))
def test_raw_and_peeled_frames_solve_alike(codes, frames, name, eps):
    dec, cap = codes.decoder(name), frames.cap(name)
    w, e = frames.raw(name, eps)
    assert (e != 0).sum(1).max() <= cap  # (on the mirror: no frame exceeds the cap, before or after peeling)
    raw = dec.erasure_solve_batch(w, e, max_unknowns=cap)
    peeled = dec.erasure_decode_batch(w, e, iterations=50, early_term=True, stop_stalled=True)
    assert np.array_equal(peeled["erased"], gf2_ref.pack(frames.peeled(name, eps)[1]))
    after = dec.erasure_solve_batch(peeled["word"], peeled["erased"], max_unknowns=cap)
    for key in ("word", "erased", "unresolved", "status"):
        assert np.array_equal(raw[key], after[key]), (name, key)
    moved = peeled["unresolved"] < (e != 0).sum(1)
    assert moved.any() and (after["rank"][moved] < raw["rank"][moved]).all() and np.array_equal(after["rank"][~moved], raw["rank"][~moved])
    assert (after["unresolved"] <= peeled["unresolved"]).all() and not (after["status"] >= ml.INCONSISTENT).any()


# ---- 5. buffers, formats, splits ----
@pytest.mark.parametrize("name", ("golden", "s40x60"))
def test_rows_of_a_call_are_the_call_on_the_rows(codes, frames, name):
    dec, cap = codes.decoder(name), frames.cap(name)
    w, e = codes.words(name)
    pw, pe = gf2_ref.pack(w), gf2_ref.pack(e)
    want = frames.want(name, "words")
    for a, b in ((0, 1), (5, 47), (69, 70)):
        got = dec.erasure_solve_batch(pw[a:b], pe[a:b], max_unknowns=cap)
        assert _same(got, {k: want[k][a:b] for k in KEYS}), (name, a, b)
    empty = dec.erasure_solve_batch(pw[:0], pe[:0], max_unknowns=cap)
    assert set(empty) == set(KEYS) and empty["word"].shape == (0, pw.shape[1]) and empty["status"].shape == (0,)
    if name == "s40x60":  # every subset of the outputs
        for count in range(len(KEYS) + 1):
            for keys in itertools.combinations(KEYS, count):
                got = dec.erasure_solve_batch(pw, pe, max_unknowns=cap, want=keys)
                assert set(got) == set(keys) and _same(got, {k: want[k] for k in keys}), keys


def test_device_tensors_and_prefilled_buffers(codes, frames):
    import torch
    dev = torch.device("cuda", 0)
    name = "s129x150t5"
    code, dec = codes.mirror(name), codes.decoder(name)
    w, e = codes.words(name)
    words = (code.nc + 31) // 32
    want = frames.want(name, "words")
    side = torch.cuda.Stream(device=dev)

    def filled(*shape):
        return torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device=dev).view(torch.uint32)

    out = {k: np.full(want[k].shape, 0x7F7F7F7F, np.uint32) for k in KEYS}  # host buffers end fully overwritten
    got = dec.erasure_solve_batch(w, e, want=(), out=out)
    assert got["word"] is out["word"] and _same(out, want)
    for stream, fmt in ((None, "bytes"), (side.cuda_stream, "packed")):
        tw, te = (torch.from_numpy(x.copy() if fmt == "bytes" else gf2_ref.pack(x).view(np.int32)).to(dev) for x in (w, e))
        if fmt == "packed":
            tw, te = tw.view(torch.uint32), te.view(torch.uint32)
        out = {"word": filled(N, words), "erased": filled(N, words), "unresolved": filled(N), "rank": filled(N), "status": filled(N)}
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream; the call runs on `stream`)
        dec.erasure_solve_batch(tw, te, want=(), out=out, stream=stream)
        dec.synchronize(stream)
        assert _same({k: v.view(torch.int32).cpu().numpy().view(np.uint32) for k, v in out.items()}, want), fmt


# ---- 6. the pipeline on device tensors ----
@pytest.mark.parametrize("name,eps", (("golden", 0.85), ("s129x150t5", 0.3)))
def test_the_pipeline_on_device_tensors(codes, frames, name, eps):
    """s129x150t5: every stopping set of this code that the channel's frames meet holds a codeword (its check matrix ends in
    150 columns of degree 1), so elimination completes no frame that peeling left — it fills bits, which is what is asserted
    there; on h.txt it completes frames."""
    import torch
    dev = torch.device("cuda", 0)
    code, dec = codes.mirror(name), codes.decoder(name)
    n, words = 100, (code.nc + 31) // 32
    info_np = np.random.default_rng(8).integers(0, 2, (n, code.kc), dtype=np.uint8)
    info = torch.from_numpy(info_np).to(dev)

    def u32(*shape):
        return torch.full(shape, -1, dtype=torch.int32, device=dev).view(torch.uint32)

    cw, word, erased, mid_word, mid_erased, word_out, erased_out = (u32(n, words) for _ in range(7))
    mid_left, left, rank, status, weight, errors = (u32(n) for _ in range(6))
    dec.encode_batch(info, want=(), out={"codeword_bits": cw})
    dec.erasure_channel_batch(cw, eps, seed=16, want=(), out={"word": word, "erased": erased})
    dec.erasure_decode_batch(word, erased, iterations=50, stop_stalled=True, want=(),
                             out={"word": mid_word, "erased": mid_erased, "unresolved": mid_left})
    dec.erasure_solve_batch(mid_word, mid_erased, max_unknowns=frames.cap(name), want=(),
                            out={"word": word_out, "erased": erased_out, "unresolved": left, "rank": rank, "status": status})
    dec.syndrome_batch(word_out, want=(), out={"weight": weight})
    dec.bit_errors_batch(word_out, cw, out=errors)
    torch.cuda.synchronize()
    host = {k: v.view(torch.int32).cpu().numpy().view(np.uint32) for k, v in
            dict(cw=cw, mid_word=mid_word, mid_erased=mid_erased, mid_left=mid_left, word_out=word_out, erased_out=erased_out, left=left,
                 rank=rank, status=status, weight=weight, errors=errors).items()}
    assert np.array_equal(host["cw"], gf2_ref.pack(code.encode(info_np)))
    assert set(host["status"]) <= {ml.SOLVED, ml.PARTIAL}  # codewords with erasures are consistent, and within the cap
    done = host["status"] == ml.SOLVED
    assert np.array_equal(done, host["left"] == 0)
    assert not host["weight"][done].any() and not host["errors"][done].any() and (host["errors"] <= host["left"]).all()
    assert np.array_equal(host["word_out"][done], host["cw"][done]) and not host["erased_out"][done].any()
    before = host["mid_left"] == 0
    assert (done | ~before).all() and 0 < before.sum() < n
    if name == "golden":
        assert done.sum() > before.sum()  # strictly more frames complete than after peeling
    assert host["left"].sum() < host["mid_left"].sum() and (host["left"] <= host["mid_left"]).all()
    want = ml.solve(code, gf2_ref.unpack(host["mid_word"], code.nc), gf2_ref.unpack(host["mid_erased"], code.nc), frames.cap(name))
    assert _same({"word": host["word_out"], "erased": host["erased_out"], "unresolved": host["left"], "rank": host["rank"],
                  "status": host["status"]}, want)


# ---- 7. no state ----
def test_the_stream_interface_is_left_alone(codes, frames):
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
                assert _same(dec.erasure_solve_batch(w, e, max_unknowns=1024), frames.want("golden", "words"))
            got.append(dec.stream_decode(batch, iterations=10, decoding="BP", want=("iters", "bit_errors", "llr_in", "llr_out", "codeword")))
        assert dec.stream_frame == 73
        runs.append(got)
    for plain, mixed in zip(*runs):
        for k in ("iters", "bit_errors", "llr_in", "llr_out", "codeword"):
            assert plain[k].dtype == mixed[k].dtype and np.array_equal(plain[k], mixed[k]), k
    assert all(r["codeword"].any() for r in runs[0])
