"""ldpc_hip_osd_syndrome_batch (include/ldpc_amd.h; libldpc_amd/csrc/kernels_osd_syndrome.hip) on the GPU: all five outputs
against the numpy mirror of tests/osd_syndrome_ref.py bit for bit — on the soft output and on the channel LLRs of frames that
the mirror of ldpc_hip_syndrome_decode_batch decoded toward their syndromes, some reaching them and some not —, the
identities with ldpc_hip_osd_batch kernel against kernel, the syndrome of every word, ties and special values under non-zero
syndromes, syndrome formats, element types, buffer kinds, NULL outputs, splits, refusals and the LDS formula.

The codes and the Codes fixture are those of test_gpu_erasure_batch.py: tests/golden/h.txt (nc a multiple of 64: no spare bit
in a row's matrix words; rank 1021 of 1024 check nodes; 159 920 bytes of LDS: the edge), s40x60 (a last word of 4 bits),
s40x60_hdup (parallel edges), s129x150t5 (shortened columns) and the (3,6)-regular code of 240 columns.  70 frames per code,
24 for h.txt with pair_depth <= 8 there.  Frames are random words x (no codewords) through channel_ref's BSC (counter noise
of seed 31) with s = H x, at a point per code where, by the mirrors alone, some frames reach s and some do not (asserted
below before any kernel runs)."""
import itertools

import numpy as np
import pytest

import channel_ref as cr
import gf2_ref
import osd_ref as osd
import osd_syndrome_ref as osr
import syndrome_decode_ref as sdr
import test_gpu_erasure_batch as peel
import test_gpu_osd as plain
from test_osd_syndrome_host import formula

pytestmark = pytest.mark.gpu
NAMES = ("golden", "s40x60", "s40x60_hdup", "s129x150t5", "r240")
SMALL = NAMES[1:]
SEED, X_SEED = 31, 5
POINTS = {"golden": 0.19, "s40x60": 0.06, "s40x60_hdup": 0.06, "s129x150t5": 0.03, "r240": 0.06}  # the BSC's crossover probability
MIN_SUM = dict(bits=6, step=0.25, scale=0.8125, offset=0.0, early_term=True, iterations=20)
KEYS = osr.KEYS


def frames_of(name):
    return 24 if name == "golden" else 70


class Inputs:
    """The frames and what the mirrors make of them, computed once and never changed."""

    def __init__(self, codes):
        self.codes, self.decoded, self.expected = codes, {}, {}

    def settings(self, name):
        nc = self.codes.mirror(name).nc
        return ((0, 0), (1, 0), (64, 0), (0, 2), (64, 8), (nc, 8)) + (((64, 256),) if name != "golden" else ())

    def frames(self, name):
        """dict(x, s, llr_in, llr_out, failed): N random words, their syndromes, their LLRs behind the BSC, and what 20
        iterations of quantized min-sum toward s leave of them (the mirror of ldpc_hip_syndrome_decode_batch)."""
        if name not in self.decoded:
            code, n = self.codes.mirror(name), frames_of(name)
            x = np.random.default_rng(X_SEED).integers(0, 2, (n, code.nc), dtype=np.uint8)
            s, _ = code.syndrome(x)
            _, llr_in = cr.bsc(code, POINTS[name], SEED, np.arange(n), x)
            r = sdr.SyndromeDecodeMirror(sdr.graph(self.codes.files[name][0])).decode_toward(llr_in, s, **MIN_SUM)
            out = {"x": x, "s": np.ascontiguousarray(s, np.uint8), "llr_in": llr_in, "llr_out": np.ascontiguousarray(r["llr_out"]),
                   "failed": r["weight"] > 0}
            for v in out.values():
                v.setflags(write=False)
            self.decoded[name] = out
        return self.decoded[name]

    def want(self, name, which):
        """{(candidates, pair_depth): the mirror's outputs} on frames(name)[which] toward frames(name)["s"]."""
        f = self.frames(name)
        return self.of(name, which, f[which], f["s"], self.settings(name))

    def of(self, name, key, llr, s, settings):
        if (name, key) not in self.expected:
            r = osr.decode_many(self.codes.mirror(name), llr, s, settings)
            for per in r.values():
                for v in per.values():
                    v.setflags(write=False)
            self.expected[(name, key)] = r
        return self.expected[(name, key)]

    def random_syndromes(self, name):
        """(s, the mirror's outputs at (64, 8)): random bits, on h.txt mostly outside the column space."""
        code = self.codes.mirror(name)
        s = np.random.default_rng(17).integers(0, 2, (frames_of(name), code.mc), dtype=np.uint8)
        return s, self.of(name, "random", self.frames(name)["llr_in"], s, ((64, 8),))[(64, 8)]


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return peel.Codes(tmp_path_factory.mktemp("osd_syndrome"))


@pytest.fixture(scope="module")
def inputs(codes):
    return Inputs(codes)


def _same(got, want):
    return all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)


def _differing(got, want):
    return {k: np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1)).tolist() for k in want if not np.array_equal(got[k], want[k])}


def _nonzero(llr):
    """The LLRs with 0.5 wherever they are zero (the sign-flip identity needs a sign everywhere)."""
    return np.where(llr == 0, 0.5, llr)


# ---- 1. decoded frames against the mirror ----
def test_the_inputs_show_every_class(codes, inputs):
    """Before any kernel runs: the frames hold what the tests below are about, by the mirrors alone."""
    seen, pairs = set(), 0
    for name in NAMES:
        f = inputs.frames(name)
        assert 0 < f["failed"].sum() < frames_of(name), (name, int(f["failed"].sum()))
        assert f["s"].any(1).all() and not np.array_equal(f["llr_in"], f["llr_out"])
        for which in ("llr_out", "llr_in"):
            out = inputs.want(name, which)
            for key, r in out.items():
                if which == "llr_out":
                    assert np.array_equal(r["status"] != osr.CODEWORD, f["failed"]), (name, key)  # the decoder's decision rule
                assert not (r["status"] == osr.INFEASIBLE).any()  # s = H x
                seen |= set(r["status"].tolist())
                pairs += int((r["status"] == osr.REPROCESSED_PAIR).sum())
            assert set(out[(0, 0)]["status"].tolist()) <= {osr.CODEWORD, osr.ORDER0}
            assert osr.REPROCESSED_PAIR not in out[(64, 0)]["status"] and osr.REPROCESSED not in out[(0, 2)]["status"]
    assert seen == {osr.CODEWORD, osr.ORDER0, osr.REPROCESSED, osr.REPROCESSED_PAIR} and pairs > 0
    assert (inputs.want("golden", "llr_in")[(64, 8)]["status"] == osr.REPROCESSED_PAIR).any()  # a pair wins at the LDS edge
    _, r = inputs.random_syndromes("golden")
    assert 0 < (r["status"] == osr.INFEASIBLE).sum() < frames_of("golden")  # rank 1021 of 1024: 7 of 8 random syndromes
    golden = codes.mirror("golden")
    assert golden.nc % 64 == 0 and len(osd.reduce(osd.matrix(golden), np.arange(golden.nc))[0]) == 1021 < golden.mc
    assert codes.mirror("s40x60").nc % 32 == 4 and (inputs.frames("s129x150t5")["llr_in"] == cr.bsc_delta(POINTS["s129x150t5"])).all(0).sum() >= 5


@pytest.mark.parametrize("name", NAMES)
def test_osd_syndrome_equals_the_mirror(codes, inputs, name):
    code, dec = codes.mirror(name), codes.decoder(name)
    f = inputs.frames(name)
    for which in ("llr_out", "llr_in"):
        for (cap, depth), want in inputs.want(name, which).items():
            got = dec.osd_syndrome_batch(f[which], f["s"], candidates=cap, pair_depth=depth)
            assert _same(got, want), (name, which, cap, depth, _differing(got, want))
            assert not gf2_ref.high_bits(got["word"], code.nc).any()
            left = dec.syndrome_batch(got["word"], want=("syndrome",))["syndrome"] ^ f["s"]  # the library's own syndrome
            assert not left.any(), (name, which, cap, depth)


def test_infeasible_syndromes(codes, inputs):
    for name in ("golden", "s40x60"):
        dec, f = codes.decoder(name), inputs.frames(name)
        s, want = inputs.random_syndromes(name)
        got = dec.osd_syndrome_batch(f["llr_in"], s, candidates=64, pair_depth=8)
        assert _same(got, want), (name, _differing(got, want))
        bad = got["status"] == osr.INFEASIBLE
        assert np.array_equal(got["word"][bad], gf2_ref.pack(osd.values(f["llr_in"])[0])[bad])  # the decisions come back
        left = dec.syndrome_batch(got["word"], want=("syndrome",))["syndrome"] ^ s
        assert not left[~bad].any() and left[bad].any(1).all(), name
    assert bad.sum() == 0  # (s40x60 has full rank: every syndrome is met)


# ---- 2. the identities with ldpc_hip_osd_batch, kernel against kernel ----
@pytest.mark.parametrize("name", NAMES)
def test_without_a_syndrome_and_pairs_it_is_osd_batch(codes, inputs, name):
    dec, f = codes.decoder(name), inputs.frames(name)
    for which in ("llr_out", "llr_in"):
        for cap in (0, 1, 64, codes.mirror(name).nc):
            a, b = dec.osd_syndrome_batch(f[which], None, candidates=cap), dec.osd_batch(f[which], candidates=cap)
            for key in ("word", "flips", "metric", "status"):
                assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (name, which, cap, key)
            assert np.array_equal(a["flipped_columns"][:, 0], b["flipped_column"]) and (a["flipped_columns"][:, 1] == osr.NO_COLUMN).all()
    assert (b["status"] != osd.CODEWORD).any()


@pytest.mark.parametrize("name", NAMES)
def test_the_sign_flip_identity(codes, inputs, name):
    """s = M u: the call is ldpc_hip_osd_batch on the LLRs with the sign flipped wherever u is 1, and u added to its word."""
    dec, f = codes.decoder(name), inputs.frames(name)
    u = f["x"]
    for which in ("llr_out", "llr_in"):
        llr = _nonzero(f[which])
        for cap in (0, 64):
            a = dec.osd_syndrome_batch(llr, f["s"], candidates=cap)
            b = dec.osd_batch(llr * (1.0 - 2.0 * u), candidates=cap)
            assert np.array_equal(a["word"], b["word"] ^ gf2_ref.pack(u)), (name, which, cap)
            for key in ("flips", "metric", "status"):
                assert np.array_equal(a[key], b[key]), (name, which, cap, key)
            assert np.array_equal(a["flipped_columns"][:, 0], b["flipped_column"])
    assert (a["status"] == osr.REPROCESSED).any()


# ---- 3. ties and special values, element types ----
@pytest.mark.parametrize("name", ("s40x60", "r240", "s129x150t5"))
def test_ties_and_special_values(codes, inputs, name):
    code, dec = codes.mirror(name), codes.decoder(name)
    f = inputs.frames(name)
    x = plain._special_frames(code, f["llr_out"])
    s = f["s"][:x.shape[0]]
    settings = ((0, 0), (7, 3), (code.nc, 8), (64, 256))
    want = inputs.of(name, "special", x, s, settings)
    assert s.any(1).all() and np.isnan(x).any() and np.isinf(x).any() and np.unique(osd.values(x)[1][3]).size < 8
    assert (want[(64, 256)]["status"] == osr.REPROCESSED_PAIR).any()
    for cap, depth in settings:
        got = dec.osd_syndrome_batch(x, s, candidates=cap, pair_depth=depth)
        assert _same(got, want[(cap, depth)]), (name, cap, depth, _differing(got, want[(cap, depth)]))
    # int8: the integer itself, no step
    k = np.clip(np.round(x[:20]), -128, 127)
    k = np.where(np.isnan(k), 0, k).astype(np.int8)
    k[3, :4] = (-128, 127, -127, 0)
    want8 = inputs.of(name, "int8", k, s[:20], settings)
    for cap, depth in settings:
        got = dec.osd_syndrome_batch(k, s[:20], candidates=cap, pair_depth=depth)
        assert _same(got, want8[(cap, depth)]), (name, "int8", cap, depth, _differing(got, want8[(cap, depth)]))
    # float32 and float16: the call on the typed values is the call on the same values widened
    with np.errstate(over="ignore"):
        for dt in (np.float32, np.float16):
            typed = x.astype(np.float32).astype(dt)
            typed[28] = np.asarray(6e-8, dt)  # (a subnormal binary16: positive, reliability 0)
            wide = typed.astype(np.float64)
            for cap, depth in ((0, 0), (code.nc, 8)):
                got, ref = dec.osd_syndrome_batch(typed, s, candidates=cap, pair_depth=depth), dec.osd_syndrome_batch(wide, s, candidates=cap, pair_depth=depth)
                assert _same(got, ref), (name, dt, cap, depth)
                assert _same(got, osr.decode(code, typed, s, cap, depth)), (name, dt, cap, depth, "mirror")


# ---- 4. syndrome formats ----
@pytest.mark.parametrize("name", ("golden", "s40x60", "s129x150t5"))
def test_syndrome_formats(codes, inputs, name):
    """Packed words as ldpc_hip_syndrome_batch writes them, with random bits from mc on; bytes other than 0 and 1."""
    code, dec = codes.mirror(name), codes.decoder(name)
    f = inputs.frames(name)
    want = inputs.want(name, "llr_in")[(64, 8)]
    packed = dec.syndrome_batch(gf2_ref.pack(f["x"]), want=("syndrome_bits",))["syndrome_bits"]
    assert np.array_equal(packed, gf2_ref.pack(f["s"]))
    garbage = peel._garbage(packed, code.mc, np.random.default_rng(3))
    assert (code.mc % 32 == 0) or not np.array_equal(garbage, packed)
    for s in (packed, garbage, f["s"] * np.uint8(7), f["s"] * np.uint8(255)):
        got = dec.osd_syndrome_batch(f["llr_in"], s, candidates=64, pair_depth=8)
        assert _same(got, want), (name, s.dtype, _differing(got, want))


# ---- 5. call shapes ----
@pytest.mark.parametrize("name", ("golden", "s40x60"))
def test_rows_of_a_call_are_the_call_on_the_rows(codes, inputs, name):
    dec, n = codes.decoder(name), frames_of(name)
    f = inputs.frames(name)
    want = inputs.want(name, "llr_in")[(64, 8)]
    for a, b in ((0, 1), (5, 17), (n - 1, n)):
        got = dec.osd_syndrome_batch(f["llr_in"][a:b], f["s"][a:b], candidates=64, pair_depth=8)
        assert _same(got, {k: want[k][a:b] for k in KEYS}), (name, a, b)
    half = [dec.osd_syndrome_batch(f["llr_in"][a:b], f["s"][a:b], candidates=64, pair_depth=8) for a, b in ((0, n // 2), (n // 2, n))]
    assert _same({k: np.concatenate((half[0][k], half[1][k])) for k in KEYS}, want)  # a call split in two
    empty = dec.osd_syndrome_batch(f["llr_in"][:0], f["s"][:0], candidates=64, pair_depth=8)
    assert set(empty) == set(KEYS) and empty["word"].shape == (0, want["word"].shape[1]) and empty["flipped_columns"].shape == (0, 2)
    if name == "s40x60":  # every subset of the outputs: the others are NULL
        for count in range(len(KEYS) + 1):
            for keys in itertools.combinations(KEYS, count):
                got = dec.osd_syndrome_batch(f["llr_in"], f["s"], candidates=64, pair_depth=8, want=keys)
                assert set(got) == set(keys) and _same(got, {k: want[k] for k in keys}), keys


def test_device_tensors_and_prefilled_buffers(codes, inputs):
    import torch
    dev = torch.device("cuda", 0)
    name = "s129x150t5"
    code, dec, n = codes.mirror(name), codes.decoder(name), frames_of(name)
    words = (code.nc + 31) // 32
    f = inputs.frames(name)
    want = inputs.want(name, "llr_out")[(64, 256)]
    side = torch.cuda.Stream(device=dev)

    def filled(*shape):
        return torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device=dev).view(torch.uint32)

    out = {k: np.full(want[k].shape, 0x7F, want[k].dtype) for k in KEYS}  # host buffers end fully overwritten
    got = dec.osd_syndrome_batch(f["llr_out"], f["s"], candidates=64, pair_depth=256, want=(), out=out)
    assert got["word"] is out["word"] and _same(out, want)
    packed = gf2_ref.pack(f["s"])
    for stream, tdt, syndrome in ((None, torch.float64, f["s"]), (side.cuda_stream, torch.float32, packed)):
        t = torch.from_numpy(f["llr_out"].copy()).to(dev).to(tdt)
        s = torch.from_numpy(syndrome.view(np.int32) if syndrome.dtype == np.uint32 else syndrome.copy()).to(dev)
        s = s.view(torch.uint32) if syndrome.dtype == np.uint32 else s
        ref = want if tdt == torch.float64 else osr.decode(code, t.cpu().numpy(), f["s"], 64, 256)
        out = {"word": filled(n, words), "flips": filled(n), "flipped_columns": filled(n, 2), "status": filled(n),
               "metric": torch.full((n,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device=dev).view(torch.uint64)}
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream; the call runs on `stream`)
        dec.osd_syndrome_batch(t, s, candidates=64, pair_depth=256, want=(), out=out, stream=stream)
        dec.synchronize(stream)
        host = {k: (v.view(torch.int64).cpu().numpy().view(np.uint64) if k == "metric" else v.view(torch.int32).cpu().numpy().view(np.uint32))
                for k, v in out.items()}
        assert _same(host, ref), (str(tdt), _differing(host, ref))
        mixed = dec.osd_syndrome_batch(t, syndrome, candidates=64, pair_depth=256)  # device LLRs, a host syndrome, host outputs
        assert _same(mixed, ref), (str(tdt), "mixed")


# ---- 6. refusals and the LDS formula where the GPU is ----
def test_refusals_and_lds_bytes(codes, inputs):
    import libldpc_amd
    lib = libldpc_amd.load_library()
    for name in NAMES:
        dec = codes.decoder(name)
        assert dec.osd_syndrome_lds_bytes() == formula(codes.mirror(name)) > 0, name
    assert codes.decoder("golden").osd_syndrome_lds_bytes() == 159920
    name = "s40x60"
    dec, f = codes.decoder(name), inputs.frames(name)
    want = inputs.want(name, "llr_in")[(64, 8)]
    llr, s = f["llr_in"], f["s"]
    out = {k: np.full(want[k].shape, 0x5A, want[k].dtype) for k in KEYS}

    def run(depth=8, kind=0, src=llr.ctypes.data, fmt=0):
        return lib.ldpc_hip_osd_syndrome_batch(dec.ctx, 64, depth, len(llr), src, kind, s.ctypes.data, fmt, out["word"].ctypes.data,
                                               out["flips"].ctypes.data, out["metric"].ctypes.data, out["flipped_columns"].ctypes.data,
                                               out["status"].ctypes.data, None)

    for kw, text in (({"depth": 257}, b"pair_depth"), ({"kind": 4}, b"LLR type"), ({"fmt": 2}, b"format"), ({"fmt": -1}, b"format"), ({"src": None}, b"null llr")):
        assert run(**kw) == -1 and b"ldpc_hip_osd_syndrome_batch" in lib.ldpc_hip_last_error() and text in lib.ldpc_hip_last_error(), kw
    assert all((v == 0x5A).all() for v in out.values())  # nothing was written
    assert run() == 0 and _same(out, want)
    with pytest.raises(RuntimeError, match="pair_depth"):
        dec.osd_syndrome_batch(llr, s, pair_depth=257)
    assert _same(dec.osd_syndrome_batch(llr, s, candidates=64, pair_depth=256), inputs.want(name, "llr_in")[(64, 256)])  # the cap itself
