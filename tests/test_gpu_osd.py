"""ldpc_hip_osd_batch (include/ldpc_amd.h; libldpc_amd/csrc/kernels_osd.hip) on the GPU: all five outputs against the numpy
mirror of tests/osd_ref.py bit for bit — on the soft output and on the channel LLRs of frames that a min-sum mirror decoded,
some to the end and some not —, ties and special values, element types, splits and buffer kinds, the chain encode -> channel
-> min-sum -> OSD -> syndrome on device tensors, and between the batches of a running stream.

The codes and the Codes fixture are those of test_gpu_erasure_batch.py: tests/golden/h.txt (rank 1021 of 1024 check nodes, the
largest rows, 158 768 bytes of LDS: the edge), s40x60 (a last word of 4 bits), s129x150t5 (shortened columns at 99999.9),
s40x60_hdup (parallel edges), s800x100 and a (3,6)-regular code of 240 columns.  70 frames per code, 24 for h.txt, where the
mirror takes a tenth of a second per frame.  Frames are channel_ref's (counter noise of seed 31) at a point per code where,
by the min-sum mirror, some of them end with a non-zero syndrome and some do not (asserted below)."""
import itertools

import numpy as np
import pytest

import channel_ref as cr
import gf2_ref
import orc
import osd_ref as osd
import test_gpu_erasure_batch as peel
from minsum_ref import MinSumMirror

pytestmark = pytest.mark.gpu
NAMES = ("golden", "s40x60", "s129x150t5", "s40x60_hdup", "s800x100", "r240")
SEED = 31
POINTS = {"golden": -4.2, "s40x60": -4.0, "s129x150t5": 1.0, "s40x60_hdup": 1.0, "s800x100": 5.0, "r240": 2.0}  # Es / sigma^2, dB
KEYS = osd.KEYS


def frames_of(name):
    return 24 if name == "golden" else 70


class Inputs:
    """The frames and what the mirror makes of them, computed once and never changed."""

    def __init__(self, codes):
        self.codes, self.decoded, self.expected = codes, {}, {}

    def candidates(self, name):
        return (0, 1, 64, self.codes.mirror(name).nc)

    def frames(self, name):
        """dict(cw, llr_in, llr_out, failed): N codewords (the all-zero one where the code has no generator) through
        channel_ref's AWGN channel and 50 iterations of the min-sum mirror with early termination."""
        if name not in self.decoded:
            code, n = self.codes.mirror(name), frames_of(name)
            h, g = self.codes.files[name]
            cw = code.encode(np.random.default_rng(7).integers(0, 2, (n, code.kc), dtype=np.uint8)) if code.has_g else None
            received, _ = cr.awgn_received(code, 1, POINTS[name], SEED, np.arange(n), cw)
            llr_in = cr.awgn_llr(code, 1, POINTS[name], received)
            r = MinSumMirror(orc.Code(h, g) if g else orc.Code(h)).decode(llr_in, early_term=True, iterations=50, codeword=cw)
            out = {"cw": np.zeros((n, code.nc), np.uint8) if cw is None else cw, "llr_in": llr_in, "llr_out": np.ascontiguousarray(r["llr_out"]),
                   "failed": code.syndrome(r["hard"])[1] > 0}
            for v in out.values():
                v.setflags(write=False)
            self.decoded[name] = out
        return self.decoded[name]

    def want(self, name, which):
        """{candidates: the mirror's outputs} on frames(name)[which]."""
        return self.of(name, which, self.frames(name)[which], self.candidates(name))

    def of(self, name, key, llr, candidates):
        if (name, key) not in self.expected:
            r = osd.decode_many(self.codes.mirror(name), llr, candidates)
            for per in r.values():
                for v in per.values():
                    v.setflags(write=False)
            self.expected[(name, key)] = r
        return self.expected[(name, key)]


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return peel.Codes(tmp_path_factory.mktemp("osd"))


@pytest.fixture(scope="module")
def inputs(codes):
    return Inputs(codes)


def _same(got, want):
    return all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)


def _differing(got, want):
    return {k: np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1)).tolist() for k in want if not np.array_equal(got[k], want[k])}


# ---- 1. the soft output and the channel LLRs of decoded frames ----
def test_the_inputs_show_every_class(codes, inputs):
    """Before any kernel runs: the frames hold what the tests below are about."""
    seen = set()
    for name in NAMES:
        f = inputs.frames(name)
        assert 0 < f["failed"].sum() < frames_of(name), (name, int(f["failed"].sum()))
        out = inputs.want(name, "llr_out")
        for cap, r in out.items():
            assert np.array_equal(r["status"] != osd.CODEWORD, f["failed"]), (name, cap)  # the decoders' decision rule
            seen |= set(r["status"].tolist())
        assert not out[0]["status"].tolist().count(osd.REPROCESSED)
    assert seen == {osd.CODEWORD, osd.ORDER0, osd.REPROCESSED}
    golden = codes.mirror("golden")
    assert len(osd.reduce(osd.matrix(golden), np.arange(golden.nc))[0]) == 1021 < golden.mc  # dependent check nodes
    assert (inputs.want("golden", "llr_in")[golden.nc]["status"] == osd.REPROCESSED).any()
    assert codes.mirror("s40x60").nc % 32 == 4 and (inputs.frames("s129x150t5")["llr_in"] == cr.SHORTEN_AWGN).sum(1).min() == 5


@pytest.mark.parametrize("name", NAMES)
def test_osd_equals_the_mirror(codes, inputs, name):
    dec = codes.decoder(name)
    for which in ("llr_out", "llr_in"):
        llr = inputs.frames(name)[which]
        for cap, want in inputs.want(name, which).items():
            got = dec.osd_batch(llr, candidates=cap)
            assert _same(got, want), (name, which, cap, _differing(got, want))
            assert not gf2_ref.high_bits(got["word"], codes.mirror(name).nc).any()
            assert not codes.mirror(name).syndrome(gf2_ref.unpack(got["word"], codes.mirror(name).nc))[1].any()


# ---- 2. ties and special values ----
def _special_frames(code, base):
    """float64 [n][nc] on a coarse grid: few distinct magnitudes, so that the order by column index decides; an all-zero row,
    rows of +0.0 and -0.0 only, rows with NaN, +-infinity and -0.0 among ordinary values, values at and beyond the clamp of q,
    and below 1 / 4096."""
    rng = np.random.default_rng(12)
    n, nc = 40, code.nc
    x = rng.integers(-3, 4, (n, nc)).astype(np.float64)  # 0, 1, 2, 3 and signs
    x[0] = 0.0
    x[1] = -0.0
    x[2] = np.where(rng.random(nc) < 0.5, 0.0, -0.0)
    for f in range(3, 12):
        at = rng.choice(nc, 9, replace=False)
        x[f, at] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 524287.5, -524288.0, 1e300, -np.nan]
    x[12:20] = np.round(base[:8] * 2) / 2  # decoded frames on a half-integer grid
    x[20:24] = base[:4] * 2.0**-14  # most reliabilities 0 or 1
    x[24:28] = rng.choice([2.0**-13, -(2.0**-12), 2.0**-12 - 2.0**-30, 1.0], (4, nc))
    return x


@pytest.mark.parametrize("name", ("s40x60", "r240", "s129x150t5"))
def test_ties_and_special_values(codes, inputs, name):
    code, dec = codes.mirror(name), codes.decoder(name)
    x = _special_frames(code, inputs.frames(name)["llr_out"])
    caps = (0, 7, code.nc)
    want = inputs.of(name, "special", x, caps)
    z, q = osd.values(x)
    assert (np.unique(q[3]).size < 8) and np.isnan(x).any() and np.isinf(x).any() and np.signbit(x[1]).all()
    for cap in caps:
        got = dec.osd_batch(x, candidates=cap)
        assert _same(got, want[cap]), (name, cap, _differing(got, want[cap]))
    assert want[0]["status"][0] in (osd.ORDER0, osd.CODEWORD) and not want[code.nc]["metric"][:3].any()  # q = 0 everywhere
    # int8: the integer itself, no step
    k = np.clip(np.round(x[:20]), -128, 127)
    k = np.where(np.isnan(k), 0, k).astype(np.int8)
    k[3, :4] = (-128, 127, -127, 0)
    want8 = inputs.of(name, "int8", k, caps)
    for cap in caps:
        got = dec.osd_batch(k, candidates=cap)
        assert _same(got, want8[cap]), (name, "int8", cap, _differing(got, want8[cap]))
    # float32 and float16: the call on the typed values is the call on the same values widened
    with np.errstate(over="ignore"):
        for dt in (np.float32, np.float16):
            typed = x.astype(np.float32).astype(dt)
            typed[28] = np.asarray(6e-8, dt)  # (a subnormal binary16: positive, reliability 0)
            wide = typed.astype(np.float64)
            for cap in (0, code.nc):
                got, ref = dec.osd_batch(typed, candidates=cap), dec.osd_batch(wide, candidates=cap)
                assert _same(got, ref), (name, dt, cap)
                assert _same(got, osd.decode(code, typed, cap)), (name, dt, cap, "mirror")


# ---- 3. call shapes ----
@pytest.mark.parametrize("name", ("golden", "s40x60"))
def test_rows_of_a_call_are_the_call_on_the_rows(codes, inputs, name):
    dec, n = codes.decoder(name), frames_of(name)
    llr = inputs.frames(name)["llr_in"]
    want = inputs.want(name, "llr_in")[64]
    for a, b in ((0, 1), (5, 17), (n - 1, n)):
        got = dec.osd_batch(llr[a:b], candidates=64)
        assert _same(got, {k: want[k][a:b] for k in KEYS}), (name, a, b)
    empty = dec.osd_batch(llr[:0], candidates=64)
    assert set(empty) == set(KEYS) and empty["word"].shape == (0, want["word"].shape[1]) and empty["metric"].shape == (0,)
    if name == "s40x60":  # every subset of the outputs
        for count in range(len(KEYS) + 1):
            for keys in itertools.combinations(KEYS, count):
                got = dec.osd_batch(llr, candidates=64, want=keys)
                assert set(got) == set(keys) and _same(got, {k: want[k] for k in keys}), keys


def test_device_tensors_and_prefilled_buffers(codes, inputs):
    import torch
    dev = torch.device("cuda", 0)
    name = "s129x150t5"
    code, dec, n = codes.mirror(name), codes.decoder(name), frames_of(name)
    words = (code.nc + 31) // 32
    llr = inputs.frames(name)["llr_out"]
    want = inputs.want(name, "llr_out")[64]
    side = torch.cuda.Stream(device=dev)

    def filled(*shape):
        return torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device=dev).view(torch.uint32)

    out = {k: np.full(want[k].shape, 0x7F, want[k].dtype) for k in KEYS}  # host buffers end fully overwritten
    got = dec.osd_batch(llr, candidates=64, want=(), out=out)
    assert got["word"] is out["word"] and _same(out, want)
    for stream, tdt in ((None, torch.float64), (side.cuda_stream, torch.float32)):
        t = torch.from_numpy(llr.copy()).to(dev).to(tdt)
        ref = want if tdt == torch.float64 else osd.decode(code, t.cpu().numpy(), 64)
        out = {"word": filled(n, words), "flips": filled(n), "flipped_column": filled(n), "status": filled(n),
               "metric": torch.full((n,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device=dev).view(torch.uint64)}
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream; the call runs on `stream`)
        dec.osd_batch(t, candidates=64, want=(), out=out, stream=stream)
        dec.synchronize(stream)
        host = {k: (v.view(torch.int64).cpu().numpy().view(np.uint64) if k == "metric" else v.view(torch.int32).cpu().numpy().view(np.uint32))
                for k, v in out.items()}
        assert _same(host, ref), (str(tdt), _differing(host, ref))


# ---- 4. the chain on device tensors ----
@pytest.mark.parametrize("name,x,n", (("r240", 3.0, 2000), ("golden", -3.6, 200), ("s129x150t5", 1.0, 300)))
def test_the_chain_on_device_tensors(codes, name, x, n):
    """BP + OSD without leaving the device.  On the regular code of 240 columns at 3.0 dB, 2 000 frames of seed 16: the two
    mirrors alone (channel_ref, minsum_ref, osd_ref) give 56 frames that min-sum leaves, 1 944 frames equal to the transmitted
    codeword before OSD and 1 977 after it with 64 candidates — strictly more is asserted there, no fewer on the other codes."""
    import torch
    dev = torch.device("cuda", 0)
    code, dec = codes.mirror(name), codes.decoder(name)
    words = (code.nc + 31) // 32

    def u32(*shape):
        return torch.full(shape, -1, dtype=torch.int32, device=dev).view(torch.uint32)

    cw = torch.zeros((n, words), dtype=torch.int32, device=dev).view(torch.uint32)
    if code.has_g:
        info = torch.from_numpy(np.random.default_rng(8).integers(0, 2, (n, code.kc), dtype=np.uint8)).to(dev)
        dec.encode_batch(info, want=(), out={"codeword_bits": cw})
    llr = torch.full((n, code.nc), 99.0, dtype=torch.float64, device=dev)
    dec.channel_batch(cw, "AWGN", x, seed=16, want=(), out={"llr": llr})
    out = {"iters": torch.zeros(n, dtype=torch.int32, device=dev), "llr_out": torch.zeros((n, code.nc), dtype=torch.float64, device=dev),
           "hard_bits": u32(n, words)}
    dec.decode_batch_typed(llr, early_term=True, iterations=50, decoding="BP_MS", want=(), out=out)
    word, flips, column, status, left, weight, err_before, err_after = u32(n, words), u32(n), u32(n), u32(n), u32(n), u32(n), u32(n), u32(n)
    metric = torch.full((n,), -1, dtype=torch.int64, device=dev).view(torch.uint64)
    dec.syndrome_batch(out["hard_bits"], want=(), out={"weight": left})
    dec.osd_batch(out["llr_out"], candidates=64, want=(),
                  out={"word": word, "flips": flips, "metric": metric, "flipped_column": column, "status": status})
    dec.syndrome_batch(word, want=(), out={"weight": weight})
    dec.bit_errors_batch(out["hard_bits"], cw, out=err_before)
    dec.bit_errors_batch(word, cw, out=err_after)
    torch.cuda.synchronize()
    host = {k: v.view(torch.int32).cpu().numpy().view(np.uint32) for k, v in
            dict(cw=cw, hard=out["hard_bits"], word=word, flips=flips, column=column, status=status, left=left, weight=weight,
                 err_before=err_before, err_after=err_after).items()}
    host["metric"] = metric.view(torch.int64).cpu().numpy().view(np.uint64)
    assert not host["weight"].any()  # a codeword, every frame
    done = host["left"] == 0
    assert 0 < done.sum() < n
    assert np.array_equal(host["status"] == osd.CODEWORD, done)
    assert np.array_equal(host["word"][done], host["hard"][done]) and not host["flips"][done].any() and not host["metric"][done].any()
    assert (host["column"][done] == osd.NO_COLUMN).all() and (host["flips"][~done] > 0).all()
    before, after = (host["hard"] == host["cw"]).all(1), (host["word"] == host["cw"]).all(1)
    assert (after | ~before).all() and not host["err_after"][after].any()
    print(f"chain {name} at {x} dB: {n} frames, {int((~done).sum())} left by min-sum, equal to the transmitted codeword "
          f"{int(before.sum())} before OSD, {int(after.sum())} after")
    if name == "r240":
        assert after.sum() > before.sum()
    else:
        assert after.sum() >= before.sum()
    left = np.flatnonzero(~done)[:40]  # what min-sum left, against the mirror
    want = osd.decode(code, out["llr_out"].cpu().numpy()[left], 64)
    got = {"word": host["word"][left], "flips": host["flips"][left], "metric": host["metric"][left],
           "flipped_column": host["column"][left], "status": host["status"][left]}
    assert _same(got, want), _differing(got, want)


# ---- 5. no state ----
def test_the_stream_interface_is_left_alone(codes, inputs):
    import libldpc_amd
    llr = inputs.frames("golden")["llr_out"]
    want = inputs.want("golden", "llr_out")[64]
    runs = []
    for between in (False, True):
        dec = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
        dec.set_noise("counter")
        dec.stream_begin("AWGN", 9, -3.0)
        got = []
        for batch in (40, 33):
            if between:
                assert _same(dec.osd_batch(llr, candidates=64), want)
            got.append(dec.stream_decode(batch, iterations=10, decoding="BP_MS", want=("iters", "bit_errors", "llr_in", "llr_out", "codeword")))
        assert dec.stream_frame == 73
        runs.append(got)
    for plain, mixed in zip(*runs):
        for k in ("iters", "bit_errors", "llr_in", "llr_out", "codeword"):
            assert plain[k].dtype == mixed[k].dtype and np.array_equal(plain[k], mixed[k]), k
    assert all(r["codeword"].any() for r in runs[0])
