"""ldpc_hip_bit_flip_batch (include/ldpc_amd.h; libldpc_amd/csrc/kernels_bit_flip.hip) on the GPU: all three outputs against
the numpy mirror of tests/bit_flip_ref.py bit for bit under the deterministic, the probabilistic, the margin and the soft
setting, over the round limits, element types, syndrome formats, call shapes and buffer kinds, the draws against the
generator's raw words, the context's settings and a running stream, and the chain syndrome -> bit flipping -> syndrome on
device tensors.

Inputs: random words x (not codewords) of numpy.random.default_rng(5), s = H x, the LLRs of x through the BSC mirror (the
hard settings: +-|llr|, the step) or the AWGN mirror (the soft setting) under Philox seed 9, at a point per code and setting
where — by the mirror, asserted before any kernel runs — some frames reach s and some do not (bit_flip_ref.POINTS,
PROB_POINTS, SOFT_POINTS); 128 frames and 100 rounds."""
import itertools

import numpy as np
import pytest

import bit_flip_ref as bf
import channel_ref as cr
import gf2_ref
import orc
import philox_ref

pytestmark = pytest.mark.gpu
KEYS = bf.KEYS
DET, PROB, MARGIN = bf.HARD_SETTINGS


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return bf.Codes(tmp_path_factory.mktemp("bf"))


def _same(got, want):
    return all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)


def _differing(got, want):
    return {k: np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1)).tolist()[:8] for k in want if not np.array_equal(got[k], want[k])}


def _call(dec, llr, syn, setting, step, iterations=bf.ROUNDS, first_frame=0, **kw):
    w, margin, prob, q_bits = setting[:4]
    return dec.bit_flip_batch(llr, syn, iterations=iterations, q_bits=q_bits, step=step, check_weight=w, margin=margin, flip_prob=prob,
                              seed=bf.SEED, first_frame=first_frame, **kw)


def _expect(codes, name, llr, syn, setting, step, iterations=bf.ROUNDS, first_frame=0):
    w, margin, prob, q_bits = setting[:4]
    return codes.mirror(name).expected(llr, syn, iterations, q_bits, step, w, margin, bf.threshold_of(prob), bf.SEED, first_frame)


def _cases(codes, name):
    """(label, setting, frames, step) of the four settings of the contract's test plan."""
    hard, prob, soft = codes.hard_frames(name), codes.hard_frames(name, eps=bf.PROB_POINTS[name]), codes.soft_frames(name)
    return (("deterministic", DET, hard, hard["step"]), ("probabilistic", PROB, prob, prob["step"]), ("margin", MARGIN, hard, hard["step"]),
            ("soft", bf.SOFT_SETTING, soft, bf.SOFT_SETTING[4]))


# ---- 1. against the mirror ----
@pytest.mark.parametrize("name", bf.NAMES)
def test_bit_flip_equals_the_mirror(codes, name):
    dec, code = codes.decoder(name), codes.gf2(name)
    for label, setting, f, step in _cases(codes, name):
        llr, s = f["llr"], f["s"]
        base = _expect(codes, name, llr, s, setting, step)
        reached = base["weight"] == 0
        degenerate = name == "golden" and setting[1] == 0 and setting[2] == 1.0  # the punctured columns tie: no frame reaches s
        assert (not reached.any()) if degenerate else 0 < reached.sum() < bf.N, (name, label)  # before any kernel runs
        if label == "deterministic" and not degenerate:
            assert int(reached.sum()) == bf.POINTS[name][2]
        if label == "margin" and bf.POINTS[name][1] == 1:
            assert int(reached.sum()) == bf.POINTS[name][2]
        assert (base["iters"][~reached] == bf.ROUNDS).all()
        packed = gf2_ref.pack(s)
        got = _call(dec, llr, packed, setting, step)
        assert _same(got, base), (name, label, _differing(got, base))
        assert not gf2_ref.high_bits(got["hard_bits"], code.nc).any()
        word = gf2_ref.unpack(got["hard_bits"], code.nc)
        assert np.array_equal(got["weight"], (code.syndrome(word)[0] != s).sum(1))  # 0 iff the word has syndrome s
        assert _same(_call(dec, llr, np.ascontiguousarray(s), setting, step), base), (name, label, "bytes")
        if code.mc % 32:  # the bits of the last syndrome word from mc on are ignored
            dirty = packed.copy()
            dirty[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(code.mc % 32)
            assert _same(_call(dec, llr, dirty, setting, step), base), (name, label, "high bits")
        m = 67  # the variants on the first frames: a partial group whatever the frames of a workgroup
        a, sa, pa = llr[:m], s[:m], packed[:m]
        for iterations in (0, 1, 7):
            want = _expect(codes, name, a, sa, setting, step, iterations)
            got = _call(dec, a, pa, setting, step, iterations)
            assert _same(got, want), (name, label, iterations, _differing(got, want))
            if iterations == 0:
                assert np.array_equal(gf2_ref.unpack(got["hard_bits"], code.nc), bf.quantize(a, setting[3], step) <= 0) and not got["iters"].any()
        # the element types: the call on the typed values is the mirror on the same values
        for kind in ("float32", "float16", "int8"):
            typed = cr.convert(a, kind, setting[3], step)
            want = _expect(codes, name, typed, sa, setting, step, 20)
            for syn in (pa, np.ascontiguousarray(sa)):
                got = _call(dec, typed, syn, setting, step, 20)
                assert _same(got, want), (name, label, kind, _differing(got, want))
        # no syndrome: toward zero
        want = _expect(codes, name, a, None, setting, step, 10)
        assert _same(_call(dec, a, None, setting, step, 10), want) and _same(_call(dec, a, np.zeros_like(pa), setting, step, 10), want)
        assert (want["weight"] > 0).any()  # (the words are no codewords)


def test_hard_decisions_as_int8(codes):
    """The caller with hard decisions only: int8 +-1 at q_bits = 2, any step; a word that meets s comes back as it went in."""
    name = "sd_mix"
    dec, code = codes.decoder(name), codes.gf2(name)
    f = codes.hard_frames(name)
    want = _expect(codes, name, f["llr"], f["s"], DET, f["step"])
    for step in (1.0, 0.125, f["step"]):
        assert _same(_call(dec, f["k"], gf2_ref.pack(f["s"]), DET, step), want), step
    exact = (1 - 2 * f["x"].astype(np.int64)).astype(np.int8)
    for setting in (DET, PROB, MARGIN):
        got = _call(dec, exact, gf2_ref.pack(f["s"]), setting, 1.0, 65535)
        assert np.array_equal(gf2_ref.unpack(got["hard_bits"], code.nc), f["x"]) and not got["iters"].any() and not got["weight"].any()
    # out-of-range magnitudes clamp, the most negative byte included
    k = np.random.default_rng(4).integers(-128, 128, f["k"].shape).astype(np.int8)
    k[0, :4] = (-128, 127, 0, -1)
    for q_bits, w, margin in ((2, 2, 0), (5, 7, 3), (8, 255, 65535)):
        setting = (w, margin, 1.0, q_bits)
        want = _expect(codes, name, k[:40], f["s"][:40], setting, 1.0, 12)
        got = _call(dec, k[:40], gf2_ref.pack(f["s"][:40]), setting, 1.0, 12)
        assert _same(got, want), (setting, _differing(got, want))


def test_special_values(codes):
    name = "sd_mix"
    dec, code = codes.decoder(name), codes.gf2(name)
    f = codes.soft_frames(name)
    rng = np.random.default_rng(12)
    n, nc = 40, code.nc
    w, margin, prob, q_bits, step = bf.SOFT_SETTING
    qmax = (1 << (q_bits - 1)) - 1
    x = f["llr"][:n].copy()
    x[0], x[1] = 0.0, -0.0
    edge = [s_ * (qmax + h) * step for s_ in (1.0, -1.0) for h in (-0.5, 0.5)] + [s_ * (k + 0.5) * step for s_ in (1.0, -1.0) for k in (0, 1, 2)]
    special = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 99999.9, -99999.9, 1e300, -1e300, 5e-324] + edge
    for r in range(3, 24):
        x[r, rng.choice(nc, len(special), replace=False)] = special
    s = gf2_ref.pack(f["s"][:n])
    want = _expect(codes, name, x, f["s"][:n], bf.SOFT_SETTING, step, 30)
    got = _call(dec, x, s, bf.SOFT_SETTING, step, 30)
    assert _same(got, want), _differing(got, want)
    with np.errstate(over="ignore"):
        for dt in (np.float32, np.float16):
            typed = x.astype(np.float32).astype(dt)
            want = _expect(codes, name, typed, f["s"][:n], bf.SOFT_SETTING, step, 30)
            got = _call(dec, typed, s, bf.SOFT_SETTING, step, 30)
            assert _same(got, want), (dt, _differing(got, want))


# ---- 2. call shapes and buffer kinds ----
@pytest.mark.parametrize("name", ("sd_r36", "s40x60_hdup"))
def test_rows_of_a_call_are_the_call_on_the_rows(codes, name):
    dec = codes.decoder(name)
    f = codes.hard_frames(name, eps=bf.PROB_POINTS[name])
    n = bf.N
    llr, s, step = f["llr"], gf2_ref.pack(f["s"]), f["step"]
    for setting in (DET, PROB):
        want = _expect(codes, name, llr, f["s"], setting, step, 40, 1000)
        # n = 1, 3, 67 and the others: whole and partial groups; a split reproduces the batch once first_frame follows
        for a, b in ((0, 1), (0, 3), (0, 67), (1, n), (n - 1, n), (0, 64), (64, n), (3, 7), (61, 128)):
            got = _call(dec, llr[a:b], s[a:b], setting, step, 40, 1000 + a)
            assert _same(got, {k: want[k][a:b] for k in KEYS}), (name, setting, a, b)
            got = _call(dec, f["k"][a:b], s[a:b], setting, 1.0, 40, 1000 + a)
            assert _same(got, {k: want[k][a:b] for k in KEYS}), (name, setting, a, b, "int8")
        if setting is PROB:  # ... and not without: the draws are the frame's
            assert not _same(_call(dec, llr[64:], s[64:], setting, step, 40, 1000), {k: want[k][64:] for k in KEYS})
        for r in range(1, 4):  # every subset of the outputs
            for keys in itertools.combinations(KEYS, r):
                got = _call(dec, llr, s, setting, step, 40, 1000, want=keys)
                assert set(got) == set(keys) and _same(got, {k: want[k] for k in keys}), keys
        assert _call(dec, llr, s, setting, step, 40, 1000, want=()) == {}
        assert _call(dec, llr[:0], s[:0], setting, step, 40)["iters"].shape == (0,)
        # one row for every frame
        row = llr[5]
        for r in (row, row[None, :], row.astype(np.float32), row.astype(np.float16), f["k"][5]):
            ref = _expect(codes, name, np.repeat(np.asarray(r).reshape(1, -1), n, 0), f["s"], setting, 1.0 if r.dtype == np.int8 else step, 40, 7)
            got = _call(dec, np.ascontiguousarray(r), s, setting, 1.0 if r.dtype == np.int8 else step, 40, 7, shared_llr=True)
            assert _same(got, ref), (name, r.dtype, r.shape, _differing(got, ref))
        assert len(np.unique(ref["hard_bits"], axis=0)) > 1


def test_device_tensors_and_prefilled_buffers(codes):
    import torch
    dev = torch.device("cuda", 0)
    name = "sd_mix"
    f, dec, code = codes.hard_frames(name), codes.decoder(name), codes.gf2(name)
    n, words = bf.N, (code.nc + 31) // 32
    llr, s, step = f["llr"], f["s"], f["step"]
    side = torch.cuda.Stream(device=dev)

    def filled(*shape):
        return torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device=dev).view(torch.uint32)

    for setting in (DET, PROB):
        want = _expect(codes, name, llr, s, setting, step, 30)
        out = {k: np.full(want[k].shape, 0x7F, want[k].dtype) for k in KEYS}
        got = _call(dec, llr, gf2_ref.pack(s), setting, step, 30, want=(), out=out)  # host buffers end fully overwritten
        assert got["hard_bits"] is out["hard_bits"] and _same(out, want)
        for stream, tdt, syn in ((None, torch.float64, gf2_ref.pack(s)), (side.cuda_stream, torch.float32, np.array(s)),
                                 (None, torch.float16, np.array(s)), (side.cuda_stream, torch.int8, gf2_ref.pack(s))):
            host_llr, call_step = (f["k"], 1.0) if tdt == torch.int8 else (llr, step)
            t = torch.from_numpy(np.array(host_llr)).to(dev).to(tdt)
            ts = torch.from_numpy(syn.view(np.int32) if syn.dtype == np.uint32 else syn).to(dev)
            ts = ts.view(torch.uint32) if syn.dtype == np.uint32 else ts
            ref = _expect(codes, name, t.cpu().numpy(), s, setting, call_step, 30)
            out = {"hard_bits": filled(n, words), "iters": filled(n), "weight": filled(n)}
            torch.cuda.synchronize()  # (the buffers were filled on torch's stream; the call runs on `stream`)
            _call(dec, t, ts, setting, call_step, 30, want=(), out=out, stream=stream)
            dec.synchronize(stream)
            host = {k: v.view(torch.int32).cpu().numpy().view(np.uint32) for k, v in out.items()}
            assert _same(host, ref), (str(tdt), _differing(host, ref))
            # device input, host output, and the other way round
            assert _same(_call(dec, t, ts, setting, call_step, 30, stream=stream), ref)
            mixed = {"weight": filled(n)}
            _call(dec, t.cpu().numpy(), syn, setting, call_step, 30, want=(), out=mixed)
            torch.cuda.synchronize()
            assert np.array_equal(mixed["weight"].view(torch.int32).cpu().numpy().view(np.uint32), ref["weight"])
    # a shared row on the device
    row = torch.from_numpy(llr[7].copy()).to(dev)
    ref = _expect(codes, name, np.repeat(llr[7][None, :], n, 0), s, PROB, step, 30)
    assert _same(_call(dec, row, gf2_ref.pack(s), PROB, step, 30, shared_llr=True), ref)


# ---- 3. the draws ----
def test_the_draws_are_the_tag_3_words_of_the_generator(codes):
    dec = codes.decoder("sd_r36")
    per_round = (dec.nc + 3) // 4
    for seed, frame, rnd in ((bf.SEED, 0, 0), (bf.SEED, 1000, 5), (2**64 - 1, 2**40 + 3, 65534)):
        raw = dec.philox(seed, bf.TAG_FLIP, frame, rnd * per_round, per_round)
        assert np.array_equal(raw, philox_ref.blocks(seed, 3, [frame], rnd * per_round + np.arange(per_round))[0])
        assert np.array_equal(raw.reshape(-1)[:dec.nc], bf.draws(seed, [frame], rnd, dec.nc)[0])
    assert not np.array_equal(dec.philox(bf.SEED, 3, 0, 0, 8), dec.philox(bf.SEED, 1, 0, 0, 8))


# ---- 4. no setting and no state ----
def test_the_settings_of_the_context_do_not_matter(codes):
    import libldpc_amd
    name = "sd_r36"
    f = codes.hard_frames(name, eps=bf.PROB_POINTS[name])
    llr, s, step = f["llr"][:96], gf2_ref.pack(f["s"][:96]), f["step"]
    want = {setting: _expect(codes, name, llr, f["s"][:96], setting, step, 40) for setting in (DET, PROB)}
    dec = libldpc_amd.HipDecoder(codes.path(name))
    modes = (("plain", lambda: None, lambda: None),
             ("correction", lambda: dec.set_min_sum_correction(0.5, 0.125), lambda: dec.set_min_sum_correction(1.0, 0.0)),
             ("quantized", lambda: dec.set_min_sum_quantization(4, 1.0), lambda: dec.set_min_sum_quantization(0)),
             ("ternary", lambda: dec.set_min_sum_ternary(2), lambda: dec.set_min_sum_ternary(0)),
             ("layered", lambda: dec.set_min_sum_schedule("layered"), lambda: dec.set_min_sum_schedule("flooding")),
             ("layered fixed", lambda: dec.set_min_sum_layered_fixed(5, 8, 0.5), lambda: dec.set_min_sum_layered_fixed(0)),
             ("counter noise", lambda: dec.set_noise("counter"), lambda: dec.set_noise("reference")))
    for label, on, off in modes:
        on()
        for setting, ref in want.items():
            got = _call(dec, llr, s, setting, step, 40)
            assert _same(got, ref), (label, setting, _differing(got, ref))
        off()
    assert dec.min_sum_quantization[0] == 0 and dec.min_sum_ternary == 0 and dec.min_sum_layered_fixed[0] == 0


def test_the_stream_interface_is_left_alone(codes):
    import libldpc_amd
    f = codes.hard_frames("golden", eps=bf.PROB_POINTS["golden"])
    llr, s = f["llr"][:67], gf2_ref.pack(f["s"][:67])
    want = _expect(codes, "golden", llr, f["s"][:67], PROB, f["step"], 20)
    runs = []
    for between in (False, True):
        dec = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
        dec.set_noise("counter")
        dec.stream_begin("AWGN", 9, -3.0)
        got = []
        for batch in (40, 33):
            if between:
                assert _same(_call(dec, llr, s, PROB, f["step"], 20), want)
            got.append(dec.stream_decode(batch, iterations=10, decoding="BP_MS", want=("iters", "bit_errors", "llr_in", "llr_out", "codeword")))
        assert dec.stream_frame == 73
        runs.append(got)
    for plain, mixed in zip(*runs):
        for k in ("iters", "bit_errors", "llr_in", "llr_out", "codeword"):
            assert plain[k].dtype == mixed[k].dtype and np.array_equal(plain[k], mixed[k]), k
    assert all(r["codeword"].any() for r in runs[0])


# ---- 5. the chain on device tensors ----
def test_the_chain_on_device_tensors(codes):
    """syndrome_batch(x) packed -> bit_flip_batch on int8 +-1 -> syndrome_batch of the returned word, all on device tensors;
    sd_r36 at its operating point.  The outputs are the mirror's; where weight == 0 the returned word's syndrome is s, and
    everywhere the weight is the number of check nodes at which it differs from s."""
    import torch
    dev = torch.device("cuda", 0)
    name = "sd_r36"
    code, dec = codes.gf2(name), codes.decoder(name)
    f = codes.hard_frames(name)
    n = bf.N
    want = _expect(codes, name, f["k"], f["s"], DET, 1.0)
    words, swords = (code.nc + 31) // 32, (code.mc + 31) // 32

    def u32(*shape):
        return torch.full(shape, -1, dtype=torch.int32, device=dev).view(torch.uint32)

    x = torch.from_numpy(f["x"].copy()).to(dev)
    s, s_after = u32(n, swords), u32(n, swords)
    dec.syndrome_batch(x, want=(), out={"syndrome_bits": s})
    out = {"hard_bits": u32(n, words), "iters": u32(n), "weight": u32(n)}
    _call(dec, torch.from_numpy(f["k"].copy()).to(dev), s, DET, 1.0, want=(), out=out)
    dec.syndrome_batch(out["hard_bits"], want=(), out={"syndrome_bits": s_after})
    torch.cuda.synchronize()
    host = {k: v.view(torch.int32).cpu().numpy().view(np.uint32) for k, v in dict(s=s, s_after=s_after, **out).items()}
    assert np.array_equal(host["s"], gf2_ref.pack(f["s"]))
    assert _same({k: host[k] for k in KEYS}, want)
    met = host["weight"] == 0
    assert int(met.sum()) == bf.POINTS[name][2] and np.array_equal(host["s_after"][met], host["s"][met])
    differ = gf2_ref.unpack(host["s_after"] ^ host["s"], code.mc).sum(1)
    assert np.array_equal(differ, host["weight"])
    print(f"chain {name}: {n} frames, {int(met.sum())} reach s")
