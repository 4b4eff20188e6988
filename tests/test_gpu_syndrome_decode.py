"""ldpc_hip_syndrome_decode_batch (include/ldpc_amd.h; libldpc_amd/csrc/kernels_syndrome_decode.hip) on the GPU: all four
outputs against the numpy mirror of tests/syndrome_decode_ref.py bit for bit, against the kernels that exist without it
(quantized min-sum toward zero, and on the augmented code [H | I]), special values, call shapes and buffer kinds, the
context's settings and a running stream, and the reconciliation chain syndrome -> channel -> decode -> check on device tensors.

Inputs: random words x (not codewords) of numpy.random.default_rng(5), s = H x, the LLRs of x through the BSC mirror under
Philox seed 9, at a point per code where — by the mirror, asserted before any kernel runs — some frames reach s and some do
not."""
import numpy as np
import pytest

import channel_ref as cr
import gf2_ref
import orc
import syndrome_decode_ref as sd

pytestmark = pytest.mark.gpu
KEYS = sd.KEYS
BASE = sd.SETTINGS[0]


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return sd.Codes(tmp_path_factory.mktemp("sd"))


def _same(got, want):
    return all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)


def _differing(got, want):
    return {k: np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1)).tolist()[:8] for k in want if not np.array_equal(got[k], want[k])}


def _call(dec, llr, syn, setting=BASE, want=KEYS, **kw):
    q, step, scale, offset = setting
    return dec.syndrome_decode_batch(llr, syn, q_bits=q, step=step, scale=scale, offset=offset, want=want, **kw)


def _expect(codes, name, llr, syn, setting=BASE, early_term=True, iterations=50):
    q, step, scale, offset = setting
    return codes.mirror(name).expected(llr, syn, q, step, scale, offset, early_term, iterations)


# ---- 1. against the mirror ----
@pytest.mark.parametrize("name", sd.NAMES)
def test_syndrome_decode_equals_the_mirror(codes, name):
    f, dec, code = codes.frames(name), codes.decoder(name), codes.gf2(name)
    llr, s = f["llr"], f["s"]
    n = llr.shape[0]
    base = _expect(codes, name, llr, s)
    reached = base["weight"] == 0
    assert 0 < reached.sum() < n, (name, int(reached.sum()))  # both kinds, before any kernel runs
    assert np.array_equal(reached, base["iters"] < 50)
    if name == "golden":  # degree-15 columns whose LLRs are 0
        zero = np.flatnonzero((llr == 0).all(0))
        assert zero.size == 128 and all(code.column_degree(c) == 15 for c in zero[:4])
    packed = gf2_ref.pack(s)
    got = _call(dec, llr, packed)
    assert _same(got, base), (name, _differing(got, base))
    assert not gf2_ref.high_bits(got["hard_bits"], code.nc).any()
    word = gf2_ref.unpack(got["hard_bits"], code.nc)
    assert np.array_equal(got["weight"], (code.syndrome(word)[0] != s).sum(1))  # 0 iff the word has syndrome s
    assert _same(_call(dec, llr, np.ascontiguousarray(s)), base), (name, "bytes")
    # the bits of the last syndrome word from mc on are ignored
    if code.mc % 32:
        dirty = packed.copy()
        dirty[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(code.mc % 32)
        assert _same(_call(dec, llr, dirty), base), (name, "high bits")
    m = 64  # the variants on the first frames
    a, sa, pa = llr[:m], s[:m], packed[:m]
    for early, iterations in ((False, 50), (False, 7), (True, 0), (False, 0), (True, 1), (False, 1)):
        want = _expect(codes, name, a, sa, BASE, early, iterations)
        got = _call(dec, a, pa, early_term=early, iterations=iterations)
        assert _same(got, want), (name, early, iterations, _differing(got, want))
    for setting in sd.SETTINGS[1:]:
        for early in (True, False):
            want = _expect(codes, name, a, sa, setting, early, 50 if early else 6)
            got = _call(dec, a, pa, setting, early_term=early, iterations=50 if early else 6)
            assert _same(got, want), (name, setting, early, _differing(got, want))
    # the element types: the call on the typed values is the mirror on the same values
    for kind, setting in (("float32", BASE), ("float16", BASE), ("int8", BASE), ("int8", sd.SETTINGS[1]), ("float16", sd.SETTINGS[3])):
        typed = cr.convert(a, kind, setting[0], setting[1])
        want = _expect(codes, name, typed, sa, setting)
        for syn in (pa, np.ascontiguousarray(sa)):
            got = _call(dec, typed, syn, setting)
            assert _same(got, want), (name, kind, setting, _differing(got, want))
    # no syndrome: toward zero
    want = _expect(codes, name, a, None)
    assert _same(_call(dec, a, None), want) and _same(_call(dec, a, np.zeros_like(pa)), want)
    assert (want["weight"] > 0).any()  # (the words are no codewords)


# ---- 2. against kernels that exist without it ----
def _toward_zero_inputs(codes, name, n=96):
    """LLRs of random words (never codewords: they run to the end) and of the all-zero codeword (most stop)."""
    f = codes.frames(name)
    return np.concatenate((f["llr"][:n // 3], cr.bsc(codes.gf2(name), sd.POINTS[name][0], sd.NOISE_SEED, np.arange(n - n // 3), None)[1]))


@pytest.mark.parametrize("name", sd.NAMES)
def test_without_a_syndrome_it_is_quantized_min_sum(codes, name):
    import libldpc_amd
    llr = _toward_zero_inputs(codes, name)
    dec, old = codes.decoder(name), libldpc_amd.HipDecoder(codes.path(name))
    stopped = set()
    for setting in sd.SETTINGS:
        q, step, scale, offset = setting
        old.set_min_sum_quantization(q, step)
        old.set_min_sum_correction(scale, offset)
        for kind in ("float64", "float16", "int8"):
            typed = cr.convert(llr, kind, q, step)
            for early, iterations in ((True, 50), (False, 5), (True, 1)):
                ref = old.decode_batch_typed(typed, early_term=early, iterations=iterations, decoding="BP_MS", want=("iters", "llr_out", "hard_bits"))
                got = _call(dec, typed, None, setting, early_term=early, iterations=iterations)
                assert np.array_equal(got["iters"], ref["iters"].astype(np.uint32)), (name, setting, kind, early, iterations)
                assert np.array_equal(got["hard_bits"], ref["hard_bits"]) and np.array_equal(got["llr_out"], ref["llr_out"]), (name, setting, kind)
                stopped |= set((got["iters"] < iterations).tolist())
    assert stopped == {True, False}


@pytest.mark.parametrize("name", ("sd_r36", "sd_mix", "sd_wide", "sd_small"))
def test_with_a_syndrome_it_is_quantized_min_sum_on_the_augmented_code(codes, name):
    """The route this call replaces: [H | I], 99999.9 (1 - 2 s) on the extra columns, decode_batch toward zero.  The messages
    are the same always; the stop is the same where the extra columns cannot tie at a total of 0 (a scale below 1; see
    test_syndrome_decode_host.py), so (1, 0) is compared without early termination."""
    f, dec, code = codes.frames(name), codes.decoder(name), codes.gf2(name)
    aug = codes.decoder(name + "+I")
    assert (aug.nc, aug.mc) == (code.nc + code.mc, code.mc)
    n = 96
    llr = f["llr"][:n]
    random_s = np.random.default_rng(3).integers(0, 2, (n, code.mc), dtype=np.uint8)
    try:
        for setting in sd.SETTINGS:
            q, step, scale, offset = setting
            aug.set_min_sum_quantization(q, step)
            aug.set_min_sum_correction(scale, offset)
            for syn in (f["s"][:n], random_s):
                wide = np.concatenate((llr, sd.SHORTEN * (1.0 - 2.0 * syn)), axis=1)
                for early, iterations in ((True, 50), (False, 6)) if scale < 1.0 else ((False, 6), (False, 1)):
                    ref = aug.decode_batch(wide, early_term=early, iterations=iterations, decoding="BP_MS", want=("iters", "hard", "llr_out"))
                    got = _call(dec, llr, gf2_ref.pack(syn), setting, early_term=early, iterations=iterations)
                    assert np.array_equal(got["iters"], ref["iters"].astype(np.uint32)), (name, setting, early)
                    assert np.array_equal(gf2_ref.unpack(got["hard_bits"], code.nc), ref["hard"][:, :code.nc]), (name, setting, early)
                    assert np.array_equal(got["llr_out"], ref["llr_out"][:, :code.nc])
                    tie = ref["llr_out"][:, code.nc:] == 0.0
                    assert np.array_equal(ref["hard"][:, code.nc:] == syn, ~tie | (syn == 1)) and (scale == 1.0 or not tie.any())
    finally:
        aug.set_min_sum_quantization(0)
        aug.set_min_sum_correction(1.0, 0.0)


# ---- 3. special values ----
@pytest.mark.parametrize("name", ("sd_mix", "sd_small"))
def test_special_values(codes, name):
    dec, code = codes.decoder(name), codes.gf2(name)
    f = codes.frames(name)
    rng = np.random.default_rng(12)
    n, nc = 64, code.nc
    s = gf2_ref.pack(f["s"][:n])
    for setting in (BASE, sd.SETTINGS[1], sd.SETTINGS[2]):
        q, step = setting[0], setting[1]
        qmax = (1 << (q - 1)) - 1
        x = f["llr"][:n].copy()
        x[0], x[1] = 0.0, -0.0
        x[2] = np.where(rng.random(nc) < 0.5, 0.0, -0.0)
        edge = [s_ * (qmax + h) * step for s_ in (1.0, -1.0) for h in (-0.5, 0.5)] + [s_ * (k + 0.5) * step for s_ in (1.0, -1.0) for k in (0, 1, 2)]
        special = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 99999.9, -99999.9, 1e300, -1e300, 5e-324] + edge
        for r in range(3, 24):
            at = rng.choice(nc, len(special), replace=False)
            x[r, at] = special
        want = _expect(codes, name, x, f["s"][:n], setting)
        got = _call(dec, x, s, setting)
        assert _same(got, want), (name, setting, _differing(got, want))
        zero = _call(dec, x, s, setting, iterations=0)  # the quantized input itself
        L = sd.quantize(x, q, step)
        assert np.array_equal(zero["llr_out"], L * step) and np.array_equal(gf2_ref.unpack(zero["hard_bits"], nc), L <= 0) and not zero["iters"].any()
        with np.errstate(over="ignore"):
            for dt in (np.float32, np.float16):
                typed = x.astype(np.float32).astype(dt)
                typed[24, :4] = np.asarray([6e-8, -6e-8, 65504.0, -65504.0], dt)  # (binary16: subnormals and the largest)
                if dt == np.float16:
                    assert np.isinf(typed[3:24]).sum() >= 21 * 4  # 99999.9 is an infinity in binary16
                want = _expect(codes, name, typed, f["s"][:n], setting)
                got = _call(dec, typed, s, setting)
                assert _same(got, want), (name, setting, dt, _differing(got, want))
                assert _same(_call(dec, typed.astype(np.float64), s, setting), want)
        k = rng.integers(-128, 128, (n, nc)).astype(np.int8)
        k[0, :6] = (-128, -127, 127, 0, qmax, -qmax)
        k[1] = -128
        want = _expect(codes, name, k, f["s"][:n], setting)
        got = _call(dec, k, s, setting)
        assert _same(got, want), (name, setting, "int8", _differing(got, want))
        assert _same(_call(dec, k.astype(np.float64) * step, s, setting), want)  # an int8 counts steps


# ---- 4. call shapes and buffer kinds ----
@pytest.mark.parametrize("name", ("sd_r36", "sd_mix"))
def test_rows_of_a_call_are_the_call_on_the_rows(codes, name):
    f, dec = codes.frames(name), codes.decoder(name)
    n = 128
    llr, s = f["llr"][:n], gf2_ref.pack(f["s"][:n])
    want = _expect(codes, name, llr, f["s"][:n])
    for a, b in ((0, 1), (1, n), (0, n - 1), (n - 1, n), (0, 64), (64, n)):
        got = _call(dec, llr[a:b], s[a:b])
        assert _same(got, {k: want[k][a:b] for k in KEYS}), (name, a, b)
    for key in KEYS:  # a single output at a time
        got = _call(dec, llr, s, want=(key,))
        assert set(got) == {key} and _same(got, {key: want[key]}), key
    assert _call(dec, llr, s, want=()) == {}
    # one row for every frame
    row = llr[5]
    shared = _expect(codes, name, np.repeat(row[None, :], n, 0), f["s"][:n])
    for r in (row, row[None, :], row.astype(np.float16), cr.quantize(row, 6, 0.25)):
        ref = shared if r.dtype == np.float64 else _expect(codes, name, np.repeat(r.reshape(1, -1), n, 0), f["s"][:n])
        got = _call(dec, np.ascontiguousarray(r), s, shared_llr=True)
        assert _same(got, ref), (name, r.dtype, r.shape, _differing(got, ref))
    assert len(np.unique(shared["hard_bits"], axis=0)) > 1


def test_device_tensors_and_prefilled_buffers(codes):
    import torch
    dev = torch.device("cuda", 0)
    name = "sd_mix"
    f, dec, code = codes.frames(name), codes.decoder(name), codes.gf2(name)
    n, words = 128, (code.nc + 31) // 32
    llr, s = f["llr"][:n], f["s"][:n]
    want = _expect(codes, name, llr, s)
    side = torch.cuda.Stream(device=dev)
    out = {k: np.full(want[k].shape, 0x7F, want[k].dtype) for k in ("hard_bits", "iters", "weight")}
    out["llr_out"] = np.full(want["llr_out"].shape, np.nan)
    got = _call(dec, llr, gf2_ref.pack(s), want=(), out=out)  # host buffers end fully overwritten
    assert got["hard_bits"] is out["hard_bits"] and _same(out, want)

    def filled(*shape):
        return torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device=dev).view(torch.uint32)

    for stream, tdt, syn in ((None, torch.float64, gf2_ref.pack(s)), (side.cuda_stream, torch.float32, np.array(s)),
                             (None, torch.int8, gf2_ref.pack(s))):
        host_llr = cr.quantize(llr, 6, 0.25) if tdt == torch.int8 else llr
        t = torch.from_numpy(np.array(host_llr)).to(dev).to(tdt)
        ts = torch.from_numpy(syn.view(np.int32) if syn.dtype == np.uint32 else syn).to(dev)
        ts = ts.view(torch.uint32) if syn.dtype == np.uint32 else ts
        ref = want if tdt == torch.float64 else _expect(codes, name, t.cpu().numpy(), s)
        out = {"hard_bits": filled(n, words), "iters": filled(n), "weight": filled(n),
               "llr_out": torch.full((n, code.nc), float("nan"), dtype=torch.float64, device=dev)}
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream; the call runs on `stream`)
        _call(dec, t, ts, want=(), out=out, stream=stream)
        dec.synchronize(stream)
        host = {k: (v.cpu().numpy() if k == "llr_out" else v.view(torch.int32).cpu().numpy().view(np.uint32)) for k, v in out.items()}
        assert _same(host, ref), (str(tdt), _differing(host, ref))
        # device input, host output, and the other way round
        assert _same(_call(dec, t, ts, stream=stream), ref)
        mixed = {"weight": filled(n)}
        _call(dec, t.cpu().numpy(), syn, want=(), out=mixed)
        torch.cuda.synchronize()
        assert np.array_equal(mixed["weight"].view(torch.int32).cpu().numpy().view(np.uint32), ref["weight"])
    # a shared row on the device
    row = torch.from_numpy(llr[7].copy()).to(dev)
    ref = _expect(codes, name, np.repeat(llr[7][None, :], n, 0), s)
    assert _same(_call(dec, row, gf2_ref.pack(s), shared_llr=True), ref)


# ---- 5. no setting and no state ----
def test_the_settings_of_the_context_do_not_matter(codes):
    import libldpc_amd
    name = "sd_r36"
    f = codes.frames(name)
    llr, s = f["llr"][:96], gf2_ref.pack(f["s"][:96])
    want = {setting: _expect(codes, name, llr, f["s"][:96], setting) for setting in (BASE, sd.SETTINGS[3])}
    dec = libldpc_amd.HipDecoder(codes.path(name))
    modes = (("plain", lambda: None, lambda: None),
             ("correction", lambda: dec.set_min_sum_correction(0.5, 0.125), lambda: dec.set_min_sum_correction(1.0, 0.0)),
             ("quantized", lambda: dec.set_min_sum_quantization(4, 1.0), lambda: dec.set_min_sum_quantization(0)),
             ("ternary", lambda: dec.set_min_sum_ternary(2), lambda: dec.set_min_sum_ternary(0)),
             ("layered", lambda: dec.set_min_sum_schedule("layered"), lambda: dec.set_min_sum_schedule("flooding")),
             ("layered fixed", lambda: dec.set_min_sum_layered_fixed(5, 8, 0.5), lambda: dec.set_min_sum_layered_fixed(0)))
    for label, on, off in modes:
        on()
        for setting, ref in want.items():
            got = _call(dec, llr, s, setting)
            assert _same(got, ref), (label, setting, _differing(got, ref))
        off()
    assert dec.min_sum_quantization[0] == 0 and dec.min_sum_ternary == 0 and dec.min_sum_layered_fixed[0] == 0


def test_the_stream_interface_is_left_alone(codes):
    import libldpc_amd
    f = codes.frames("golden")
    llr, s = f["llr"], gf2_ref.pack(f["s"])
    want = _expect(codes, "golden", llr, f["s"])
    runs = []
    for between in (False, True):
        dec = libldpc_amd.HipDecoder(orc.H_TXT, orc.G_TXT)
        dec.set_noise("counter")
        dec.stream_begin("AWGN", 9, -3.0)
        got = []
        for batch in (40, 33):
            if between:
                assert _same(_call(dec, llr, s), want)
            got.append(dec.stream_decode(batch, iterations=10, decoding="BP_MS", want=("iters", "bit_errors", "llr_in", "llr_out", "codeword")))
        assert dec.stream_frame == 73
        runs.append(got)
    for plain, mixed in zip(*runs):
        for k in ("iters", "bit_errors", "llr_in", "llr_out", "codeword"):
            assert plain[k].dtype == mixed[k].dtype and np.array_equal(plain[k], mixed[k]), k
    assert all(r["codeword"].any() for r in runs[0])


# ---- 6. the chain on device tensors ----
def test_the_chain_on_device_tensors(codes):
    """Reconciliation without leaving the device: syndrome_batch(x) packed -> channel_batch(x, BSC, int8) -> syndrome_decode_batch
    -> bit_errors_batch against x and syndrome_batch of the result against s.  sd_r36 at eps = 0.04, 512 frames, Philox seed 9,
    (6, 0.25, 0.8125): the mirrors alone give 510 of 512 frames back as x, and none when the same LLRs are decoded toward
    zero (both recomputed and asserted here first).  Conditions: at least 90 % come back as x; toward zero at most 1 %."""
    import torch
    dev = torch.device("cuda", 0)
    name, eps, n = "sd_r36", 0.04, 512
    q, step, scale, offset = BASE
    code, dec = codes.gf2(name), codes.decoder(name)
    f = codes.frames(name, eps, n)
    k = cr.quantize(f["llr"], q, step)
    toward_s, toward_0 = _expect(codes, name, k, f["s"]), _expect(codes, name, k, None)
    back_s = (gf2_ref.unpack(toward_s["hard_bits"], code.nc) == f["x"]).all(1)
    back_0 = (gf2_ref.unpack(toward_0["hard_bits"], code.nc) == f["x"]).all(1)
    assert (int(back_s.sum()), int(back_0.sum())) == (510, 0)
    words, swords = (code.nc + 31) // 32, (code.mc + 31) // 32

    def u32(*shape):
        return torch.full(shape, -1, dtype=torch.int32, device=dev).view(torch.uint32)

    x = torch.from_numpy(f["x"].copy()).to(dev)
    s, s_after, left = u32(n, swords), u32(n, swords), u32(n)
    dec.syndrome_batch(x, want=(), out={"syndrome_bits": s})
    llr = torch.full((n, code.nc), 99, dtype=torch.int8, device=dev)
    dec.channel_batch(x, "BSC", eps, seed=sd.NOISE_SEED, llr="int8", q_bits=q, step=step, want=(), out={"llr": llr})
    out = {"hard_bits": u32(n, words), "iters": u32(n), "weight": u32(n)}
    zero = {"hard_bits": u32(n, words)}
    _call(dec, llr, s, want=(), out=out)
    _call(dec, llr, None, want=(), out=zero)
    errors, errors_0 = u32(n), u32(n)
    dec.bit_errors_batch(out["hard_bits"], x, out=errors)
    dec.bit_errors_batch(zero["hard_bits"], x, out=errors_0)
    dec.syndrome_batch(out["hard_bits"], want=(), out={"syndrome_bits": s_after, "weight": left})
    torch.cuda.synchronize()
    host = {k_: v.view(torch.int32).cpu().numpy().view(np.uint32) for k_, v in
            dict(s=s, s_after=s_after, left=left, errors=errors, errors_0=errors_0, **out).items()}
    assert np.array_equal(llr.cpu().numpy(), k) and np.array_equal(host["s"], gf2_ref.pack(f["s"]))  # the mirrors' inputs
    met = host["weight"] == 0
    assert 0 < met.sum() and (host["s_after"][met] == host["s"][met]).all()  # every frame with weight 0 has syndrome s
    assert np.array_equal(met, (host["s_after"] == host["s"]).all(1))
    same, same_0 = int((host["errors"] == 0).sum()), int((host["errors_0"] == 0).sum())
    print(f"chain {name} at eps {eps}: {n} frames, {int(met.sum())} reach s, {same} come back as x; toward zero {same_0}")
    assert same >= 0.9 * n and same_0 <= 0.01 * n
    assert _same({k_: host[k_] for k_ in ("hard_bits", "iters", "weight")}, {k_: toward_s[k_] for k_ in ("hard_bits", "iters", "weight")})
