"""ldpc_hip_syndrome_decode_layered_batch (include/ldpc_amd.h; libldpc_amd/csrc/kernels_syndrome_decode_layered.hip) on the
GPU: all four outputs against the numpy mirror of tests/syndrome_decode_layered_ref.py bit for bit, against the kernels that
exist without it (fixed-point layered min-sum toward zero, and on the augmented code [H | I]), special values, call shapes and
buffer kinds, the context's settings and a running stream, and the chain syndrome -> decode -> OSD on device tensors.

Inputs: random words x (not codewords) of numpy.random.default_rng(5), s = H x, the LLRs of x through the BSC mirror under
Philox seed 9, at a point per code where — by the mirror, asserted before any kernel runs — some frames reach s and some do
not (syndrome_decode_layered_ref.POINTS)."""
import itertools

import numpy as np
import pytest

import channel_ref as cr
import gf2_ref
import orc
import syndrome_decode_layered_ref as sdl
import syndrome_decode_ref as sd

pytestmark = pytest.mark.gpu
KEYS = sdl.KEYS
BASE = sdl.SETTINGS[0]


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    return sdl.Codes(tmp_path_factory.mktemp("sdl"))


def _same(got, want):
    return all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)


def _differing(got, want):
    return {k: np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1)).tolist()[:8] for k in want if not np.array_equal(got[k], want[k])}


def _call(dec, llr, syn, setting=BASE, want=KEYS, **kw):
    q, p, step, scale, offset = setting
    return dec.syndrome_decode_layered_batch(llr, syn, msg_bits=q, app_bits=p, step=step, scale=scale, offset=offset, want=want, **kw)


def _expect(codes, name, llr, syn, setting=BASE, early_term=True, iterations=50):
    return codes.mirror(name).expected(llr, syn, *setting, early_term, iterations)


# ---- 1. against the mirror ----
@pytest.mark.parametrize("name", sdl.NAMES)
def test_syndrome_decode_layered_equals_the_mirror(codes, name):
    f, dec, code = codes.frames(name), codes.decoder(name), codes.gf2(name)
    llr, s = f["llr"], f["s"]
    n = llr.shape[0]
    base = _expect(codes, name, llr, s)
    reached = base["weight"] == 0
    assert int(reached.sum()) == sdl.REACHED[name] and 0 < reached.sum() < n  # both kinds, before any kernel runs
    assert np.array_equal(reached, base["iters"] < 50)
    packed = gf2_ref.pack(s)
    got = _call(dec, llr, packed)
    assert _same(got, base), (name, _differing(got, base))
    assert not gf2_ref.high_bits(got["hard_bits"], code.nc).any()
    word = gf2_ref.unpack(got["hard_bits"], code.nc)
    assert np.array_equal(got["weight"], (code.syndrome(word)[0] != s).sum(1))  # 0 iff the word has syndrome s
    assert _same(_call(dec, llr, np.ascontiguousarray(s)), base), (name, "bytes")
    if code.mc % 32:  # the bits of the last syndrome word from mc on are ignored
        dirty = packed.copy()
        dirty[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(code.mc % 32)
        assert _same(_call(dec, llr, dirty), base), (name, "high bits")
    m = 64  # the variants on the first frames
    a, sa, pa = llr[:m], s[:m], packed[:m]
    for early, iterations in ((False, 50), (True, 0), (False, 0), (True, 1), (False, 1)):
        want = _expect(codes, name, a, sa, BASE, early, iterations)
        got = _call(dec, a, pa, early_term=early, iterations=iterations)
        assert _same(got, want), (name, early, iterations, _differing(got, want))
    for setting in sdl.SETTINGS[1:]:
        for early, iterations in ((True, 50), (False, 50), (False, 1), (True, 0)):
            want = _expect(codes, name, a, sa, setting, early, iterations)
            for syn in (pa, np.ascontiguousarray(sa)):
                got = _call(dec, a, syn, setting, early_term=early, iterations=iterations)
                assert _same(got, want), (name, setting, early, iterations, _differing(got, want))
    # the element types: the call on the typed values is the mirror on the same values
    for setting, kind in itertools.product(sdl.SETTINGS, ("float32", "float16", "int8")):
        typed = cr.convert(a, kind, setting[0], setting[2])
        for early, iterations in ((True, 50), (False, 1), (False, 0)):
            want = _expect(codes, name, typed, sa, setting, early, iterations)
            for syn in (pa, np.ascontiguousarray(sa)):
                got = _call(dec, typed, syn, setting, early_term=early, iterations=iterations)
                assert _same(got, want), (name, kind, setting, early, iterations, _differing(got, want))
    # no syndrome: toward zero
    want = _expect(codes, name, a, None)
    assert _same(_call(dec, a, None), want) and _same(_call(dec, a, np.zeros_like(pa)), want)
    assert (want["weight"] > 0).any()  # (the words are no codewords)


# ---- 2. against kernels that exist without it ----
def _toward_zero_inputs(codes, name, n=96):
    """LLRs of random words (never codewords: they run to the end) and of the all-zero codeword (most stop)."""
    f = codes.frames(name)
    return np.concatenate((f["llr"][:n // 3], cr.bsc(codes.gf2(name), sdl.POINTS[name][0], sd.NOISE_SEED, np.arange(n - n // 3), None)[1]))


@pytest.mark.parametrize("name", sdl.NAMES)
def test_without_a_syndrome_it_is_fixed_point_layered_min_sum(codes, name):
    """Identity (a)."""
    import libldpc_amd
    llr = _toward_zero_inputs(codes, name)
    dec, old = codes.decoder(name), libldpc_amd.HipDecoder(codes.path(name))
    stopped = set()
    for setting in sdl.SETTINGS:
        q, p, step, scale, offset = setting
        old.set_min_sum_layered_fixed(q, p, step)
        old.set_min_sum_correction(scale, offset)
        for kind in ("float64", "float32", "float16", "int8"):
            typed = cr.convert(llr, kind, q, step)
            for early, iterations in ((True, 50), (False, 5), (True, 1)):
                ref = old.decode_batch_typed(typed, early_term=early, iterations=iterations, decoding="BP_MS", want=("iters", "llr_out", "hard_bits"))
                got = _call(dec, typed, None, setting, early_term=early, iterations=iterations)
                assert np.array_equal(got["iters"], ref["iters"].astype(np.uint32)), (name, setting, kind, early, iterations)
                assert np.array_equal(got["hard_bits"], ref["hard_bits"]) and np.array_equal(got["llr_out"], ref["llr_out"]), (name, setting, kind)
                stopped |= set((got["iters"] < iterations).tolist())
    assert stopped == {True, False}


@pytest.mark.parametrize("name", ("sd_r36", "sd_small", "sdl_odd"))
def test_with_a_syndrome_it_is_that_decoder_on_the_augmented_code(codes, name):
    """Identity (b), the route this call replaces: [H | I], 99999.9 (1 - 2 s) on the extra columns, decode_batch toward zero
    under fixed-point layered min-sum, without early termination; where every check node has degree <= 7 (sd_mix has degree 8:
    tests/test_syndrome_decode_layered_host.py) and app_bits > msg_bits."""
    f, dec, code = codes.frames(name), codes.decoder(name), codes.gf2(name)
    aug = codes.decoder(name + "+I")
    assert (aug.nc, aug.mc) == (code.nc + code.mc, code.mc)
    n = 96
    llr = f["llr"][:n]
    random_s = np.random.default_rng(3).integers(0, 2, (n, code.mc), dtype=np.uint8)
    try:
        for setting in sdl.SETTINGS:
            q, p, step, scale, offset = setting
            if p <= q:
                continue
            aug.set_min_sum_layered_fixed(q, p, step)
            aug.set_min_sum_correction(scale, offset)
            for syn in (f["s"][:n], random_s):
                wide = np.concatenate((llr, sd.SHORTEN * (1.0 - 2.0 * syn)), axis=1)
                for iterations in (1, 6):
                    ref = aug.decode_batch(wide, early_term=False, iterations=iterations, decoding="BP_MS", want=("iters", "hard", "llr_out"))
                    got = _call(dec, llr, gf2_ref.pack(syn), setting, early_term=False, iterations=iterations)
                    assert np.array_equal(gf2_ref.unpack(got["hard_bits"], code.nc), ref["hard"][:, :code.nc]), (name, setting, iterations)
                    assert np.array_equal(got["llr_out"], ref["llr_out"][:, :code.nc]), (name, setting, iterations)
    finally:
        aug.set_min_sum_layered_fixed(0)
        aug.set_min_sum_correction(1.0, 0.0)


def test_a_code_outside_the_layered_plan_is_refused(codes):
    dec = codes.decoder("sd_wide")
    assert dec.syndrome_decode_layered_lds_bytes() == -1
    with pytest.raises(RuntimeError, match="ldpc_hip_syndrome_decode_layered_batch"):
        dec.syndrome_decode_layered_batch(np.ones((4, dec.nc), np.int8))
    assert dec.syndrome_decode_batch(np.ones((4, dec.nc), np.int8))["iters"].shape == (4,)  # (the flooding call takes it)


def test_argument_refusals(codes):
    """Every refusal of the header, with frames: -1, the entry named, nothing written."""
    dec = codes.decoder("sd_small")
    llr = np.ones((4, dec.nc), np.float64)
    nan = float("nan")
    out = {"iters": np.full(4, 77, np.uint32)}
    for kw in (dict(msg_bits=1), dict(msg_bits=9), dict(app_bits=5), dict(app_bits=17), dict(msg_bits=8, app_bits=7), dict(step=nan), dict(step=0.0),
               dict(step=2.0**-21), dict(step=2.0**21), dict(scale=nan), dict(scale=0.0), dict(scale=1.5), dict(offset=nan), dict(offset=-1.0),
               dict(offset=2e6)):
        with pytest.raises(RuntimeError, match="ldpc_hip_syndrome_decode_layered_batch"):
            dec.syndrome_decode_layered_batch(llr, want=(), out=out, **kw)
    import ctypes as ct
    from libldpc_amd.binding import ldpc_hip_syndrome_decode_layered as Spec
    lib = dec.lib
    good = (5, 1, 6, 8, 0.25, 0.8125, 0.0, 0)

    def run(spec=good, kind=0, src=llr.ctypes.data, fmt=0):
        p = None if spec is None else ct.byref(Spec(*spec))
        return lib.ldpc_hip_syndrome_decode_layered_batch(dec.ctx, p, 4, src, kind, None, fmt, None, out["iters"].ctypes.data, None, None, None)

    for bad in (dict(spec=None), dict(spec=good[:1] + (2,) + good[2:]), dict(spec=good[:7] + (2,)), dict(kind=4), dict(fmt=2), dict(src=None)):
        assert run(**bad) == -1 and b"ldpc_hip_syndrome_decode_layered_batch" in lib.ldpc_hip_last_error(), bad
    assert (out["iters"] == 77).all()
    assert run() == 0 and (out["iters"] <= 5).all()


# ---- 3. special values ----
@pytest.mark.parametrize("name", ("sd_mix", "sdl_odd"))
def test_special_values(codes, name):
    dec, code = codes.decoder(name), codes.gf2(name)
    f = codes.frames(name)
    rng = np.random.default_rng(12)
    n, nc = 64, code.nc
    s = gf2_ref.pack(f["s"][:n])
    for setting in (BASE, sdl.SETTINGS[1], sdl.SETTINGS[2]):
        q, step = setting[0], setting[2]
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
@pytest.mark.parametrize("name", ("sd_r36", "sdl_odd"))
def test_rows_of_a_call_are_the_call_on_the_rows(codes, name):
    f, dec = codes.frames(name), codes.decoder(name)
    n = 128
    llr, s = f["llr"][:n], gf2_ref.pack(f["s"][:n])
    want = _expect(codes, name, llr, f["s"][:n])
    k8 = cr.quantize(llr, 6, 0.25)  # (sdl_odd: rows of 63 bytes, every alignment)
    want8 = _expect(codes, name, k8, f["s"][:n])
    for a, b in ((0, 1), (1, n), (0, n - 1), (n - 1, n), (0, 64), (64, n), (3, 7), (2, 9)):
        got = _call(dec, llr[a:b], s[a:b])
        assert _same(got, {k: want[k][a:b] for k in KEYS}), (name, a, b)
        got = _call(dec, k8[a:b], s[a:b])
        assert _same(got, {k: want8[k][a:b] for k in KEYS}), (name, a, b, "int8")
    for r in range(1, 4):  # every subset of the outputs
        for keys in itertools.combinations(KEYS, r):
            got = _call(dec, llr, s, want=keys)
            assert set(got) == set(keys) and _same(got, {k: want[k] for k in keys}), keys
    assert _call(dec, llr, s, want=()) == {}
    # one row for every frame
    row = llr[5]
    shared = _expect(codes, name, np.repeat(row[None, :], n, 0), f["s"][:n])
    for r in (row, row[None, :], row.astype(np.float32), row.astype(np.float16), cr.quantize(row, 6, 0.25)):
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
                             (None, torch.float16, np.array(s)), (None, torch.int8, gf2_ref.pack(s))):
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
    want = {setting: _expect(codes, name, llr, f["s"][:96], setting) for setting in (BASE, sdl.SETTINGS[3])}
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
    """syndrome_batch(x) packed -> syndrome_decode_layered_batch on int8 LLRs -> osd_syndrome_batch on its llr_out, all on device
    tensors; sd_r36 at its operating point.  The decoder's outputs are the mirror's; a frame that reached s comes out of OSD
    as it went in (OSD_CODEWORD, the same word); every word OSD returns has syndrome s (the code's rows are independent or
    the status says infeasible)."""
    import torch
    dev = torch.device("cuda", 0)
    name = "sd_r36"
    q, p, step, scale, offset = BASE
    code, dec = codes.gf2(name), codes.decoder(name)
    f = codes.frames(name)
    n = f["llr"].shape[0]
    k = cr.quantize(f["llr"], q, step)
    want = _expect(codes, name, k, f["s"])
    words, swords = (code.nc + 31) // 32, (code.mc + 31) // 32

    def u32(*shape):
        return torch.full(shape, -1, dtype=torch.int32, device=dev).view(torch.uint32)

    x = torch.from_numpy(f["x"].copy()).to(dev)
    s, s_after, left = u32(n, swords), u32(n, swords), u32(n)
    dec.syndrome_batch(x, want=(), out={"syndrome_bits": s})
    llr = torch.from_numpy(k).to(dev)
    out = {"hard_bits": u32(n, words), "iters": u32(n), "weight": u32(n), "llr_out": torch.full((n, code.nc), float("nan"), dtype=torch.float64, device=dev)}
    _call(dec, llr, s, want=(), out=out)
    osd = {"word": u32(n, words), "status": u32(n)}
    dec.osd_syndrome_batch(out["llr_out"], s, candidates=16, pair_depth=0, want=(), out=osd)
    dec.syndrome_batch(osd["word"], want=(), out={"syndrome_bits": s_after, "weight": left})
    torch.cuda.synchronize()
    host = {k_: v.view(torch.int32).cpu().numpy().view(np.uint32) for k_, v in
            dict(s=s, s_after=s_after, left=left, hard_bits=out["hard_bits"], iters=out["iters"], weight=out["weight"], **osd).items()}
    host["llr_out"] = out["llr_out"].cpu().numpy()
    assert np.array_equal(host["s"], gf2_ref.pack(f["s"]))
    assert _same({k_: host[k_] for k_ in KEYS}, want)
    met = host["weight"] == 0
    assert 0 < met.sum() < n
    assert (host["status"][met] == dec.OSD_CODEWORD).all() and np.array_equal(host["word"][met], host["hard_bits"][met])
    feasible = host["status"] != dec.OSD_INFEASIBLE
    assert feasible[met].all() and np.array_equal(host["s_after"][feasible], host["s"][feasible])
    assert np.array_equal(host["left"][feasible], f["s"].sum(1)[feasible])  # (syndrome_batch counts the ones of H x)
    print(f"chain {name}: {n} frames, {int(met.sum())} reach s in the decoder, {int(feasible.sum())} after OSD")
