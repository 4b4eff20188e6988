"""Transmitted codewords beyond g.txt on the GPU: every encoder kernel and every decoder's codeword path on the code pairs of
tests/generator_codes.py (generator known by construction; test_generator_codes_host.py holds the pairs to their shapes and
kernel paths and chooses the channel points).  Every comparison is np.array_equal — against the det-mode oracle for the
parity paths, against the numpy mirrors fed the GPU's own llr_in for the opt-in min-sum settings.  No tolerance anywhere."""
import ctypes as ct
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

import generator_codes as gc
import orc
import philox_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("iters", "bit_errors", "hard", "llr_out", "llr_in", "codeword")


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """name -> (h path, g path, oracle code with G); the library under test is the tree's own."""
    import libldpc_amd
    assert os.path.realpath(libldpc_amd.LIB_PATH) == os.path.realpath(os.path.join(ROOT, "libldpc_amd", "libldpc.so"))
    d = tmp_path_factory.mktemp("pairs")
    out = {}
    for name in list(gc.SYSTEMATIC) + list(gc.NULL_SPACE):
        h, g = gc.write_pair(d, name)
        out[name] = (h, g, orc.Code(h, g))
    return out


def _oracle_codewords(code, chan, x, seed, count):
    """The codewords of frames [0, count) from one orc_chan_run_frames (orc.Code.run_frames without the other vectors)."""
    L = orc.lib()
    ch = L.orc_chan_new(code.h, orc.CHAN[chan], seed, orc.MATH_DET, 0, 1, 0, 0)
    L.orc_chan_set_param(ch, float(x))
    cw = np.zeros((count, code.nc), np.uint8)
    L.orc_chan_run_frames(ch, 0, count, None, None, None, None, None, cw.ctypes.data_as(ct.c_void_p))
    L.orc_chan_free(ch)
    return cw


def _recount(code, hard, codeword):
    tx = np.asarray(code.bit_pos)
    return (hard[:, tx] != codeword[:, tx]).sum(1)


# ---- a. encoder shapes ----
# batches around the 1024-thread prefix scan (one frame per thread with idle threads, exactly full + 1, two per thread with a
# ragged end, three per thread) and two skips, which launch the codeword kernel for the batch's last frame alone
BATCHES = (1, 31, -7, 33, 1023, -1500, 1025, 2500)  # (negative: stream_skip)


@pytest.mark.parametrize("name", gc.ENCODER_PAIRS)
def test_encoder_shapes(pairs, name):
    """The running codeword of every frame, across batch boundaries and skips, equals the oracle's.  (What this cannot see:
    the bits of the last info word from kc on.  The engine refuses G.rows > kc, so neither the masks nor the walk read them;
    a library that fills them with other draws, or leaves the counter mode's unmasked, passes here and everywhere.)"""
    import libldpc_amd
    h, g, code = pairs[name]
    dec = libldpc_amd.HipDecoder(h, g)
    want = _oracle_codewords(code, "AWGN", 3.0, 5, sum(abs(b) for b in BATCHES))
    assert want.any(axis=1).mean() > 0.9 and not want[:, code.g_cols:].any()
    dec.stream_begin("AWGN", 5, 3.0)
    pos = 0
    for i, b in enumerate(BATCHES):
        if b < 0:
            dec.stream_skip(-b)
        else:
            got = dec.stream_decode(b, iterations=i % 2, want=("codeword",))["codeword"]
            assert np.array_equal(got, want[pos:pos + b]), (name, b, pos)
        pos += abs(b)
    assert dec.stream_frame == pos


# ---- b. counter-noise encoder ----
@pytest.mark.parametrize("name", gc.COUNTER_PAIRS)
def test_counter_noise_codewords(pairs, name):
    import libldpc_amd
    h, g, code = pairs[name]
    dec = libldpc_amd.HipDecoder(h, g)
    n, seed = 200, 21
    dec.set_noise("counter")
    dec.stream_begin("AWGN", seed, 1.0)
    for first in (0, 2**33 + n):  # (frames beyond 2^32: the counter's upper word)
        dec.stream_skip(first - dec.stream_frame)
        got = dec.stream_decode(n, want=("codeword", "hard", "bit_errors"))
        info = pr.info_bits(seed, first + np.arange(n), code.kc)
        for f in range(n):
            assert np.array_equal(got["codeword"][f, :code.g_cols], code.encode(info[f, :code.g_rows])), (name, first, f)
        assert not got["codeword"][:, code.g_cols:].any()
        assert np.array_equal(got["bit_errors"], _recount(code, got["hard"], got["codeword"]))
        assert got["codeword"].any(1).mean() > 0.9 and (got["bit_errors"] > 0).any()


# ---- c. decoders with transmitted codewords ----
@pytest.mark.parametrize("residency", list(gc.DECODERS))
def test_decoders_with_transmitted_codewords(pairs, residency):
    import libldpc_amd
    name, form, fused, _ = gc.DECODERS[residency]
    h, g, code = pairs[name]
    dec = libldpc_amd.HipDecoder(h, g)
    assert dec.residency == residency.split("_")[0] and dec.register_form == form and bool(dec.fused_plan()["ok"]) == fused
    points = gc.POINTS[residency]
    for case, (ch, decoding, early, iters, compat) in gc.CASES.items():
        dec.set_bec_compat(compat)
        dec.stream_begin(ch, gc.SEED, points[case])
        dec.stream_skip(gc.SKIP)
        r = dec.stream_decode(gc.FRAMES, early_term=early, iterations=iters, decoding=decoding, want=OUT)
        o = code.run_frames(ch, points[case], seed=gc.SEED, skip=gc.SKIP, count=gc.FRAMES, min_sum=decoding == "BP_MS",
                            early_term=early, iters=iters, math=orc.MATH_DET, bec_compat=compat)
        for k in OUT:
            assert np.array_equal(r[k], o[k].astype(r[k].dtype)), (residency, case, k)
        assert np.array_equal(r["bit_errors"], _recount(code, r["hard"], r["codeword"])), (residency, case)
        gc.check_mixed(r["iters"], r["bit_errors"], r["codeword"], early, iters, (residency, case))
    dec.set_bec_compat(False)
    for setting, (ch, takes) in gc.OPT_IN.items():
        if residency not in takes:
            continue
        o = code.run_frames(ch, points[setting], seed=gc.SEED, skip=gc.SKIP, count=gc.FRAMES, iters=0, math=orc.MATH_DET)
        for early in (True, False):
            gc.switch_on(dec, setting)
            dec.stream_begin(ch, gc.SEED, points[setting])
            dec.stream_skip(gc.SKIP)
            r = dec.stream_decode(gc.FRAMES, early_term=early, iterations=gc.OPT_IN_ITERATIONS, decoding="BP_MS", want=OUT)
            gc.switch_off(dec)
            assert np.array_equal(r["llr_in"], o["llr_in"]) and np.array_equal(r["codeword"], o["codeword"]), (residency, setting)
            m = gc.mirror_decode(code, setting, r["llr_in"], o["codeword"], early)
            assert np.array_equal(r["iters"], m["iters"].astype(np.uint32)), (residency, setting, early)
            assert np.array_equal(r["hard"], m["hard"]), (residency, setting, early)
            assert np.array_equal(r["llr_out"].view(np.uint64), m["llr_out"].view(np.uint64)), (residency, setting, early)
            assert np.array_equal(r["bit_errors"], _recount(code, r["hard"], o["codeword"])), (residency, setting, early)
            if early:
                gc.check_mixed(r["iters"], r["bit_errors"], r["codeword"], True, gc.OPT_IN_ITERATIONS, (residency, setting))


# ---- d. sharded encoding ----
def _shard_worker(rank, world, shm, h, g, chan, x, seed, target, steps, q):
    sys.path.insert(0, ROOT)
    import libldpc_amd
    dec = libldpc_amd.HipDecoder(h, g)
    dec.set_bec_compat(True)
    comm = libldpc_amd.Comm(rank, world, shm_name=shm)
    dec.stream_begin(chan, seed, x)
    out = []
    for _ in range(steps):
        bufs, step = dec.stream_decode_sharded(comm, target, want=("iters", "bit_errors", "codeword"))
        out.append((step,) + tuple(bufs[k][:step[3]].copy() for k in ("iters", "bit_errors", "codeword")))
    q.put((rank, out))


@pytest.mark.parametrize("chan,x", [("AWGN", 3.0), ("BEC", 0.2)])
@pytest.mark.parametrize("name", gc.SHARDED_PAIRS)
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_encoding(pairs, world, name, chan, x):
    """Every frame of two sharded steps — whichever rank encoded and decoded it — has the iteration count, the bit-error
    count and the codeword of the same frame in a one-rank run, whose codewords are the oracle's.  (At most `world` = 3 rank
    processes and this one hold the GPU at a time.)"""
    import libldpc_amd
    h, g, code = pairs[name]
    target, steps, seed = 12000, 2, 13
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    shm = f"/ldpc_amd_test_{os.getpid()}_g{world}"
    ps = [ctx.Process(target=_shard_worker, args=(r, world, shm, h, g, chan, x, seed, target, steps, q)) for r in range(world)]
    [p.start() for p in ps]
    got = dict(q.get(timeout=300) for _ in range(world))
    [p.join(timeout=60) for p in ps]
    total = got[0][-1][0][0] + got[0][-1][0][1]
    dec = libldpc_amd.HipDecoder(h, g)
    dec.set_bec_compat(True)
    dec.stream_begin(chan, seed, x)
    ref = dec.stream_decode(total, want=("iters", "bit_errors", "codeword"))
    assert np.array_equal(ref["codeword"], _oracle_codewords(code, chan, x, seed, total))
    assert ref["codeword"].any(1).mean() > 0.9 and (ref["bit_errors"] > 0).any() and (ref["bit_errors"] == 0).any()
    pos, busy = 0, set()
    for s in range(steps):
        step0 = got[0][s][0]
        assert step0[0] == pos
        nxt = step0[0]
        for r in range(world):
            step, it, be, cw = got[r][s]
            assert step[:2] == step0[:2] and step[2] == nxt
            sl = slice(step[2], step[2] + step[3])
            assert np.array_equal(it, ref["iters"][sl]) and np.array_equal(be, ref["bit_errors"][sl]), (s, r)
            assert np.array_equal(cw, ref["codeword"][sl]), (s, r)
            if step[3]:
                busy.add(r)
            nxt += step[3]
        assert nxt == step0[0] + step0[1]
        pos = nxt
    assert busy == set(range(world)) and total >= target * steps * 0.7


# ---- e. batch counters ----
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099, 12288, 12292, 16387, 65536])
def test_batch_counters_sizes_and_alignment(pairs, n):
    """ldpc_hip_batch_counters against int64 sums in numpy: sizes on both sides of the vector loads (n % 4), of the unrolled
    loop (it runs from n / 4 > 3072 on) and of one pass of the 1024 threads; 16-byte-aligned pointers, pointers one element
    further (the scalar loop), and one of each; bit-error counts whose sum leaves 32 bits."""
    import torch
    import libldpc_amd
    dec = libldpc_amd.HipDecoder(pairs["s40x60"][0])
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(n)
    max_iters = 50
    it = np.where(rng.random(n + 1) < 0.5, max_iters, rng.integers(0, max_iters, n + 1)).astype(np.int32)
    be = np.where(rng.random(n + 1) < 0.7, 0, rng.integers(1, 2**31, n + 1)).astype(np.int32)
    be[-1] = 2**31 - 1
    t_it, t_be = torch.from_numpy(it).to(dev), torch.from_numpy(be).to(dev)
    assert t_it.data_ptr() % 16 == 0 and t_be.data_ptr() % 16 == 0
    c = torch.full((5,), -1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for off_it, off_be in ((0, 0), (1, 1), (0, 1), (1, 0)):
        a, b = t_it[off_it:off_it + n], t_be[off_be:off_be + n]
        assert a.data_ptr() % 16 == 4 * off_it and b.data_ptr() % 16 == 4 * off_be
        ia, ib = it[off_it:off_it + n].astype(np.int64), be[off_be:off_be + n].astype(np.int64)
        for early in (True, False):
            c.fill_(-1)
            dec.batch_counters(a.data_ptr(), b.data_ptr(), n, max_iters, early, c.data_ptr(), stream)
            torch.cuda.synchronize()
            want = [n, int((ib > 0).sum()), int(ib.sum()), int(ia.sum()), int((ia < max_iters).sum()) if early else 0]
            assert c.cpu().tolist() == want, (n, off_it, off_be, early)
    if n >= 4099:
        assert int(be[:n].astype(np.int64).sum()) > 2**32
