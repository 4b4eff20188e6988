"""Counter-based noise mode on the GPU (include/ldpc_amd.h, ldpc_hip_set_noise): the device generator and
every channel prologue against the Python restatement (tests/philox_ref.py), the decode of that noise against the
decode-from-LLRs path and the oracle, invariance under batch splits, skips and sharding, and error rates against the
parity stream's.  Statistical bounds are five standard errors."""
import math
import os
import subprocess
import time

import numpy as np
import pytest

import orc
import philox_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTS = ("iters", "bit_errors", "hard", "llr_out", "llr_in")


def _dec(path=orc.H_TXT, gen=""):
    import libldpc_amd
    return libldpc_amd.HipDecoder(path, gen)


@pytest.fixture(scope="module")
def hdec():
    return _dec()


@pytest.fixture(scope="module")
def hcode():
    return orc.Code(orc.H_TXT)


def _counter(dec, chan, seed, x):
    dec.set_noise("counter")
    dec.stream_begin(chan, seed, x)


def test_philox_known_answers_and_sample(hdec):
    for (c0, c1, c2, c3), (k0, k1), out in pr.KNOWN_ANSWERS:
        got = hdec.philox(k0 | k1 << 32, c3, c1 | c2 << 32, c0, 1)
        assert tuple(int(v) for v in got[0]) == out
    rng = np.random.default_rng(11)
    for _ in range(24):
        seed, tag = int(rng.integers(0, 2**63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 3))
        frame = int(rng.integers(0, 2**62)) if rng.random() < 0.5 else int(rng.integers(0, 2**20))
        first = int(rng.integers(0, 2**32 - 4096))
        got = hdec.philox(seed, tag, frame, first, 300)
        assert np.array_equal(got, pr.blocks(seed, tag, [frame], first + np.arange(300))[0])


def _transmitted(code):
    tx = np.zeros(code.nc, bool)
    tx[code.bit_pos] = True
    return tx


@pytest.mark.parametrize("chan,x", [("BSC", 0.1), ("BEC", 0.3)])
def test_bsc_bec_llr_in_exact(hdec, hcode, chan, x):
    n, seed = 300, 9
    hits = pr.draws(seed, np.arange(n), hcode.nct, x)
    tx = _transmitted(hcode)
    for compat in ((False, True) if chan == "BEC" else (False,)):
        hdec.set_bec_compat(compat)
        _counter(hdec, chan, seed, x)
        got = hdec.stream_decode(n, want=OUTS)
        want = np.zeros((n, hcode.nc))
        if chan == "BSC":
            delta = math.log((1 - x) / x)
            want[:, hcode.bit_pos] = np.where(hits, -delta, delta)
        else:
            want[:, hcode.bit_pos] = np.where(hits, float(orc.ERASURE), 0.0)
        assert np.array_equal(got["llr_in"][:, tx], want[:, tx])
        # punctured / shortened columns: the parity mode's values
        hdec.set_noise("reference")
        hdec.stream_begin(chan, seed, x)
        par = hdec.stream_decode(4, want=("llr_in",))
        assert np.array_equal(got["llr_in"][:, ~tx], np.repeat(par["llr_in"][:1, ~tx], n, 0))
        if chan == "BEC":  # the decode of those symbols is the oracle's
            for f in range(0, n, 37):
                it, out, hard = hcode.decode_bec(got["llr_in"][f].astype(np.uint8), np.zeros(hcode.nc, np.uint8), compat=compat)
                assert it == got["iters"][f] and np.array_equal(hard, got["hard"][f])
                assert np.array_equal(out.astype(np.float64), got["llr_out"][f])
    hdec.set_bec_compat(False)


CASES = [("BP", True), ("BP", False), ("BP_MS", False)]


@pytest.mark.parametrize("code", ["h", "8k"])
def test_counter_decode_equals_decode_of_its_llrs(code, h8k_file):
    path, n, x = (orc.H_TXT, 3000, -4.0) if code == "h" else (h8k_file, 256, 2.0)
    dec = _dec(path)
    llr_first = None
    for decoding, et in CASES:
        _counter(dec, "AWGN", 3, x)
        got = dec.stream_decode(n, early_term=et, decoding=decoding, want=OUTS)
        ref = dec.decode_batch(got["llr_in"], early_term=et, decoding=decoding, want=("iters", "bit_errors", "hard", "llr_out"))
        for k in ("iters", "bit_errors", "hard", "llr_out"):
            assert np.array_equal(got[k], ref[k]), (code, decoding, et, k)
        if llr_first is None:
            llr_first = got["llr_in"]
        assert np.array_equal(got["llr_in"], llr_first)  # a frame's channel does not depend on the decoder
        oc = orc.Code(path)
        for f in (0, 1):
            it, out, hard = oc.decode(got["llr_in"][f], min_sum=decoding == "BP_MS", early_term=et, math=orc.MATH_DET)
            assert it == got["iters"][f] and np.array_equal(hard, got["hard"][f]) and np.array_equal(out, got["llr_out"][f])


def test_split_and_skip_invariance(hdec, hcode):
    want = ("iters", "bit_errors", "llr_in")
    _counter(hdec, "AWGN", 5, -4.0)
    one = hdec.stream_decode(5000, want=want)
    _counter(hdec, "AWGN", 5, -4.0)
    parts = [hdec.stream_decode(m, want=want) for m in (1, 999, 4000)]
    for k in want:
        assert np.array_equal(one[k], np.concatenate([p[k] for p in parts])), k
    _counter(hdec, "AWGN", 5, -4.0)
    hdec.stream_skip(1234)
    sl = hdec.stream_decode(100, want=want)
    for k in want:
        assert np.array_equal(sl[k], one[k][1234:1334]), k
    assert hdec.stream_frame == 1334
    t0 = time.perf_counter()
    hdec.stream_skip(2**40)
    assert time.perf_counter() - t0 < 0.5 and hdec.stream_frame == 2**40 + 1334
    far = hdec.stream_decode(1, want=want)
    nrm, r = pr.awgn_normals(5, [2**40 + 1334], hcode.nct)
    sigma2 = 10 ** (4.0 / 10)
    got = (far["llr_in"][0, hcode.bit_pos] * sigma2 / 2 - 1) / math.sqrt(sigma2)
    assert np.all(np.abs(got - nrm[0]) <= 2e-5 + 2e-7 / r[0])


def test_generator_codewords(hcode):
    dec = _dec(orc.H_TXT, orc.G_TXT)
    gc = orc.Code(orc.H_TXT, orc.G_TXT)
    n, seed = 400, 21
    _counter(dec, "AWGN", seed, 1.0)
    dec.stream_skip(2**33)  # (frames beyond 2^32: the counter's upper word)
    got = dec.stream_decode(n, want=("codeword", "hard", "bit_errors"))
    info = pr.info_bits(seed, 2**33 + np.arange(n), gc.kc)
    for f in range(n):
        assert np.array_equal(got["codeword"][f, :gc.g_cols], gc.encode(info[f, :gc.g_rows])), f
    be = (got["hard"][:, gc.bit_pos] != got["codeword"][:, gc.bit_pos]).sum(1)
    assert np.array_equal(be, got["bit_errors"])
    assert got["codeword"].any(1).mean() > 0.9  # (not the all-zero codeword)


@pytest.mark.parametrize("chan,x", [("AWGN", -4.0), ("BEC", 0.7)])
def test_sharded_echo_equals_one_rank(chan, x):
    import libldpc_amd
    dec = _dec(orc.H_TXT, orc.G_TXT)
    dec.set_bec_compat(chan == "BEC")
    want = ("iters", "bit_errors", "llr_in", "codeword")
    target = 1000
    _counter(dec, chan, 4, x)
    full = dec.stream_decode(2 * target, want=want)
    for world in (2, 3, 8):
        for r in range(world):
            comm = libldpc_amd.Comm(r, world, echo=True)
            _counter(dec, chan, 4, x)
            for step in range(2):
                bufs, (s_first, s_frames, first, n) = dec.stream_decode_sharded(comm, target, want=want)
                assert s_first == step * target and s_frames == target and dec.shard_capacity(target, world) >= n
                for k in want:
                    assert np.array_equal(bufs[k][:n], full[k][first:first + n]), (world, r, k)
            assert comm.exchange_stats()["calls"] == 0
            comm.close()
    dec.set_bec_compat(False)


def test_no_state_leaks_between_modes(golden_frames):
    dec = _dec()
    _counter(dec, "AWGN", 0, -4.0)
    dec.stream_decode(20000)
    dec.stream_skip(10**6)
    assert dec.jump_tasks == 0
    with pytest.raises(RuntimeError, match="counter"):
        dec.stream_raw_draws
    dec.set_fast_mode(1)
    with pytest.raises(RuntimeError, match="fast"):
        dec.stream_decode(4)
    dec.set_fast_mode(0)
    dec.set_noise("reference")
    dec.stream_begin("AWGN", 0, -4.0)
    got = dec.stream_decode(8, want=OUTS)
    g = "awgn_bp_m4/"
    assert np.array_equal(got["iters"], golden_frames[g + "iters"]) and np.array_equal(got["hard"], golden_frames[g + "hard"])
    assert np.max(np.abs(got["llr_out"] - golden_frames[g + "llr_out"])) < 1e-5


def _cli(args, out, extra=()):
    exe = os.path.join(ROOT, "libldpc_amd", "ldpcsim")
    txt = subprocess.run([exe, orc.H_TXT, str(out)] + list(args) + list(extra), stdout=subprocess.PIPE, text=True, check=True).stdout
    return txt, [ln.split()[:5] for ln in open(out).read().splitlines()]


def test_cli_counter_devices_equal_one_device(tmp_path):
    args = ["0.2", "0.29", "0.04", "--channel", "BSC", "--max-frames", "3000", "--frame-error-count", "20"]
    head, one = _cli(args, tmp_path / "one.txt", ("--noise", "counter"))
    assert "NON-PARITY" in head and len(one) >= 3
    _, many = _cli(args, tmp_path / "many.txt", ("--noise", "counter", "--devices", "0,0", "--comm", "shm"))
    assert many == one
    head_ref, ref = _cli(args, tmp_path / "ref.txt")
    assert "NON-PARITY" not in head_ref and ref != one


def test_awgn_normals_statistics(hdec, hcode):
    nf, seed, x = 4096, 77, 0.0
    _counter(hdec, "AWGN", seed, x)
    llr = hdec.stream_decode(nf, want=("llr_in",))["llr_in"][:, hcode.bit_pos]
    sigma2 = 10 ** (-x / 10)
    n = (llr * sigma2 / 2 - 1) / math.sqrt(sigma2)
    N = n.size
    assert abs(n.mean()) < 5 / math.sqrt(N)
    assert abs(n.var() - 1) < 5 * math.sqrt(2 / N)
    for t in (2, 3):
        p = math.erfc(t / math.sqrt(2))
        assert abs((np.abs(n) > t).mean() - p) < 5 * math.sqrt(p * (1 - p) / N), t
    within = (n[:, :-1] * n[:, 1:]).mean()
    between = (n[:-1] * n[1:]).mean()
    assert abs(within) < 5 / math.sqrt(n[:, 1:].size) and abs(between) < 5 / math.sqrt(n[1:].size)
    assert np.abs(n).max() <= 6.77
    # against the restatement: the binary32 arguments are the same; the device's log2 / sqrt / sin / cos are within a few
    # ulp (2e-5 absolute at |n| <= 6.77 is about 40 ulp of binary32 there); where u is within 1e-6 of 1 a radius near 0
    # takes the log's absolute error (~2e-7 in r^2) as 2e-7 / r
    want, r = pr.awgn_normals(seed, np.arange(nf), hcode.nct)
    err = np.abs(n - want)
    assert np.all(err <= 2e-5 + 2e-7 / r), float(err.max())


def _rates(dec, chan, x, counter, frames):
    dec.set_noise("counter" if counter else "reference")
    dec.set_bec_compat(chan == "BEC")
    dec.stream_begin(chan, 1, x)
    it, be = [], []
    for _ in range(frames // 65536):
        o = dec.stream_decode(65536)
        it.append(o["iters"]), be.append(o["bit_errors"])
    it, be = np.concatenate(it).astype(np.float64), np.concatenate(be)
    return (be > 0).mean(), it.mean(), it.var()


@pytest.mark.parametrize("chan,x", [("AWGN", -4.0), ("BSC", 0.24), ("BEC", 0.9)])
def test_error_rates_agree_with_parity(hdec, chan, x):
    N = 2**20
    p_ref, m_ref, v_ref = _rates(hdec, chan, x, False, N)
    p_ctr, m_ctr, v_ctr = _rates(hdec, chan, x, True, N)
    hdec.set_bec_compat(False)
    hdec.set_noise("reference")
    assert 1e-3 <= p_ref <= 0.5, p_ref
    assert abs(p_ctr - p_ref) <= 5 * math.sqrt(2 * p_ref * (1 - p_ref) / N), (p_ref, p_ctr)
    assert abs(m_ctr - m_ref) <= 5 * math.sqrt((v_ref + v_ctr) / N), (m_ref, m_ctr)
