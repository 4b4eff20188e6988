"""ldpc_hip_osd_batch and ldpc_hip_osd_lds_bytes (include/ldpc_amd.h) without a GPU: the exported symbols and their
prototypes, everything the call refuses before it touches a device, the binding's own checks, the LDS formula, the numpy
mirror (tests/osd_ref.py) against enumeration over all codewords of a tiny code and against the identities the header
states, and the compile-time resources of kernels_osd.hip."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

import erasure_ref as er
import generator_codes as gc
import gf2_ref
import orc
import osd_ref as osd

F64, F32, F16, I8 = 0, 1, 2, 3
OSD = b"ldpc_hip_osd_batch"


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(lib):
    """Every test of this file, the mirror's included, is about the contract of one entry: without it none has a subject."""
    assert hasattr(lib, "ldpc_hip_osd_batch") and hasattr(lib, "ldpc_hip_osd_lds_bytes")


def _regular(directory, nc, seed=1):
    sys.path.insert(0, os.path.join(orc.ROOT, "tools"))
    import gen_regular_code
    path = os.path.join(str(directory), f"r{nc}.h.txt")
    if not os.path.exists(path):
        open(path, "w").write(gen_regular_code.generate(nc, 3, 6, seed))
    return path, ""


# 7 check nodes over 13 columns: check node 5 is the sum of check nodes 0 and 1 (rank 6), column 12 is listed by none
TINY = ((0, 1, 2, 6), (2, 3, 4, 7), (4, 5, 0, 8), (1, 3, 5, 9), (0, 3, 10, 11), (0, 1, 3, 4, 6, 7), (6, 7, 8, 9, 10))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("osd")
    out = {"golden": (orc.H_TXT, orc.G_TXT), "r240": _regular(d, 240), "r14000": _regular(d, 14000)}
    for name in ("s40x60", "s129x150t5", "s800x100"):
        out[name] = gc.write_pair(d, name)
    out["s40x60_hdup"] = (er.repeat_entries(out["s40x60"][0], os.path.join(str(d), "s40x60_hdup.h.txt")), "")  # parallel edges in H
    tiny = os.path.join(str(d), "tiny.h.txt")
    open(tiny, "w").write("\n".join(f"{r} {c}" for r, cols in enumerate(TINY) for c in cols) + "\n6 12\n6 12\n")  # (12: listed twice)
    out["tiny"] = (tiny, "")
    return out


def test_symbols_and_signatures(lib):
    vp, u64, u32, i32 = ct.c_void_p, ct.c_uint64, ct.c_uint32, ct.c_int
    assert lib.ldpc_hip_osd_batch.argtypes == [vp, u32, u64, vp, i32, vp, vp, vp, vp, vp, vp] and lib.ldpc_hip_osd_batch.restype == i32
    assert lib.ldpc_hip_osd_lds_bytes.argtypes == [vp] and lib.ldpc_hip_osd_lds_bytes.restype == ct.c_int64
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_osd_batch(ldpc_hip_ctx *ctx, uint32_t candidates, uint64_t n, const void *llr, int llr_type, "
            "uint32_t *word_out, uint32_t *flips, uint64_t *metric, uint32_t *flipped_column, uint32_t *status, "
            "void *hip_stream);") in flat
    assert "int64_t ldpc_hip_osd_lds_bytes(const ldpc_hip_ctx *ctx);" in flat
    assert "LDPC_HIP_OSD_CODEWORD = 0, LDPC_HIP_OSD_ORDER0 = 1, LDPC_HIP_OSD_REPROCESSED = 2" in flat
    import libldpc_amd
    d = libldpc_amd.HipDecoder
    assert (d.OSD_CODEWORD, d.OSD_ORDER0, d.OSD_REPROCESSED, d.OSD_NO_COLUMN) == (osd.CODEWORD, osd.ORDER0, osd.REPROCESSED, osd.NO_COLUMN)
    assert d.LLR_TYPES == {"float64": F64, "float32": F32, "float16": F16, "int8": I8}


def test_refusals_come_before_the_gpu(lib, files):
    """No GPU here: a call that reached the device would fail with another message, or not at all."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(*files["s129x150t5"])
    llr = np.ones((2, d.nc), np.float64)
    word, cnt, metric = np.zeros((2, (d.nc + 31) // 32), np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint64)
    err = lib.ldpc_hip_last_error

    def run(n, candidates=4, kind=F64, src=llr.ctypes.data, ctx=None, outs=True):
        o = [word.ctypes.data, cnt.ctypes.data, metric.ctypes.data, cnt.ctypes.data, cnt.ctypes.data] if outs else [None] * 5
        return lib.ldpc_hip_osd_batch(ctx or d.ctx, candidates, n, src, kind, *o, None)

    for n in (0, 2):
        for kind in (4, -1, 17):
            assert run(n, kind=kind) == -1 and OSD in err() and b"LLR type" in err(), (n, kind, err())
    assert run(2, src=None) == -1 and OSD in err()
    # after the checks n == 0 returns 0 (no GPU needed): every type, any number of candidates, with and without buffers
    for kind in (F64, F32, F16, I8):
        for candidates in (0, 1, d.nc, 2**32 - 1):
            assert run(0, candidates, kind) == 0 and run(0, candidates, kind, None) == 0 and run(0, candidates, kind, outs=False) == 0
    # a code whose frame does not fit is refused before the GPU, frames or none
    big = libldpc_amd.HipDecoder(*files["r14000"])
    assert big.osd_lds_bytes() == -1 and lib.ldpc_hip_osd_lds_bytes(big.ctx) == -1
    wide = np.ones((2, 14000), np.float32)
    for n in (0, 2):
        assert run(n, kind=F32, src=wide.ctypes.data, ctx=big.ctx) == -1 and OSD in err() and b"LDS" in err()
    with pytest.raises(RuntimeError, match="ldpc_hip_osd_batch"):
        big.osd_batch(wide[:0])
    # the binding, n == 0
    for dt in (np.float64, np.float32, np.float16, np.int8):
        r = d.osd_batch(np.zeros((0, d.nc), dt), candidates=8)
        assert set(r) == set(osd.KEYS) and r["word"].shape == (0, (d.nc + 31) // 32) and r["status"].shape == (0,)
        assert r["metric"].dtype == np.uint64 and all(r[k].dtype == np.uint32 for k in osd.KEYS if k != "metric")


def test_binding_refuses_other_dtypes_and_shapes(lib, files):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(*files["s40x60"])
    words = (d.nc + 31) // 32
    ok = np.zeros((0, d.nc), np.float32)
    for dt in (np.uint8, np.int16, np.int32, np.int64, np.uint32, np.bool_, np.complex64):
        with pytest.raises(TypeError, match="osd_batch"):
            d.osd_batch(np.zeros((1, d.nc), dt))
    for shape in ((1, d.nc + 1), (1, d.nc - 1), (d.nc,), (1, 1, d.nc), (1, words)):
        with pytest.raises(ValueError, match="osd_batch"):
            d.osd_batch(np.zeros(shape, np.float64))
    for candidates in (-1, 2**32):
        with pytest.raises(ValueError, match="candidates"):
            d.osd_batch(ok, candidates=candidates)
    with pytest.raises(KeyError):
        d.osd_batch(ok, want=("rank",))
    with pytest.raises(TypeError, match="metric"):
        d.osd_batch(ok, want=(), out={"metric": np.zeros(0, np.uint32)})
    with pytest.raises(TypeError, match="flips"):
        d.osd_batch(ok, want=(), out={"flips": np.zeros(0, np.uint64)})
    with pytest.raises(ValueError, match="status"):
        d.osd_batch(ok, want=(), out={"status": np.zeros(1, np.uint32)})
    with pytest.raises(ValueError, match="word"):
        d.osd_batch(ok, want=(), out={"word": np.zeros((0, words + 1), np.uint32)})


def _formula(code):
    """The formula of the header, restated; None where the header says -1."""
    if code.nc >= 65536 or code.mc > 32768:
        return None
    v = -(-code.nc // 64)
    s = (v + 1) | 1
    total = -(-(max(8 * code.mc * s, -(-4 * code.nc // 8) * 8) + 24 * v + -(-2 * code.nc // 8) * 8 + 384) // 16) * 16
    return total if total <= 160 * 1024 else None


def test_lds_bytes_formula(lib, files):
    import libldpc_amd
    golden = gf2_ref.Gf2Code(*files["golden"])
    assert (golden.nc, golden.mc) == (1152, 1024)
    assert _formula(golden) == 158768 == 8 * 1024 * 19 + 24 * 18 + 2304 + 384 <= 160 * 1024  # one frame per CU
    assert _formula(gf2_ref.Gf2Code(*files["tiny"])) == 7 * 3 * 8 + 24 + 32 + 384  # (13 columns: one word and its neighbours)
    seen = {}
    for name in ("golden", "s40x60", "s129x150t5", "s800x100", "r240", "r14000"):
        want = _formula(gf2_ref.Gf2Code(*files[name]))
        seen[name] = libldpc_amd.HipDecoder(*files[name]).osd_lds_bytes()
        assert seen[name] == (-1 if want is None else want), name
    assert seen["r14000"] == -1 and all(v > 0 for k, v in seen.items() if k != "r14000")
    assert seen["r240"] == 120 * 5 * 8 + 24 * 4 + 480 + 384 and seen["r240"] * 16 < 160 * 1024  # small codes: several frames a CU


def _noisy(code, n, snr_db, seed, encoded=True):
    """(codewords, llr): n frames of BPSK in Gaussian noise, LLR = 2 y / sigma^2, binary64."""
    rng = np.random.default_rng(seed)
    cw = code.encode(rng.integers(0, 2, (n, code.kc), dtype=np.uint8)) if code.has_g and encoded else np.zeros((n, code.nc), np.uint8)
    sigma2 = 10 ** (-snr_db / 10)
    y = 1.0 - 2.0 * cw + rng.normal(0.0, np.sqrt(sigma2), cw.shape)
    return cw, 2.0 * y / sigma2


def test_values_of_the_first_step():
    x = np.asarray([[0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf, 2.0**-13, -(2.0**-12), 524287.5, 524288.0, 1e300, 0.75 + 2.0**-13]])
    z, q = osd.values(x)
    assert z.tolist() == [[1, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0]]
    assert q.tolist() == [[0, 0, 4096, 4096, 0, 2**31 - 1, 2**31 - 1, 0, 1, 2**31 - 2048, 2**31 - 1, 2**31 - 1, 3072]]
    z, q = osd.values(np.asarray([[-128, -1, 0, 1, 127]], np.int8))
    assert z.tolist() == [[1, 1, 1, 0, 0]] and q.tolist() == [[128 * 4096, 4096, 0, 4096, 127 * 4096]]
    for dt in (np.float32, np.float16):
        v = np.asarray([[1.5, -2.25, 6e-8, np.nan, -np.inf, 65504.0]], dt)
        for a, b in zip(osd.values(v), osd.values(v.astype(np.float64))):
            assert np.array_equal(a, b)
    assert osd.order_of(np.asarray([5, 0, 5, 3, 0])).tolist() == [1, 4, 3, 0, 2]  # ties: the smaller column first


def test_the_mirror_equals_enumeration_on_a_tiny_code(files):
    """From the definition alone: P by the rank of column sets, x0 as the ONLY codeword that agrees with z on K, every x_j
    likewise, the winner by comparing their metrics."""
    code = gf2_ref.Gf2Code(*files["tiny"])
    m = osd.matrix(code)
    assert (code.nc, code.mc) == (13, 7) and not m[:, 12].any() and er.incidence(code)[6, 12] == 2
    words = osd.codewords(m)
    assert words.shape[0] == 2 ** (13 - 6)  # rank 6: one check node depends on the others
    rng = np.random.default_rng(5)
    n = 80
    llr = np.round(rng.normal(1.0, 1.5, (n, code.nc)) * 4) / 4  # a grid: equal reliabilities happen
    llr[:8] = np.where(words[rng.integers(0, len(words), 8)] == 1, -1.0, 1.0) * rng.integers(1, 4, (8, code.nc))  # codewords
    llr[8, 3], llr[9, 5], llr[10, :] = np.nan, np.inf, 0.0
    z, q = osd.values(llr)
    statuses = set()
    for cap in (0, 1, 3, 7, 20):
        got = osd.decode(code, llr, cap)
        for f in range(n):
            solved, kept = osd.solved_set_by_rank(m, osd.order_of(q[f]))
            assert len(solved) == 6 and len(kept) == 7
            agree = words[(words[:, kept] == z[f, kept]).all(1)]
            assert agree.shape[0] == 1  # x0 exists and is the only one
            best, word, column = int(q[f][agree[0] != z[f]].sum()), agree[0], osd.NO_COLUMN
            for t in range(min(cap, len(kept))):
                want = z[f, kept].copy()
                want[t] ^= 1
                xj = words[(words[:, kept] == want).all(1)]
                assert xj.shape[0] == 1
                mj = int(q[f][xj[0] != z[f]].sum())
                if mj < best:
                    best, word, column = mj, xj[0], kept[t]
            is_cw = (words == z[f]).all(1).any()
            status = osd.CODEWORD if is_cw else osd.REPROCESSED if column != osd.NO_COLUMN else osd.ORDER0
            assert np.array_equal(gf2_ref.unpack(got["word"][f:f + 1], code.nc)[0], word), (cap, f)
            assert (got["flips"][f], got["metric"][f], got["flipped_column"][f], got["status"][f]) == ((word != z[f]).sum(), best, column, status), (cap, f)
            statuses.add(status)
    assert statuses == {osd.CODEWORD, osd.ORDER0, osd.REPROCESSED}
    assert (osd.decode(code, llr, 7)["status"][:8] == osd.CODEWORD).all()


POINTS = {"s40x60": 3.0, "s40x60_hdup": 3.0, "s129x150t5": 3.0, "r240": 1.0}


@pytest.mark.parametrize("name", tuple(POINTS))
def test_identities_of_the_mirror(files, name):
    code = gf2_ref.Gf2Code(*files[name])
    m = osd.matrix(code)
    n = 24
    cw, llr = _noisy(code, n, POINTS[name], 3)
    llr[:4] = (1.0 - 2.0 * cw[:4]) * np.abs(llr[:4])  # codewords go in
    z, q = osd.values(llr)
    rank = len(osd.reduce(m, np.arange(code.nc))[0])
    k = code.nc - rank
    caps = (0, 1, 8, k, k + 50)
    got = osd.decode_many(code, llr, caps)
    before = None
    for cap in caps:
        r = got[cap]
        word = gf2_ref.unpack(r["word"], code.nc)
        assert not code.syndrome(word)[1].any() and not gf2_ref.high_bits(r["word"], code.nc).any(), (name, cap)  # codewords come out
        assert np.array_equal(word[:4], cw[:4]) and (r["status"][:4] == osd.CODEWORD).all() and not r["metric"][:4].any() and not r["flips"][:4].any()
        assert np.array_equal(r["status"] == osd.CODEWORD, code.syndrome(z)[1] == 0)
        assert np.array_equal(r["flips"], (word != z).sum(1)) and np.array_equal(r["metric"], (q * (word != z)).sum(1).astype(np.uint64))
        assert np.array_equal(r["status"] == osd.REPROCESSED, r["flipped_column"] != osd.NO_COLUMN)
        if before is not None:
            assert (r["metric"] <= before).all(), (name, cap)  # non-increasing in candidates
        before = r["metric"]
    assert 0 < (got[0]["status"] != osd.CODEWORD).sum() and (got[k]["metric"] < got[0]["metric"]).any(), name
    for key in osd.KEYS:
        assert np.array_equal(got[k][key], got[k + 50][key]), key  # more than |K| counts as |K|
    # P does not depend on the rows' order, nor x0 on the pivots
    shuffle = np.random.default_rng(9).permutation(code.mc)
    for f in range(4, 10):
        order = osd.order_of(q[f])
        a, b = osd.reduce(m, order), osd.reduce(m[shuffle], order)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) == rank
        assert np.array_equal(a[2], b[2])  # the reduced row of a pivot column is the same row, wherever it stands


def test_an_entry_listed_twice_cancels(files):
    plain, dup = gf2_ref.Gf2Code(*files["s40x60"]), gf2_ref.Gf2Code(*files["s40x60_hdup"])
    twice = np.argwhere(er.incidence(dup) == 2)
    assert twice.shape == (1, 2) and er.incidence(dup).max() == 3
    r, c = twice[0]
    assert osd.matrix(dup)[r, c] == 0 and osd.matrix(plain)[r, c] == 1 and (osd.matrix(dup) != osd.matrix(plain)).sum() == 1
    _, llr = _noisy(plain, 12, 2.0, 4)
    a, b = osd.decode(plain, llr, 8), osd.decode(dup, llr, 8)
    assert not np.array_equal(a["word"], b["word"])  # another matrix, other codewords
    assert not dup.syndrome(gf2_ref.unpack(b["word"], dup.nc))[1].any()  # (three listings count as one: the syndrome's rule too)


def test_kernel_resources(lib):
    """kernels_osd.hip: one kernel, no scratch, no spills, no static LDS beside the frame's, and registers that let a
    workgroup of 1024 threads run (at most 128)."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_osd.hip")
    assert res and len(res) == 1 and "osd_kernel" in next(iter(res))
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] <= 128 and r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
    assert len(build.kernel_resources("kernels_erasure_solve.hip")) == 1 and len(build.kernel_resources("kernels_erasure.hip")) == 2
    assert len(build.kernel_resources("kernels_convert.hip")) == 4  # (the neighbours are as they were: three widenings, one packing)
