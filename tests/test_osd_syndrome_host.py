"""ldpc_hip_osd_syndrome_batch and ldpc_hip_osd_syndrome_lds_bytes (include/ldpc_amd.h) without a GPU: the exported symbols
and their prototypes, what the call refuses before it touches a device, the binding's own checks, the LDS formula, the
compile-time resources of kernels_osd_syndrome.hip, and the numpy mirror (tests/osd_syndrome_ref.py) against enumeration of
every x with M x = s on a code of 13 columns — feasibility, order 0, every single and every pair from the definition, the
order among equal metrics — and against the four identities the header states."""
import ctypes as ct
import os

import numpy as np
import pytest

import gf2_ref
import orc
import osd_ref as osd
import osd_syndrome_ref as osr
import test_osd_host as plain

F64, F32, F16, I8 = 0, 1, 2, 3
U8, PACKED32 = 0, 1
ENTRY = b"ldpc_hip_osd_syndrome_batch"
files = plain.files  # the codes of test_osd_host.py (module-scoped fixture)


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module", autouse=True)
def the_entry_exists(lib):
    """Every test of this file, the mirror's included, is about the contract of one entry: without it none has a subject."""
    assert hasattr(lib, "ldpc_hip_osd_syndrome_batch") and hasattr(lib, "ldpc_hip_osd_syndrome_lds_bytes")


def test_symbols_and_signatures(lib):
    vp, u64, u32, i32 = ct.c_void_p, ct.c_uint64, ct.c_uint32, ct.c_int
    f = lib.ldpc_hip_osd_syndrome_batch
    assert f.argtypes == [vp, u32, u32, u64, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp] and f.restype == i32
    assert lib.ldpc_hip_osd_syndrome_lds_bytes.argtypes == [vp] and lib.ldpc_hip_osd_syndrome_lds_bytes.restype == ct.c_int64
    flat = " ".join(open(os.path.join(orc.ROOT, "include", "ldpc_amd.h")).read().split())
    assert ("int ldpc_hip_osd_syndrome_batch(ldpc_hip_ctx *ctx, uint32_t candidates, uint32_t pair_depth, uint64_t n, const void *llr, "
            "int llr_type, const void *syndrome, int syndrome_format, uint32_t *word_out, uint32_t *flips, uint64_t *metric, "
            "uint32_t *flipped_columns /* [n][2] */, uint32_t *status, void *hip_stream);") in flat
    assert "int64_t ldpc_hip_osd_syndrome_lds_bytes(const ldpc_hip_ctx *ctx);" in flat
    assert "LDPC_HIP_OSD_REPROCESSED_PAIR = 3, LDPC_HIP_OSD_INFEASIBLE = 4" in flat
    assert "OSD toward a syndrome is not offered" not in flat
    import libldpc_amd
    d = libldpc_amd.HipDecoder
    assert (d.OSD_REPROCESSED_PAIR, d.OSD_INFEASIBLE) == (osr.REPROCESSED_PAIR, osr.INFEASIBLE) == (3, 4)
    assert (osr.CODEWORD, osr.ORDER0, osr.REPROCESSED, osr.NO_COLUMN) == (d.OSD_CODEWORD, d.OSD_ORDER0, d.OSD_REPROCESSED, d.OSD_NO_COLUMN)


def test_refusals_come_before_the_gpu(lib, files):
    """No GPU here: a call that reached the device would fail with another message, or not at all."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(*files["s129x150t5"])
    llr = np.ones((2, d.nc), np.float64)
    syn = np.zeros((2, d.mc), np.uint8)
    word, cnt, metric = np.zeros((2, (d.nc + 31) // 32), np.uint32), np.zeros(4, np.uint32), np.zeros(2, np.uint64)
    err = lib.ldpc_hip_last_error

    def run(n, candidates=4, depth=4, kind=F64, src=llr.ctypes.data, s=syn.ctypes.data, fmt=U8, ctx=None, outs=True):
        o = [word.ctypes.data, cnt.ctypes.data, metric.ctypes.data, cnt.ctypes.data, cnt.ctypes.data] if outs else [None] * 5
        return lib.ldpc_hip_osd_syndrome_batch(ctx or d.ctx, candidates, depth, n, src, kind, s, fmt, *o, None)

    for n in (0, 2):
        for kind in (4, -1, 17):
            assert run(n, kind=kind) == -1 and ENTRY in err() and b"LLR type" in err(), (n, kind, err())
        for fmt in (2, -1, 9):
            for s in (syn.ctypes.data, None):
                assert run(n, fmt=fmt, s=s) == -1 and ENTRY in err() and b"format" in err(), (n, fmt, err())
        for depth in (257, 1000, 2**32 - 1):
            assert run(n, depth=depth) == -1 and ENTRY in err() and b"pair_depth" in err(), (n, depth, err())
    assert run(2, src=None) == -1 and ENTRY in err()
    # after the checks n == 0 returns 0 (no GPU needed)
    for kind in (F64, F32, F16, I8):
        for candidates, depth in ((0, 0), (1, 2), (d.nc, 256), (2**32 - 1, 256)):
            for fmt in (U8, PACKED32):
                assert run(0, candidates, depth, kind, fmt=fmt) == 0 and run(0, candidates, depth, kind, None, None, fmt) == 0
                assert run(0, candidates, depth, kind, fmt=fmt, outs=False) == 0
    # a code whose frame does not fit is refused before the GPU, frames or none
    big = libldpc_amd.HipDecoder(*files["r14000"])
    assert big.osd_syndrome_lds_bytes() == -1 and lib.ldpc_hip_osd_syndrome_lds_bytes(big.ctx) == -1
    wide = np.ones((2, 14000), np.float32)
    for n in (0, 2):
        assert run(n, kind=F32, src=wide.ctypes.data, s=None, ctx=big.ctx) == -1 and ENTRY in err() and b"LDS" in err()
    with pytest.raises(RuntimeError, match="ldpc_hip_osd_syndrome_batch"):
        big.osd_syndrome_batch(wide[:0])
    with pytest.raises(RuntimeError, match="pair_depth"):
        d.osd_syndrome_batch(llr[:0], pair_depth=257)
    # the binding, n == 0
    for dt in (np.float64, np.float32, np.float16, np.int8):
        for s in (None, syn[:0], np.zeros((0, (d.mc + 31) // 32), np.uint32)):
            r = d.osd_syndrome_batch(np.zeros((0, d.nc), dt), s, candidates=8, pair_depth=8)
            assert set(r) == set(osr.KEYS) and r["word"].shape == (0, (d.nc + 31) // 32) and r["flipped_columns"].shape == (0, 2)
            assert r["metric"].dtype == np.uint64 and all(r[k].dtype == np.uint32 for k in osr.KEYS if k != "metric")


def test_binding_refuses_other_dtypes_and_shapes(lib, files):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(*files["s40x60"])
    ok = np.zeros((0, d.nc), np.float32)
    for dt in (np.uint8, np.int16, np.int32, np.uint32, np.bool_):
        with pytest.raises(TypeError, match="osd_syndrome_batch"):
            d.osd_syndrome_batch(np.zeros((1, d.nc), dt))
    for shape in ((1, d.nc + 1), (d.nc,), (1, 1, d.nc)):
        with pytest.raises(ValueError, match="osd_syndrome_batch"):
            d.osd_syndrome_batch(np.zeros(shape, np.float64))
    for dt in (np.int8, np.float32, np.uint16):
        with pytest.raises(TypeError, match="osd_syndrome_batch"):
            d.osd_syndrome_batch(ok, np.zeros((0, d.mc), dt))
    with pytest.raises(ValueError, match="osd_syndrome_batch"):
        d.osd_syndrome_batch(ok, np.zeros((0, d.mc + 1), np.uint8))
    with pytest.raises(ValueError, match="rows"):
        d.osd_syndrome_batch(ok, np.zeros((1, d.mc), np.uint8))
    for kw in ({"candidates": -1}, {"candidates": 2**32}, {"pair_depth": -1}, {"pair_depth": 2**32}):
        with pytest.raises(ValueError, match="pair_depth"):
            d.osd_syndrome_batch(ok, **kw)
    with pytest.raises(KeyError):
        d.osd_syndrome_batch(ok, want=("flipped_column",))
    with pytest.raises(ValueError, match="flipped_columns"):
        d.osd_syndrome_batch(ok, want=(), out={"flipped_columns": np.zeros(0, np.uint32)})
    with pytest.raises(TypeError, match="metric"):
        d.osd_syndrome_batch(ok, want=(), out={"metric": np.zeros(0, np.uint32)})


def formula(code):
    """The formula of the header, restated; None where the header says -1."""
    if code.nc >= 65536 or code.mc > 32768:
        return None
    v = -(-code.nc // 64)
    s = (v + 1) | 1
    total = -(-(max(8 * code.mc * s, -(-4 * code.nc // 8) * 8) + 24 * v + -(-2 * code.nc // 8) * 8 + 1536) // 16) * 16
    return total if total <= 160 * 1024 else None


def test_lds_bytes_formula(lib, files):
    import libldpc_amd
    golden = gf2_ref.Gf2Code(*files["golden"])
    assert formula(golden) == 159920 == 8 * 1024 * 19 + 24 * 18 + 2304 + 1536 <= 160 * 1024  # still one frame per CU
    for name in ("golden", "s40x60", "s129x150t5", "s800x100", "r240", "tiny", "r14000"):
        want = formula(gf2_ref.Gf2Code(*files[name]))
        d = libldpc_amd.HipDecoder(*files[name])
        assert d.osd_syndrome_lds_bytes() == (-1 if want is None else want), name
        if want is not None:
            assert d.osd_syndrome_lds_bytes() == d.osd_lds_bytes() + 1536 - 384, name
    assert formula(gf2_ref.Gf2Code(*files["r14000"])) is None


def test_kernel_resources(lib):
    """kernels_osd_syndrome.hip: one kernel, no scratch, no spills, no static LDS beside the frame's, and registers that let
    a workgroup of 1024 threads run (at most 128); kernels_osd.hip still holds its one kernel."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_osd_syndrome.hip")
    assert res and len(res) == 1 and "osd_syndrome_kernel" in next(iter(res))
    for name, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r["VGPRs"] <= 128 and r.get("LDS Size [bytes/block]", 0) == 0, (name, r)
    assert len(build.kernel_resources("kernels_osd.hip")) == 1


# ---- the mirror against the definition ----
def _tiny_inputs(code, m, n=320):
    """LLRs on a grid of quarters (equal reliabilities happen), among them a NaN, an infinity and an all-zero row; syndromes:
    s = M u of a random word u on the even frames (feasible), random bits on the odd ones, all zero on the first four."""
    rng = np.random.default_rng(6)
    llr = np.round(rng.normal(1.0, 1.5, (n, code.nc)) * 4) / 4
    llr[8, 3], llr[9, 5], llr[10, :] = np.nan, np.inf, 0.0
    llr[40:] = rng.integers(-2, 3, (n - 40, code.nc)).astype(np.float64)  # the coarse grid: 0, 1, 2 and signs
    u = rng.integers(0, 2, (n, code.nc), dtype=np.uint8)
    s = ((u.astype(np.int64) @ m.T.astype(np.int64)) & 1).astype(np.uint8)
    s[1::2] = rng.integers(0, 2, (n // 2, code.mc), dtype=np.uint8)
    s[:4] = 0
    return llr, s


def test_the_mirror_equals_enumeration_on_a_tiny_code(files):
    """From the definition alone: every x with M x = s listed; P by the rank of column sets; x0, every x_t and every x_{t1,t2}
    as the ONLY listed word that agrees with the wanted bits on K; the best candidate as the first of the smallest metric in
    the order of e; it wins iff it is strictly below x0.  Also that the ties the order is about do occur."""
    code = gf2_ref.Gf2Code(*files["tiny"])
    m = osd.matrix(code)
    assert (code.nc, code.mc) == (13, 7)
    every = ((np.arange(2**code.nc)[:, None] >> np.arange(code.nc)[None, :]) & 1).astype(np.int64)
    syndromes = (every @ m.T.astype(np.int64)) & 1
    llr, s = _tiny_inputs(code, m)
    z, q = osd.values(llr)
    settings = ((0, 0), (1, 0), (3, 0), (0, 2), (0, 3), (2, 4), (7, 7), (20, 256), (1, 5), (0, 7))
    got = osr.decode_many(code, llr, s, settings)
    seen, single_beats_equal_pair, first_of_equal_pairs = set(), 0, 0
    for f in range(llr.shape[0]):
        words = every[(syndromes == s[f]).all(1)].astype(np.uint8)
        met = ((m.astype(np.int64) @ z[f].astype(np.int64)) & 1 == s[f]).all()
        assert words.shape[0] in (0, 2 ** (13 - 6))  # rank 6: a coset of the code, or nothing
        solved, kept = osd.solved_set_by_rank(m, osd.order_of(q[f]))

        def only(flipped):
            want = z[f, kept].copy()
            want[list(flipped)] ^= 1
            x = words[(words[:, kept] == want).all(1)]
            assert x.shape[0] == 1
            return x[0], int(q[f][x[0] != z[f]].sum())

        for cap, depth in settings:
            r = {k: got[(cap, depth)][k][f] for k in osr.KEYS}
            word = gf2_ref.unpack(got[(cap, depth)]["word"][f:f + 1], code.nc)[0]
            if met or not words.shape[0]:
                status = osr.CODEWORD if met else osr.INFEASIBLE
                want = (z[f], 0, 0, [osr.NO_COLUMN] * 2, status)
            else:
                x0, metric0 = only(())
                flips = [(t,) for t in range(min(cap, len(kept)))]
                flips += [(t1, t2) for t1 in range(min(depth, len(kept))) for t2 in range(t1 + 1, min(depth, len(kept)))]
                best, tried = None, []
                for flipped in flips:  # in the order of e
                    x, metric = only(flipped)
                    tried.append((metric, flipped))
                    if best is None or metric < best[1]:
                        best = (x, metric, flipped)
                if best is not None and best[1] < metric0:
                    equal = [flipped for metric, flipped in tried if metric == best[1]]
                    assert equal[0] == best[2]
                    single_beats_equal_pair += len(equal[0]) == 1 and len(equal[-1]) == 2
                    first_of_equal_pairs += len(equal[0]) == 2 and len(equal) > 1
                    columns = [kept[t] for t in best[2]] + [osr.NO_COLUMN] * (2 - len(best[2]))
                    want = (best[0], int((best[0] != z[f]).sum()), best[1], columns, osr.REPROCESSED if len(best[2]) == 1 else osr.REPROCESSED_PAIR)
                else:
                    want = (x0, int((x0 != z[f]).sum()), metric0, [osr.NO_COLUMN] * 2, osr.ORDER0)
            assert np.array_equal(word, want[0]), (f, cap, depth)
            assert (r["flips"], r["metric"], r["flipped_columns"].tolist(), r["status"]) == want[1:], (f, cap, depth, r, want)
            seen.add(want[4])
    assert seen == {osr.CODEWORD, osr.ORDER0, osr.REPROCESSED, osr.REPROCESSED_PAIR, osr.INFEASIBLE}
    assert single_beats_equal_pair > 0 and first_of_equal_pairs > 0, (single_beats_equal_pair, first_of_equal_pairs)


def test_feasibility_is_the_column_space(files):
    """Infeasible iff no word has the syndrome, whatever the LLRs: on the tiny code (rank 6 of 7) and on a code of full rank."""
    code = gf2_ref.Gf2Code(*files["tiny"])
    m = osd.matrix(code)
    every = ((np.arange(2**code.nc)[:, None] >> np.arange(code.nc)[None, :]) & 1).astype(np.int64)
    reachable = set(map(bytes, ((every @ m.T.astype(np.int64)) & 1).astype(np.uint8)))
    assert len(reachable) == 2**6
    s = ((np.arange(2**code.mc)[:, None] >> np.arange(code.mc)[None, :]) & 1).astype(np.uint8)  # all 128 syndromes
    rng = np.random.default_rng(2)
    for llr in (rng.normal(0.5, 2.0, (128, code.nc)), np.ones((128, code.nc)), rng.integers(-1, 2, (128, code.nc)).astype(np.float64)):
        r = osr.decode(code, llr, s, 2, 3)
        assert np.array_equal(r["status"] == osr.INFEASIBLE, np.asarray([bytes(row) not in reachable for row in s]))
        assert (r["status"] == osr.INFEASIBLE).sum() == 64
        bad = r["status"] == osr.INFEASIBLE
        assert np.array_equal(r["word"][bad], gf2_ref.pack(osd.values(llr)[0])[bad]) and not r["metric"][bad].any() and not r["flips"][bad].any()
        assert (r["flipped_columns"][bad] == osr.NO_COLUMN).all()
    full = gf2_ref.Gf2Code(*files["s40x60"])
    assert len(osd.reduce(osd.matrix(full), np.arange(full.nc))[0]) == full.mc
    r = osr.decode(full, rng.normal(0.5, 2.0, (16, full.nc)), rng.integers(0, 2, (16, full.mc), dtype=np.uint8), 4, 4)
    assert not (r["status"] == osr.INFEASIBLE).any()


POINTS = {"s40x60": 3.0, "s40x60_hdup": 3.0, "s129x150t5": 3.0, "r240": 1.0}


@pytest.mark.parametrize("name", tuple(POINTS))
def test_identities_of_the_mirror(files, name):
    code = gf2_ref.Gf2Code(*files[name])
    m = osd.matrix(code)
    n = 20
    _, llr = plain._noisy(code, n, POINTS[name], 3, encoded=False)
    assert not (llr == 0).any() and not np.isnan(llr).any()
    rng = np.random.default_rng(4)
    u = rng.integers(0, 2, (n, code.nc), dtype=np.uint8)
    s = ((u.astype(np.int64) @ m.T.astype(np.int64)) & 1).astype(np.uint8)
    z, q = osd.values(llr)
    k = code.nc - len(osd.reduce(m, np.arange(code.nc))[0])
    settings = ((0, 0), (1, 0), (8, 0), (k + 50, 0), (0, 2), (0, 6), (8, 6), (8, 24), (k, 24))
    got = osr.decode_many(code, llr, s, settings)
    # 1. the syndrome of every word is s (s = M u: no frame is infeasible)
    for key, r in got.items():
        word = gf2_ref.unpack(r["word"], code.nc)
        assert not (r["status"] == osr.INFEASIBLE).any()
        assert np.array_equal(code.syndrome(word)[0], s) and not gf2_ref.high_bits(r["word"], code.nc).any(), (name, key)
        assert np.array_equal(r["flips"], (word != z).sum(1)) and np.array_equal(r["metric"], (q * (word != z)).sum(1).astype(np.uint64))
        assert np.array_equal(r["status"] == osr.REPROCESSED_PAIR, r["flipped_columns"][:, 1] != osr.NO_COLUMN)
        assert np.array_equal(r["status"] >= osr.REPROCESSED, r["flipped_columns"][:, 0] != osr.NO_COLUMN)
    # 2. the metric is non-increasing in candidates and in pair_depth
    for a, b in (((0, 0), (1, 0)), ((1, 0), (8, 0)), ((8, 0), (k + 50, 0)), ((0, 0), (0, 2)), ((0, 2), (0, 6)), ((0, 6), (8, 6)),
                 ((8, 0), (8, 6)), ((8, 6), (8, 24)), ((8, 24), (k, 24))):
        assert (got[b]["metric"] <= got[a]["metric"]).all(), (name, a, b)
    assert (got[(8, 24)]["metric"] < got[(8, 0)]["metric"]).any() and (got[(8, 24)]["status"] == osr.REPROCESSED_PAIR).any(), name
    # 3. no syndrome and no pairs: ldpc_hip_osd_batch
    for cap in (0, 1, 8, k + 50):
        a, b = osr.decode(code, llr, None, cap, 0), osd.decode(code, llr, cap)
        for key in ("word", "flips", "metric", "status"):
            assert np.array_equal(a[key], b[key]) and a[key].dtype == b[key].dtype, (name, cap, key)
        assert np.array_equal(a["flipped_columns"][:, 0], b["flipped_column"]) and (a["flipped_columns"][:, 1] == osr.NO_COLUMN).all()
    # 4. s = M u: the call is ldpc_hip_osd_batch on the LLRs with the signs flipped where u is 1, and u added to the word
    flipped = llr * (1.0 - 2.0 * u)
    for cap in (0, 1, 8, k + 50):
        a, b = got[(cap, 0)], osd.decode(code, flipped, cap)
        assert np.array_equal(a["word"], b["word"] ^ gf2_ref.pack(u)), (name, cap)
        for key in ("flips", "metric", "status"):
            assert np.array_equal(a[key], b[key]), (name, cap, key)
        assert np.array_equal(a["flipped_columns"][:, 0], b["flipped_column"])
