"""The code pairs of tests/generator_codes.py without a GPU: that they are what they claim to be (sizes, every row of G a
codeword under the oracle, the repeated entry without effect), that each lands on the encoder kernel and the decoder the GPU
tests mean it for (the library builds its plans on the host), and that the channel points of test_gpu_generator_codes.py give
the oracle — and the mirrors of the opt-in settings — both frames that converge on a non-zero codeword and frames that fail."""
import numpy as np
import pytest

import generator_codes as gc
import orc

LDS = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """name -> (h path, g path, oracle code with G)"""
    d = tmp_path_factory.mktemp("pairs")
    out = {}
    for name in list(gc.SYSTEMATIC) + list(gc.NULL_SPACE):
        h, g = gc.write_pair(d, name)
        out[name] = (h, g, orc.Code(h, g))
    return out


def test_every_pair_is_used():
    used = set(gc.ENCODER_PAIRS) | set(gc.COUNTER_PAIRS) | set(gc.SHARDED_PAIRS) | {v[0] for v in gc.DECODERS.values()}
    assert used == set(gc.SYSTEMATIC) | set(gc.NULL_SPACE)


@pytest.mark.parametrize("name", list(gc.SYSTEMATIC) + list(gc.NULL_SPACE))
def test_sizes_and_rows_of_g_are_codewords(pairs, name):
    _, _, c = pairs[name]
    if name in gc.SYSTEMATIC:
        args, (nc, mc, kc, g_rows, g_cols, _) = gc.SYSTEMATIC[name]
        assert (c.nc, c.mc, c.kc, c.g_rows, c.g_cols) == (nc, mc, kc, g_rows, g_cols)
        assert c.num_shorten == args.get("tail", 0) and c.nct == nc - c.num_shorten
        assert c.g_nnz == c.nnz - 2 * c.num_shorten + args["k"] - mc + 2 * bool(args.get("duplicate"))  # k + |A| entries
        present = np.arange(c.g_rows)
    else:
        args, (nc, mc, kc, g_rows, _) = gc.NULL_SPACE[name]
        assert (c.nc, c.mc, c.kc, c.g_rows) == (nc, mc, kc, g_rows) and c.g_cols <= nc
        present = np.linspace(0, kc - 1, args["n_rows"]).astype(np.int64)
        assert c.max_degree == args["dc"] and np.bincount(c.edge_col, minlength=nc).min() == args["dv"]  # no leaf
    assert c.has_G and c.g_rows <= c.kc and c.g_cols <= c.nc
    word, info = np.zeros(c.nc, np.uint8), np.zeros(c.g_rows, np.uint8)
    nonzero = 0
    for i in range(c.g_rows):
        info[:] = 0
        info[i] = 1
        word[:c.g_cols] = c.encode(info)
        assert not c.syndrome(word).any(), (name, i)
        nonzero += bool(word.any())
    assert nonzero == len(present)
    info[:] = 0
    info[present] = 1
    assert c.encode(info).any()  # (and the rows named are the non-zero ones)
    # a random combination too, in the shape the channel uses it
    u = (np.random.default_rng(1).random(c.g_rows) < 0.5).astype(np.uint8)
    word[:c.g_cols] = c.encode(u)
    assert word.any() and not c.syndrome(word).any()


def test_repeated_entry_encodes_as_if_absent(pairs):
    plain, dup = pairs["s40x60"][2], pairs["s40x60_dup"][2]
    assert dup.g_nnz == plain.g_nnz + 2 and np.array_equal(dup.edge_row, plain.edge_row) and np.array_equal(dup.edge_col, plain.edge_col)
    rng = np.random.default_rng(2)
    for _ in range(50):
        u = (rng.random(plain.g_rows) < 0.5).astype(np.uint8)
        assert np.array_equal(dup.encode(u), plain.encode(u))
    a = plain.run_frames("AWGN", 3.0, seed=gc.SEED, count=40, iters=0, math=orc.MATH_DET)["codeword"]
    b = dup.run_frames("AWGN", 3.0, seed=gc.SEED, count=40, iters=0, math=orc.MATH_DET)["codeword"]
    assert np.array_equal(a, b) and a.any(axis=1).mean() > 0.9


def test_encoder_paths(pairs):
    """The rule of launch_encode_codewords restated from sizes alone: each pair takes the kernel it is listed for, and the
    listed pairs reach every dense width, the walk by nc alone, by kc alone and with a narrow G."""
    seen = {}
    for name, (_, _, c) in pairs.items():
        want = (gc.SYSTEMATIC.get(name) or gc.NULL_SPACE[name])[1][-1]
        assert gc.encoder_path(c.nc, c.kc, c.g_rows) == want, name
        seen[name] = want
    enc = [seen[n] for n in gc.ENCODER_PAIRS]
    assert enc == ["dense1", "dense1", "dense3", "dense4", "walk", "walk", "walk", "dense1"]
    c = {n: pairs[n][2] for n in gc.ENCODER_PAIRS}
    assert c["s40x60"].kc % 64 == 40 and c["s40x60"].nc < 256 and c["s64x100"].kc == 64
    assert c["s129x150t5"].kc == 134 == 2 * 64 + 6 and c["s129x150t5"].g_rows < c["s129x150t5"].kc and c["s129x150t5"].g_cols < c["s129x150t5"].nc
    assert c["s256x1792"].nc == 2048 and c["s256x1792"].kc == 256
    assert c["s200x1849"].nc == 2049 and (c["s200x1849"].kc + 63) // 64 == 4 and c["s200x1849"].kc % 64 != 0  # the walk by nc alone
    assert (c["s257x200"].kc + 63) // 64 == 5 and c["s257x200"].nc <= 2048                                       # by kc alone
    assert (c["s300x250t3"].kc + 63) // 64 == 5 and c["s300x250t3"].g_cols < c["s300x250t3"].nc
    assert [seen[n] for n in gc.COUNTER_PAIRS] == ["dense1", "dense3", "walk"]
    assert [seen[n] for n in gc.SHARDED_PAIRS] == ["walk", "dense3"]


def _bec_sliced(c):
    """bec_sliced_fits (kernels_bec.hip) from sizes alone: 10 nnz + 16 nc + 16 bytes within 160 KiB - 1 KiB, fewer than 65 536
    edges, at most 512 check-node blocks and 128 variable-node blocks (blocks: up to 64 nodes of one degree, plan.cpp)."""
    blocks = lambda deg: int(((np.bincount(deg) + 63) // 64).sum())
    cn = blocks(np.bincount(c.edge_row, minlength=c.mc))
    vn = blocks(np.bincount(c.edge_col, minlength=c.nc))
    return 10 * c.nnz + 16 * c.nc + 16 <= LDS - 1024 and len(c.bit_pos) <= c.nnz and 0 < c.nnz < 65536 and cn <= 512 and 4 * vn <= 512


@pytest.mark.parametrize("residency", list(gc.DECODERS))
def test_decoder_paths(lib, pairs, residency):
    import libldpc_amd
    name, form, fused, sliced = gc.DECODERS[residency]
    h, g, c = pairs[name]
    d = libldpc_amd.HipDecoder(h, g)
    assert (d.nc, d.mc, d.nnz, d.kc, d.nct) == (c.nc, c.mc, c.nnz, c.kc, c.nct)
    assert d.residency == residency.split("_")[0] and d.register_form == form, (d.residency, d.register_form)
    assert bool(d.fused_plan()["ok"]) == fused
    assert _bec_sliced(c) == sliced
    for dec in ("BP", "BP_MS"):
        assert d.decoder_choice(True, 50, dec) == "resident"
    for setting, (_, takes) in gc.OPT_IN.items():
        if residency in takes:
            gc.switch_on(d, setting)
            assert d.decoder_choice(True, gc.OPT_IN_ITERATIONS, "BP_MS") == {"corrected": "resident", "layered": "layered-min-sum",
                                                                              "quantized": "quantized-min-sum", "ternary": "ternary"}[setting]
        else:
            with pytest.raises(RuntimeError):
                gc.switch_on(d, setting)
        gc.switch_off(d)


def test_register_mailbox_fits_beside_the_static_lds(lib, pairs):
    """The messages-form register kernels ask for 9 bytes per mailbox entry of dynamic LDS beside their static LDS.
    build_reg_plan (plan.cpp) restated from the column degrees: blocks of up to 64 columns of one degree, degrees descending,
    fill a round of at most cap = ((160 KiB - 512) / 9 rounded down to 64) entries; the mailbox is the fullest round rounded
    up to 64.  The s6000x3600 pair fills the mailbox to the cap itself — with 256 bytes left for the static LDS instead of
    512 that was 16 bytes more than a CU has, and no launch of the pair succeeded."""
    from libldpc_amd import build
    res = build.kernel_resources("kernels_reg.hip")
    static = max(v["LDS Size [bytes/block]"] for k, v in res.items() if "decode_reg" in k)
    assert 0 < static <= 512, static
    c = pairs[gc.DECODERS["registers_messages"][0]][2]
    cap = ((LDS - 512) // 9) & ~63
    fill = peak = 0
    for d, count in sorted(enumerate(np.bincount(np.bincount(c.edge_col, minlength=c.nc))), reverse=True):
        for need in [64 * d] * (count // 64) + [count % 64 * d] * bool(count % 64):
            fill = need if fill + need > cap else fill + need
            peak = max(peak, fill)
    entries = (peak + 63) & ~63
    assert entries == cap == 18112
    assert 9 * entries + static <= LDS


@pytest.mark.parametrize("residency", list(gc.DECODERS))
def test_channel_points_give_converged_and_failed_frames(pairs, residency):
    c = pairs[gc.DECODERS[residency][0]][2]
    for case, (ch, dec, early, iters, compat) in gc.CASES.items():
        x = gc.POINTS[residency][case]
        o = c.run_frames(ch, x, seed=gc.SEED, skip=gc.SKIP, count=gc.FRAMES, min_sum=dec == "BP_MS", early_term=early, iters=iters,
                         math=orc.MATH_DET, bec_compat=compat)
        print(residency, case, x, "converged / failed / non-zero:", gc.check_mixed(o["iters"], o["bit_errors"], o["codeword"], early, iters, case))
        tx = np.asarray(c.bit_pos)
        assert np.array_equal(o["bit_errors"], (o["hard"][:, tx] != o["codeword"][:, tx]).sum(1))
        assert not o["codeword"][:, c.g_cols:].any()
    for setting, (ch, takes) in gc.OPT_IN.items():
        if residency not in takes:
            assert setting not in gc.POINTS[residency]
            continue
        x = gc.POINTS[residency][setting]
        o = c.run_frames(ch, x, seed=gc.SEED, skip=gc.SKIP, count=gc.FRAMES, iters=0, math=orc.MATH_DET)
        m = gc.mirror_decode(c, setting, o["llr_in"], o["codeword"])
        print(residency, setting, x, "converged / failed / non-zero:",
              gc.check_mixed(m["iters"], m["bit_errors"], o["codeword"], True, gc.OPT_IN_ITERATIONS, setting))
