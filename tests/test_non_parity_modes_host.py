"""The non-parity sum-product modes (ldpc_hip_set_fast_mode 1 / 2 / 3) without a GPU: the four codes of non_parity_codes.py
are what that module says they are and the library loads them, the layered plan of each equals the oracle's restatement row
for row, every mode runs them in one launch, and the yardstick that test_gpu_non_parity_modes.py takes its tolerances from
(the mirror against itself on inputs moved by 2e-7) leaves those tolerances with something to say."""
import numpy as np
import pytest

import non_parity_codes as npc
import orc


@pytest.fixture(scope="module")
def codes(tmp_path_factory):
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    paths = npc.write_codes(tmp_path_factory.mktemp("non_parity"), npc.NAMES + npc.VN_NAMES)
    return {name: (path, orc.Code(path), libldpc_amd.HipDecoder(path)) for name, path in paths.items()}


@pytest.fixture(scope="module")
def inputs(codes):
    return {(name, ch): npc.reference_inputs(codes[name][1], name, ch) for name in npc.NAMES + npc.VN_NAMES
            for ch, _ in npc.CHANNELS[name]}


def _histogram(values):
    return dict(zip(*(a.tolist() for a in np.unique(values, return_counts=True))))


def test_codes_are_what_the_module_says(codes):
    """Degree histograms, punctured and shortened columns, sizes; the library loads each (host only) as an LDS-resident code."""
    shape = {"np_mix": (790, 535, 2600), "np_r36": (576, 288, 1728), "np_r48": (500, 250, 2000), "np_r37": (490, 210, 1470)}
    for name in npc.NAMES:
        path, code, d = codes[name]
        vn, cn, _ = npc.CODES[name]
        assert (code.nc, code.mc, code.nnz) == shape[name] == (d.nc, d.mc, d.nnz), name
        # make_code_by_degrees hands the degrees out in the order given: column c has degree vn[c], row r degree cn[r]
        assert np.array_equal(np.bincount(code.edge_col, minlength=code.nc), vn), name
        assert np.array_equal(np.bincount(code.edge_row, minlength=code.mc), cn), name
        assert len(set(zip(code.edge_row.tolist(), code.edge_col.tolist()))) == code.nnz, name  # no edge twice
        assert d.residency == "lds", (name, d.residency)
    _, mix, _ = codes["np_mix"]
    assert _histogram(np.bincount(mix.edge_col)) == {1: 70, 2: 200, 3: 330, 4: 100, 6: 50, 9: 30, 17: 10}
    assert _histogram(np.bincount(mix.edge_row)) == {2: 50, 3: 100, 4: 100, 5: 80, 6: 100, 7: 40, 8: 65}
    assert mix.puncture.tolist() == [5, 300, 789] and mix.shorten.tolist() == [11, 640] and mix.nct == 785
    assert mix.nc % 4 and mix.nc % 64
    for name, (dv, dc) in (("np_r36", (3, 6)), ("np_r48", (4, 8)), ("np_r37", (3, 7))):
        _, code, _ = codes[name]
        assert _histogram(np.bincount(code.edge_col)) == {dv: code.nc} and _histogram(np.bincount(code.edge_row)) == {dc: code.mc}
        assert code.num_puncture == code.num_shorten == 0


def test_variable_node_routines_reached():
    """What the module's docstring says about mode 1's variable-node routines, from the restated deal of plan.cpp."""
    waves, taken = npc.vn_paths(npc.CODES["np_mix"][0])
    assert waves == [[17, 2], [9, 3, 3, 2], [6, 3, 3, 2, 2], [4, 4, 3, 3, 1, 1]]
    assert taken == {("vn_fast_any", "loop"), ("vn_fast_wide", 9), ("vn_fast_wide", 6), ("vn_fast_wide", 4), ("vn_fast_any", 4),
                     ("vn_fast_any", 3), ("vn_fast", 2), ("vn_fast", 1)}
    for name, blocks, deg in (("np_r36", 9, 3), ("np_r48", 8, 4), ("np_r37", 8, 3)):
        waves, taken = npc.vn_paths(npc.CODES[name][0])
        assert sum(map(len, waves)) == blocks and max(map(len, waves)) <= 8, name
        assert taken == {("vn_fast_wide", deg), ("vn_fast_any", deg)}, name
    # the four codes more: the four widest degrees first in the four waves, and with np_mix every case of both switches
    firsts = {"np_vn16": [16, 15, 14, 13], "np_vn20": [20, 19, 18, 17], "np_vn12": [12, 11, 10, 8], "np_vn7": [7, 5, 4, 3]}
    union = set(npc.vn_paths(npc.CODES["np_mix"][0])[1])
    for name in npc.VN_NAMES:
        waves, taken = npc.vn_paths(npc.VN_CODES[name][0])
        assert [w[0] for w in waves] == firsts[name] and max(map(len, waves)) <= 8, (name, waves)
        union |= taken
    assert union >= {(routine, d) for routine in ("vn_fast_wide", "vn_fast_any") for d in range(3, 17)} | {("vn_fast_any", "loop")}


def test_variable_node_codes_load_and_have_a_yardstick(codes, inputs):
    """The four codes for mode 1's variable-node switches: as described, LDS-resident, taken by mode 1 in one launch; the
    yardstick of their fixed sweeps is there and small, leaves out next to nothing, and flips nothing outside that."""
    for name in npc.VN_NAMES:
        _, code, d = codes[name]
        vn, cn, _ = npc.VN_CODES[name]
        assert np.array_equal(np.bincount(code.edge_col, minlength=code.nc), vn) and set(np.bincount(code.edge_row).tolist()) == {8}
        assert (code.nc, code.mc, code.nnz) == (len(vn), len(cn), sum(vn)) == (d.nc, d.mc, d.nnz) and d.residency == "lds", name
        assert len(set(zip(code.edge_row.tolist(), code.edge_col.tolist()))) == code.nnz, name
        d.set_fast_mode(1)
        assert d.decode_stages(False, 3, "BP") == ["whole"] and d.decoder_choice(False, 3, "BP") == "fast32", name
        d.set_fast_mode(0)
        for iters in npc.SWEEPS:
            s = npc.Sweeps(code, 1, inputs[(name, "AWGN")], iters)
            assert 0.0 < s.yard < 2e-5 and s.left_out < 0.00215 and s.yard_flips_outside == 0, (name, iters, s.yard, s.left_out)
            assert s.hard.any() and not s.hard.all(), (name, iters)


def test_layer_plans_match_the_restatement(codes):
    """ldpc_hip_selftest_layer_plan == orc.Code.layer_steps() row for row on all four codes; np_mix: more than 20 steps in
    seven degree classes, several of them partly filled (the step tables of kernels_layered.hip beyond h.txt's two classes
    of full and quarter-filled steps)."""
    for name in npc.NAMES:
        _, code, d = codes[name]
        mine = np.full(code.mc, -1, np.int32)
        n = d.lib.ldpc_hip_selftest_layer_plan(d.ctx, mine.ctypes.data)
        n_ref, ref = code.layer_steps()
        assert n == n_ref > 0 and np.array_equal(mine, ref), name
        counts = np.bincount(ref, minlength=n)
        degree = np.bincount(code.edge_row, minlength=code.mc)
        for s in range(n):  # a step holds rows of one degree that share no column, at most 64
            rows = np.flatnonzero(ref == s)
            cols = code.edge_col[np.isin(code.edge_row, rows)]
            assert 0 < rows.size <= 64 and len(set(degree[rows].tolist())) == 1 and len(set(cols.tolist())) == cols.size, (name, s)
        if name == "np_mix":
            classes = {int(degree[np.flatnonzero(ref == s)[0]]) for s in range(n)}
            assert n > 20 and classes == set(range(2, 9)) and (counts < 64).sum() >= 7 and (counts % 2 == 1).any(), (n, counts.tolist())


def test_one_launch_and_the_decoder_named(codes):
    for name in npc.NAMES:
        _, _, d = codes[name]
        for mode in npc.MODES:
            d.set_fast_mode(mode)
            for early in (True, False):
                for iters in (30, 3, 0):
                    assert d.decode_stages(early, iters, "BP") == ["whole"], (name, mode, early, iters)
                    assert d.decoder_choice(early, iters, "BP") == npc.DECODER[mode], (name, mode, early, iters)
            assert d.decoder_choice(True, 30, "BP_MS") == "resident", (name, mode)  # min-sum ignores the mode
        d.set_fast_mode(0)
        assert d.decoder_choice() == "resident", name


@pytest.mark.parametrize("mode", npc.MODES)
@pytest.mark.parametrize("name", npc.NAMES)
def test_yardstick_of_the_fixed_sweeps(codes, inputs, name, mode):
    """A: for 1, 2 and 3 sweeps the mirror's own deviation under the perturbation is there (not zero: the margin multiplies
    something) and small against a structural error (deviations of order 1): below 2e-5 with binary32 messages, below 1e-2 with
    binary16 ones (measured: 1.3e-6 .. 1.6e-5 and 5.5e-4 .. 4.1e-3).  The decisions the GPU test leaves out of its comparison —
    where the mirror's |llr_out| is within 16 x the yardstick — may be 1 % of a run's elements there; the yardstick leaves out
    0.21 % at the most (np_r37, AWGN, mode 3, one sweep: 527 of 250 880), and no decision that the perturbation flips lies
    outside the set left out (np_mix on the BSC, mode 1, one sweep: 77 flips, all of them inside)."""
    code = codes[name][1]
    for ch, _ in npc.CHANNELS[name]:
        for iters in npc.SWEEPS:
            s = npc.Sweeps(code, mode, inputs[(name, ch)], iters)
            what = (name, mode, ch, iters)
            assert 0.0 < s.yard < (1e-2 if mode == 3 else 2e-5), (what, s.yard)
            assert s.left_out < 0.00215, (what, s.left_out)  # (0.21 % to the digits it is stated in; the GPU test allows 1 %)
            assert s.yard_flips_outside == 0, (what, s.yard_flips_outside)
            assert not np.isnan(s.llr).any() and s.hard.any() and not s.hard.all(), what


@pytest.mark.parametrize("mode", npc.MODES)
@pytest.mark.parametrize("name", npc.NAMES)
def test_yardstick_of_the_whole_decodes(codes, inputs, name, mode):
    """B: with early termination and 30 iterations the perturbation alone changes the count or a decision of at most 8 frames
    of 512 (measured: 5 at the most, np_r37, AWGN, mode 3) — except where the mirror's own totals hold exact zeros: np_mix on
    the BSC in modes 1 and 2, 49 frames (non_parity_codes.py, Whole, says why).  Among the frames in which no |llr_out| of the
    mirror is within the bound, which the GPU test counts a second time, it is at most 8 everywhere, and outside mode 3, whose
    bound is wide, those are most frames.  Most frames converge (the GPU test's LLR comparison has frames to look at), and
    not all in the same sweep."""
    code = codes[name][1]
    for ch, _ in npc.CHANNELS[name]:
        w = npc.Whole(code, mode, inputs[(name, ch)])
        what = (name, mode, ch)
        print(what, "disagree", w.yard_disagree, "clear frames", int(w.clear.sum()), "of them disagree", w.yard_disagree_clear)
        assert w.yard_disagree_clear <= 8, (what, w.yard_disagree_clear)
        assert w.yard_disagree <= 8 or w.ties, (what, w.yard_disagree)
        assert w.ties == (name == "np_mix" and ch == "BSC" and mode != 3), what
        assert mode == 3 or w.clear.sum() > 0.75 * npc.FRAMES, (what, int(w.clear.sum()))
        assert w.yard_frames > npc.FRAMES // 2 and w.yard > 0.0, (what, w.yard_frames, w.yard)
        assert len(set(w.it.tolist())) >= 3, (what, sorted(set(w.it.tolist())))
