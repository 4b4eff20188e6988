"""The simulation loop's counters, stop rule and report (libldpc_amd/csrc/sim_fold.hpp) without a GPU: the functions the two
drivers of sim.cpp call, run over given per-frame results through ldpc_hip_selftest_sim_fold, against a restatement of the
reference's loop (src/sim/ldpcsim.cpp:175-255), for every way of cutting the frames into batches and ranks' ranges."""
import itertools

import numpy as np
import pytest

N = 3000
MIN_FEC = (0, 1, 2, 50)
WORLDS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def fold():
    from libldpc_amd import binding, build
    build.build()
    return binding.sim_fold


def reference_loop(iters, bit_errors, min_fec, max_frames):
    """ldpc_sim::start's do-while over the given frames, one thread, the stop flag down.  Returns ([frames, fec, bec, iters,
    frames at the last report, iterations at the last report, the rule fired], frames consumed)."""
    frames = fec = bec = it_sum = rep_frames = rep_iters = i = 0
    while i < len(iters):  # (an array that runs out before the rule fires: the loop is still going)
        it_sum += int(iters[i])  # :176
        if fec < min_fec:  # :178
            frames += 1
            if bit_errors[i] > 0:  # :190
                bec += int(bit_errors[i])
                fec += 1
                rep_frames, rep_iters = frames, it_sum  # :202-248, the values the report is made of
        i += 1
        if not (fec < min_fec and frames < max_frames):  # :255
            return [frames, fec, bec, it_sum, rep_frames, rep_iters, 1], i
    return [frames, fec, bec, it_sum, rep_frames, rep_iters, 0], i


def streams():
    """Seeded per-frame results with frame-error densities from 0 to 1."""
    rng = np.random.default_rng(20240607)
    out = []
    for density in (0.0, 0.004, 0.05, 0.5, 1.0):
        it = rng.integers(1, 51, N).astype(np.uint32)
        be = np.where(rng.random(N) < density, rng.integers(1, 300, N), 0).astype(np.uint32)
        out.append((it, be))
    return out


def pad(ends, world):
    """Whole steps: trailing ranks without frames fill the last one."""
    ends = [int(e) for e in ends]
    return ends + [ends[-1]] * (-len(ends) % world)


def cuts(world, consumed, rng):
    """Ways of presenting frames [0, N) as ranges, `world` to a step; `consumed` is where the reference's loop stops."""
    c = consumed
    a, b = sorted(int(v) for v in rng.integers(1, N, 2))
    yield pad([N], world)  # one range (world > 1: the other ranks' ranges are empty, trailing)
    yield pad(range(1, N + 1), world)  # single-frame ranges
    yield pad(np.append(np.sort(rng.integers(0, N + 1, 40)), N), world)  # random, with empty ranges wherever they fall
    yield pad(np.append(np.sort(rng.choice([0, a, b, c], 30)), N), world)  # mostly empty ranges
    yield pad([c, N], world)  # a range, a batch or a step, ends exactly on the stopping frame
    yield [c // 2] * (world - 1) + [c] + pad([N], world)  # ... as the last rank of its step
    yield [0] * (world - 1) + [N]  # leading ranks empty
    yield [0] * world + [0] * (world - 1) + [a] + pad([N], world)  # a whole step empty, then leading ranks empty
    if world > 2:
        yield [a] + [a] * (world - 2) + [b] + [b] + [b] * (world - 2) + [N]  # middle ranks empty
        yield [0] + [c] * (world - 1) + [c] * (world - 1) + [N]  # the stopping frame before empty middle and trailing ranks


def expected_step(ends, world, consumed, fired):
    """(steps walked, frames consumed of the last step walked) for the reference's loop over these steps."""
    step_end = ends[world - 1::world]
    step_begin = [0] + step_end[:-1]
    if not fired:
        return len(step_end), step_end[-1] - step_begin[-1]
    s = next(k for k in range(len(step_end)) if step_begin[k] < consumed <= step_end[k])
    return s + 1, consumed - step_begin[s]


def max_frames_cases(it, be, min_fec):
    inside = reference_loop(it, be, min_fec, 10**10)[1] // 2 + 1  # (before the frame-error rule alone would stop)
    return (0, 1, inside, N + 1000)


def test_counters_equal_the_reference_loop_for_every_cut(fold):
    rng = np.random.default_rng(7)
    checked = 0
    for (it, be), min_fec in itertools.product(streams(), MIN_FEC):
        for max_frames in max_frames_cases(it, be, min_fec):
            want, consumed = reference_loop(it, be, min_fec, max_frames)
            for world in WORLDS:
                for ends in cuts(world, consumed, rng):
                    steps, got = fold(it, be, ends, world, min_fec, max_frames)
                    what = (min_fec, max_frames, world, ends[:12], consumed)
                    assert got[:7] == want, what
                    assert (steps, got[7]) == expected_step(ends, world, consumed, want[6]), what
                    checked += 1
    assert checked > 2000


def test_split_invariance(fold):
    """One stream, one rule: no cut into batches and no number of ranks changes a counter, the report or the stop."""
    rng = np.random.default_rng(11)
    it, be = streams()[2]
    for min_fec, max_frames in ((50, 10**10), (50, 700), (2, 10**10), (0, 10**10), (50, 0), (10**6, 10**10)):
        consumed = reference_loop(it, be, min_fec, max_frames)[1]
        seen = {tuple(fold(it, be, ends, world, min_fec, max_frames)[1][:7]) for world in WORLDS for ends in cuts(world, consumed, rng)}
        assert len(seen) == 1, (min_fec, max_frames, seen)


@pytest.mark.parametrize("world", (1, 2))
def test_reference_numbers_of_the_headline_stream(fold, golden_bulk, golden_sim, world):
    """The reference's own per-frame counters (AWGN -4 dB, seed 0) in 4096-frame steps: its totals, and the result-file line
    of its CLI run with --max-frames 2000."""
    it, be = golden_bulk["iters"], golden_bulk["bit_errors"]
    n = len(it)
    ends = sorted(set(range(4096 // world, n, 4096 // world)) | {n})
    ends += [n] * (-len(ends) % world)
    steps, out = fold(it, be, ends, world, 50, 2000)
    assert out[:7] == [2000, 2, 299, 25920, 1962, 25448, 1] and (steps, out[7]) == (1, 2000)
    frames, fec, bec, iters, rep_frames, rep_iters = out[:6]
    line = "%f %.3e %.3e %d %.3e" % (-4.0, fec / rep_frames, bec / (rep_frames * 1152), rep_frames, rep_iters / rep_frames)
    assert line == golden_sim["cli"]["awgn_bp"]["lines"][1] == "-4.000000 1.019e-03 1.323e-04 1962 1.297e+01"
    steps, out = fold(it, be, ends, world, 50, 10**10)
    assert out[:4] == [40108, 50, 10932, 517402] and out[6] == 1
    assert out[4] == 40108 and (steps, out[7]) == (40108 // 4096 + 1, 40108 % 4096)  # (the 50th frame error stops the loop)
    assert out[:7] == reference_loop(it, be, 50, 10**10)[0]


def test_bad_arguments(fold):
    it, be = streams()[1]
    assert fold(it, be, [10, 5, N], 1)[0] == -1  # ends not ascending
    assert fold(it, be, [10, N + 1], 1)[0] == -1  # beyond the frames given
    assert fold(it, be, [10, 20, N], 2)[0] == -1  # not whole steps
    assert fold(it, be, [N], 0)[0] == -1 and fold(it, be, [N], -1)[0] == -1
    assert fold(it, be, [N], 1)[0] == 1
