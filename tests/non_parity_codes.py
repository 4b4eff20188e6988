"""What the tests of the three opt-in NON-PARITY sum-product modes (ldpc_hip_set_fast_mode 1 / 2 / 3: kernels_fast.hip,
kernels_layered.hip) share: four small codes that reach the kernel paths h.txt does not, the inputs, the mirror's own
sensitivity (the yardstick every tolerance is taken from) and the comparisons.  A plain module, like orc.py and
minsum_common.py; test_non_parity_modes_host.py checks on the CPU what is said here, test_gpu_non_parity_modes.py uses it.

The codes (make_code_by_degrees of test_gpu_random_codes.py, seeded with crc32 of the name):

  np_mix  790 x 535, 2600 edges; column degrees 1 (70), 2 (200), 3 (330), 4 (100), 6 (50), 9 (30), 17 (10); every check degree
          2..8 (50, 100, 100, 80, 100, 40, 65 rows); columns 5, 300, 789 punctured, 11 and 640 shortened; nc is no multiple of
          4 or of 64
  np_r36  (3,6)-regular, 576 x 288      np_r48  (4,8)-regular, 500 x 250      np_r37  (3,7)-regular, 490 x 210

Check nodes: cn_fast<D> (mode 1), cn_layered<D, float> / <D, _Float16> (modes 2 / 3) and cn_parity<D> (modes 2 / 3 with early
termination) run for D = 2..8 on np_mix — D = 2 is the special case without forward / backward recursion — and for D = 6, 8, 7
on np_r36, np_r48, np_r37.  The layered step table of np_mix has seven degree classes and partly filled steps (HOST test 2).

Variable nodes of mode 1 (plan.cpp, build_plan: blocks of up to 64 nodes of one degree, sorted by degree descending, dealt by
cost 2 d + 2 to the least loaded of four waves; kernels_fast.hip: a wave's FIRST block of degree 3..16 keeps its slot
indices packed in registers, vn_fast_wide; degrees 1 and 2 ride in one register, vn_fast<1> / vn_fast<2>; every other block
goes through the slot table, vn_fast_any) — restated by vn_paths() below:

  np_mix  wave 0: [17, 2]  wave 1: [9, 3, 3, 2]  wave 2: [6, 3, 3, 2, 2]  wave 3: [4, 4, 3, 3, 1, 1]
          -> the generic loop of vn_fast_any (degree 17 > 16, although first in its wave), vn_fast_wide 9, 6 and 4,
             vn_fast_any 4 and 3, vn_fast<2>, vn_fast<1>
  np_r36  nine blocks of degree 3 (wave 0 takes three): vn_fast_wide 3, vn_fast_any 3
  np_r48  eight blocks of degree 4: vn_fast_wide 4, vn_fast_any 4         np_r37  eight blocks of degree 3: as np_r36
The other cases of the two switches (vn_fast_wide and vn_fast_any, degrees 3..16 each) are reached by four codes more, which only
mode 1's fixed sweeps run — eight columns of each degree named, padded with columns of degree 2 (np_vn7: and 1), every check node
of degree 8; the four widest degrees come first in the four waves:

  np_vn16  280 x 161: vn_fast_wide 16, 15, 14, 13; vn_fast_any 12, 11, 10, 8, 7, 5
  np_vn20  340 x 212: the generic loop 20, 19, 18, 17; vn_fast_any 16, 15, 14, 13, 9, 6
  np_vn12  128 x 65:  vn_fast_wide 12, 11, 10, 8           np_vn7  80 x 30: vn_fast_wide 7, 5, 4, 3

Together: every case 3..16 of both switches and the loop (cases 1 and 2 of vn_fast_any cannot be reached: such blocks never get there).
"""
import os
import zlib

import numpy as np

import orc
from test_gpu_random_codes import make_code_by_degrees

CODES = {
    # name: (column degrees, row degrees, lines in front)
    "np_mix": ([1] * 70 + [2] * 200 + [3] * 330 + [4] * 100 + [6] * 50 + [9] * 30 + [17] * 10,
               [2] * 50 + [3] * 100 + [4] * 100 + [5] * 80 + [6] * 100 + [7] * 40 + [8] * 65,
               "puncture [3]: 5 300 789\nshorten [2]: 11 640\n"),
    "np_r36": ([3] * 576, [6] * 288, ""),
    "np_r48": ([4] * 500, [8] * 250, ""),
    "np_r37": ([3] * 490, [7] * 210, ""),
}
NAMES = tuple(CODES)


def _vn_code(degrees, pad):
    vn = [d for d in degrees for _ in range(8)] + pad
    assert sum(vn) % 8 == 0
    return vn, [8] * (sum(vn) // 8), ""


# the codes for the variable-node switches of mode 1 (the docstring above)
VN_CODES = {
    "np_vn16": _vn_code([16, 15, 14, 13, 12, 11, 10, 8, 7, 5], [2] * 200),
    "np_vn20": _vn_code([20, 19, 18, 17, 16, 15, 14, 13, 9, 6], [2] * 260),
    "np_vn12": _vn_code([12, 11, 10, 8], [2] * 96),
    "np_vn7": _vn_code([7, 5, 4, 3], [2] * 40 + [1] * 8),
}
VN_NAMES = tuple(VN_CODES)
MODES = (1, 2, 3)
DECODER = {1: "fast32", 2: "layered32", 3: "layered16"}
SEED, FRAMES = 7, 512
# channel points of the inputs: np_mix at 5.0 dB only (at 8 dB its punctured columns leave totals at exactly zero)
CHANNELS = {name: (("AWGN", 5.0 if name == "np_mix" else 3.0), ("BSC", 0.03)) for name in NAMES}
CHANNELS.update({name: (("AWGN", 3.0),) for name in VN_NAMES})
SWEEPS = (1, 2, 3)        # A: fixed sweeps without early termination
WHOLE_ITERATIONS = 30     # B: whole decodes with early termination
MARGIN = 16               # A: bound = MARGIN x the yardstick's largest deviation (see test_gpu_non_parity_modes.py)


def write_code(name, directory):
    vn, cn, front = CODES[name] if name in CODES else VN_CODES[name]
    path = os.path.join(str(directory), name + ".txt")
    make_code_by_degrees(path, vn, cn, np.random.default_rng(zlib.crc32(name.encode())))
    if front:
        body = open(path).read()
        open(path, "w").write(front + body)
    return path


def write_codes(directory, names=NAMES):
    """The four codes (or those of `names`) as files in `directory`: {name: path}."""
    return {name: write_code(name, directory) for name in names}


def vn_paths(col_degrees):
    """Which variable-node routine of kernels_fast.hip a code's blocks take, restated from plan.cpp (build_plan, deal):
    (per wave the degrees of its blocks in order, the set of (routine, degree))."""
    degs = sorted(col_degrees, reverse=True)
    blocks = []
    for d in sorted(set(degs), reverse=True):
        n = degs.count(d)
        blocks += [d] * ((n + 63) // 64)
    waves, load = [[] for _ in range(4)], [0] * 4
    for d in blocks:  # (already in descending cost 2 d + 2; ties keep their order)
        w = load.index(min(load))
        waves[w].append(d)
        load[w] += 2 * d + 2
    taken = set()
    for blks in waves:
        for i, d in enumerate(blks):
            if d <= 2:
                taken.add(("vn_fast", d))
            elif i == 0 and d <= 16:
                taken.add(("vn_fast_wide", d))
            else:
                taken.add(("vn_fast_any", d if d <= 16 else "loop"))
    return waves, taken


def reference_inputs(code, name, ch):
    """llr_in of the FRAMES frames of the reference stream the tests decode, from the CPU oracle (what the GPU dumps, bit for
    bit: test_gpu_non_parity_modes.py checks that on np_mix)."""
    x = dict(CHANNELS[name])[ch]
    return code.run_frames(ch, x, seed=SEED, count=FRAMES, iters=0, math=orc.MATH_DET)["llr_in"]


def yardstick_inputs(llr):
    """The inputs moved by a few units of binary32's last place: llr * (1 + 2e-7 u), u uniform in (-1, 1) — the perturbation
    test_non_parity_modes_against_their_mirror cites.  The mirror on these against the mirror on llr is the yardstick."""
    u = np.random.default_rng(1).uniform(-1.0, 1.0, llr.shape)
    return llr * (1.0 + 2e-7 * u)


def deviation(a, b):
    """|a - b| / max(|a|, 1), element by element; a is the mirror's llr_out."""
    return np.abs(a - b) / np.maximum(np.abs(a), 1.0)


class Sweeps:
    """A: the mirror after `iters` sweeps without early termination, and its yardstick."""

    def __init__(self, code, mode, llr, iters):
        self.iters = iters
        self.it, self.llr, self.hard = code.decode_fast(mode, llr, early_term=False, iters=iters)
        _, self.y_llr, self.y_hard = code.decode_fast(mode, yardstick_inputs(llr), early_term=False, iters=iters)
        self.yard = float(deviation(self.llr, self.y_llr).max())
        self.bound = MARGIN * self.yard
        self.compared = np.abs(self.llr) > self.bound  # where a decision is compared: the mirror's LLR is beyond the bound
        self.left_out = float(1.0 - self.compared.mean())
        self.yard_flips_outside = int(((self.hard != self.y_hard) & self.compared).sum())

    def check(self, got, what):
        """Results `got` of the library against the mirror; returns the largest deviation as a multiple of the yardstick."""
        assert (got["iters"] == self.iters).all() and (self.it == self.iters).all(), what
        dev = float(deviation(self.llr, got["llr_out"]).max())
        multiple = dev / self.yard
        print(f"sweeps {what}: deviation {dev:.3e} = {multiple:.3f} x yardstick {self.yard:.3e}, left out {self.left_out:.5f}")
        assert dev <= self.bound, (what, dev, self.bound)
        assert np.array_equal(got["hard"][self.compared], self.hard[self.compared]), what
        assert self.left_out <= 0.01, (what, self.left_out)
        return multiple


class Whole:
    """B: the mirror's whole decodes with early termination, and its yardstick."""

    def __init__(self, code, mode, llr, iters=WHOLE_ITERATIONS):
        self.iters = iters
        self.it, self.llr, self.hard = code.decode_fast(mode, llr, early_term=True, iters=iters)
        y_it, y_llr, y_hard = code.decode_fast(mode, yardstick_inputs(llr), early_term=True, iters=iters)
        self.converged = self.it < iters
        agree = self.agree(y_it, y_hard)
        self.yard_disagree = int((~agree).sum())
        on = agree & self.converged
        self.yard_frames = int(on.sum())
        self.yard = float(deviation(self.llr[on], y_llr[on]).max()) if on.any() else 0.0
        self.bound = MARGIN * self.yard
        # Ties.  np_mix has five pairs of degree-1 columns on one check node each; on the BSC, where every input has the same
        # magnitude, a pair with opposite signs ends with both totals at EXACTLY zero in modes 1 and 2 (nothing else ever
        # reaches a degree-1 column), and which way `<= 0` falls is decided by the last bit: the perturbation alone then
        # changes a decision in 49 frames of 512 — both decisions of a pair together, its input being one number; in the
        # kernels, whose two lanes round apart, the pair's parity moves as well, and with it the syndrome and iters.  The cap
        # taken from that count (4 x 49 + 4) says little there, so the frames in which the mirror has NO |llr_out| within the
        # bound — none of its decisions hangs on the last bits — are counted a second time on their own.
        self.clear = ~(np.abs(self.llr) <= self.bound).any(axis=1)
        self.ties = bool((self.llr == 0.0).any())
        self.yard_disagree_clear = int((~agree & self.clear).sum())

    def agree(self, it, hard):
        return (it == self.it) & (hard == self.hard).all(axis=1)

    def check(self, got, what):
        agree = self.agree(got["iters"], got["hard"])
        disagree, clear = int((~agree).sum()), int((~agree & self.clear).sum())
        on = agree & self.converged
        dev = float(deviation(self.llr[on], got["llr_out"][on]).max())
        print(f"whole {what}: {disagree} frames disagree (yardstick {self.yard_disagree}), of {int(self.clear.sum())} clear "
              f"frames {clear} (yardstick {self.yard_disagree_clear}), deviation {dev:.3e} = {dev / self.yard:.3f} x yardstick "
              f"{self.yard:.3e} on {int(on.sum())} frames")
        assert disagree <= 4 * self.yard_disagree + 4, (what, disagree, self.yard_disagree)
        assert clear <= 4 * self.yard_disagree_clear + 4, (what, clear, self.yard_disagree_clear)
        assert on.sum() > len(self.it) // 2, (what, int(on.sum()))
        assert dev <= self.bound, (what, dev, self.bound)
        return dev / self.yard
