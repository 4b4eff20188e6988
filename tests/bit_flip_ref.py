"""numpy restatement of ldpc_hip_bit_flip_batch as include/ldpc_amd.h states it, items 1..7: gradient-descent bit flipping
toward a given syndrome, deterministic (GDBF, every candidate flips) and probabilistic (PGDBF, a candidate flips iff its
Philox draw under tag 3 is below the threshold) — the mirror kernels_bit_flip.hip is held against, bit for bit.  Does not
import the library.  The codes of the tests (those of tests/syndrome_decode_ref.py and the code with entries listed twice of
tests/test_gpu_erasure_batch.py), the settings and the operating points live here too."""
import os

import numpy as np

import channel_ref as cr
import erasure_ref as er
import generator_codes as gc
import gf2_ref
import philox_ref
import syndrome_decode_ref as sd
from quantized_minsum_ref import qmax_of, quantize

KEYS = ("hard_bits", "iters", "weight")
TAG_FLIP = 3
EVERY_CANDIDATE = 0xFFFFFFFF
NAMES = sd.NAMES + ("s40x60_hdup",)
N, ROUNDS = 128, 100
# the BSC point per code at which the deterministic setting (w = 2, q_bits = 2, step = |llr|, N frames, ROUNDS rounds)
# leaves frames that reach their syndrome and frames that do not, with the margin it needs and the frames that reach it
# (test_bit_flip_host.py asserts the count).  "golden" with margin 0 reaches s on no frame: its 128 punctured columns
# quantize to 0, all tie, and flip together — kept as the degenerate case.
POINTS = {"sd_r36": (0.03, 0, 106), "sd_mix": (0.01, 0, 107), "sd_wide": (0.004, 0, 110), "sd_small": (0.05, 0, 87),
          "golden": (0.01, 1, 75), "s40x60_hdup": (0.03, 0, 102)}
# (w, margin, flip_prob, q_bits): the step of the first three is the |llr| of the BSC point
HARD_SETTINGS = ((2, 0, 1.0, 2), (2, 0, 0.7, 2), (2, 1, 1.0, 2))
SOFT_SETTING = (16, 4, 1.0, 6, 0.25)  # ... and the step, on AWGN LLRs
# the BSC point of the probabilistic setting (2, 0, 0.7, 2): that of POINTS wherever both kinds of frame occur there among
# the first 67 frames too (reached, of 128: sd_mix 118, sd_wide 119, s40x60_hdup 102).  Moved: sd_r36 and sd_small, where all
# of the first 67 reach s at the deterministic point (0.04: 111, 0.1: 122), and "golden", which reaches s on no frame at
# 0.01 and on 19 at 0.004 — the draws break the tie of the punctured columns
PROB_POINTS = {name: p[0] for name, p in POINTS.items()} | {"sd_r36": 0.04, "sd_small": 0.1, "golden": 0.004}
# Es / sigma^2 in dB of the AWGN LLRs of the soft setting, and the frames of 128 that reach s there
SOFT_POINTS = {"sd_r36": 5.0, "sd_mix": 7.0, "sd_wide": 7.0, "sd_small": 3.0, "golden": 9.0, "s40x60_hdup": 5.0}
SOFT_REACHED = {"sd_r36": 90, "sd_mix": 76, "sd_wide": 82, "sd_small": 89, "golden": 59, "s40x60_hdup": 65}
SEED = 77  # of the draws


def threshold_of(flip_prob):
    """flip_prob 1.0 -> 0xFFFFFFFF (no draws), any other value -> floor(p 2^32)."""
    return EVERY_CANDIDATE if float(flip_prob) == 1.0 else int(float(flip_prob) * 2.0**32)


def draws(seed, frames, rnd, nc):
    """uint32 [len(frames)][nc]: word v & 3 of block rnd ceil(nc / 4) + (v >> 2) of each frame under tag 3."""
    per_round = (nc + 3) // 4
    w = philox_ref.blocks(seed, TAG_FLIP, np.asarray(frames, np.uint64), rnd * per_round + np.arange(per_round))
    return w.reshape(len(frames), -1)[:, :nc]


def _groups(index):
    """The entries sorted by the node they belong to: (order, the first entry of every node that has one, those nodes)."""
    order = np.argsort(index, kind="stable")
    g = index[order]
    starts = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
    return order, starts, g[starts]


def _sums(src, gather, groups, size):
    """out[n][size]: the sum of src[n][gather[e]] over the entries e of every node — every listing counts; a node without
    entries gets 0."""
    order, starts, present = groups
    out = np.zeros((src.shape[0], size), np.int64)
    if order.size and src.shape[0]:
        out[:, present] = np.add.reduceat(src[:, gather[order]], starts, axis=1)
    return out


class BitFlipMirror:
    def __init__(self, path):
        g = gf2_ref.Gf2Code(path)
        self.code, self.nc, self.mc = g, g.nc, g.mc
        self.by_row, self.by_col = _groups(g.h_rows), _groups(g.h_cols)

    def input_values(self, llr, bits, step):
        """L[n][nc], item 1: an int8 k counts steps, clamp(k); every other type is widened exactly and quantized."""
        llr = np.asarray(llr)
        if llr.dtype == np.int8:
            q = qmax_of(bits)
            return np.clip(llr.astype(np.int64), -q, q).reshape(-1, self.nc)
        return quantize(llr.astype(np.float64), bits, step).astype(np.int64).reshape(-1, self.nc)

    def unmet(self, x, syn):
        """u[n][mc], item 2: s XOR the XOR of x over the entries of each row (an entry listed twice counts twice)."""
        return (_sums(x.astype(np.int64), self.code.h_cols, self.by_row, self.mc) + syn) & 1

    def decode(self, llr, syndrome=None, iterations=50, q_bits=2, step=1.0, check_weight=2, margin=0, flip_threshold=EVERY_CANDIDATE,
               seed=0, first_frame=0, trace=None):
        """llr[n][nc] (any element type of the call; one row with a syndrome of n rows = the shared row), syndrome[n][mc]
        bytes in file row order (None = all zero) -> dict(hard [n][nc], iters [n], weight [n]).  trace: a list that receives
        (round, frames still running, their penalties P, the flips) of every round."""
        L = self.input_values(llr, q_bits, step)
        if syndrome is not None and L.shape[0] == 1:
            L = np.repeat(L, np.asarray(syndrome).shape[0], axis=0)
        n = L.shape[0]
        syn = np.zeros((n, self.mc), np.int64) if syndrome is None else (np.asarray(syndrome) != 0).astype(np.int64).reshape(n, self.mc)
        y, r = (L <= 0).astype(np.int64), np.abs(L)
        x = y.copy()
        iters = np.full(n, iterations, np.int64)
        active = np.arange(n)
        for t in range(iterations + 1):
            u = self.unmet(x[active], syn[active])
            met = ~u.any(axis=1)
            iters[active[met]] = t                    # a word that meets s is never flipped
            active, u = active[~met], u[~met]
            if t == iterations or active.size == 0:
                break
            U = _sums(u, self.code.h_rows, self.by_col, self.nc)  # an entry listed twice adds twice
            P = check_weight * U + np.where(x[active] != y[active], r[active], -r[active])
            flips = P >= P.max(axis=1, keepdims=True) - margin
            if flip_threshold != EVERY_CANDIDATE:
                flips &= draws(seed, first_frame + active, t, self.nc) < np.uint32(flip_threshold)
            if trace is not None:
                trace.append((t, active.copy(), P, flips.copy()))
            x[active] ^= flips                        # a round in which nothing flips still counts
        weight = self.unmet(x, syn).sum(axis=1)
        return {"hard": x.astype(np.uint8), "iters": iters, "weight": weight}

    def expected(self, *args, **kwargs):
        """decode in the dtypes and layouts of the call's outputs."""
        r = self.decode(*args, **kwargs)
        return {"hard_bits": gf2_ref.pack(r["hard"]), "iters": r["iters"].astype(np.uint32), "weight": r["weight"].astype(np.uint32)}


class Codes(sd.Codes):
    """sd.Codes with this entry's mirror, the code with entries listed twice, and the AWGN frames of the soft setting."""

    def path(self, name):
        if name == "s40x60_hdup" and name not in self.files:
            plain = gc.write_pair(self.directory, "s40x60")[0]
            self.files[name] = er.repeat_entries(plain, os.path.join(str(self.directory), "s40x60_hdup.h.txt"))
        return super().path(name)

    def mirror(self, name):
        if name not in self._mirror:
            self._mirror[name] = BitFlipMirror(self.path(name))
        return self._mirror[name]

    def hard_frames(self, name, n=N, eps=None):
        """dict(x, s, llr, step, k): the BSC frames of POINTS[name] (or of eps); step = |llr| of the point, k = the int8 +-1
        (a punctured column's 0 stays 0) the LLRs quantize to."""
        f = dict(self.frames(name, POINTS[name][0] if eps is None else eps, n))
        f["step"] = float(np.abs(f["llr"]).max())
        f["k"] = np.sign(f["llr"]).astype(np.int8)
        f["k"].setflags(write=False)
        return f

    def soft_frames(self, name, n=N):
        """dict(x, s, llr): n random words through the AWGN mirror (BPSK) at SOFT_POINTS[name]."""
        key = (name, "awgn", n)
        if key not in self._frames:
            code = self.gf2(name)
            x = np.random.default_rng(sd.X_SEED).integers(0, 2, (n, code.nc), dtype=np.uint8)
            s, _ = code.syndrome(x)
            received, _ = cr.awgn_received(code, 1, SOFT_POINTS[name], sd.NOISE_SEED, np.arange(n), x)
            out = {"x": x, "s": s, "llr": cr.awgn_llr(code, 1, SOFT_POINTS[name], received)}
            for v in out.values():
                v.setflags(write=False)
            self._frames[key] = out
        return self._frames[key]
