"""numpy restatement of ldpc_hip_syndrome_decode_layered_batch as include/ldpc_amd.h states it: fixed-point layered min-sum
decoding toward a given syndrome — the mirror kernels_syndrome_decode_layered.hip is held against, bit for bit.
LayeredFixedMinSumMirror (tests/layered_fixed_minsum_ref.py) with the two changes (a check node's sign parity starts at its
syndrome bit; the stop test asks for the syndrome) and the two additions (weight; iterations == 0 returns the quantized
input).  Does not import the library.  The codes, the BSC inputs and write_augmented are those of tests/syndrome_decode_ref.py;
one code is added here."""
import os
import zlib

import numpy as np

import gf2_ref
import orc
import syndrome_decode_ref as sd
from layered_fixed_minsum_ref import LayeredFixedMinSumMirror
from quantized_minsum_ref import correction_table, qmax_of, quantize
from test_gpu_random_codes import make_code_by_degrees

KEYS = sd.KEYS
# (column degrees, check degrees) of this file's own code.  nc = 63: odd, fewer columns than lanes, int8 rows at every byte
# alignment; every step of degree 7
SDL_ODD = ([3] * 63, [7] * 27)
NAMES = ("sd_small", "sdl_odd", "sd_r36", "sd_mix", "golden")  # what the layered plan takes (sd_wide: check nodes of degree 20)
# (msg_bits, app_bits, step, scale, offset)
SETTINGS = ((6, 8, 0.25, 0.8125, 0.0), (8, 16, 0.125, 1.0, 0.0), (2, 2, 2.0, 1.0, 0.0), (5, 7, 0.5, 0.75, 0.25))
# the BSC point and the frames per code at which, under SETTINGS[0] and 50 sweeps, some frames reach their syndrome and some
# do not (chosen on this mirror, with the inputs of sd.Codes.frames: tests/test_syndrome_decode_layered_host.py holds the
# counts)
POINTS = {"sd_small": (0.06, 128), "sdl_odd": (0.06, 128), "sd_r36": (0.07, 256), "sd_mix": (0.02, 256), "golden": (0.15, 64)}
REACHED = {"sd_small": 91, "sdl_odd": 91, "sd_r36": 196, "sd_mix": 212, "golden": 58}  # the frames of POINTS[name] that reach s


class SyndromeDecodeLayeredMirror(LayeredFixedMinSumMirror):
    def __init__(self, path):
        code = orc.Code(path)
        super().__init__(code)
        n_steps, step_of = code.layer_steps()
        # the file rows of each step's check nodes, in the order LayeredMinSumMirror lists their columns
        self.step_rows = [np.nonzero(np.asarray(step_of) == s)[0] for s in range(n_steps)]
        assert all(r.size == c.shape[0] for r, c in zip(self.step_rows, self.steps))

    def input_values(self, llr, msg_bits, step):
        """L[n][nc]: an int8 k counts steps, clamp(k); every other type is widened exactly and quantized."""
        llr = np.asarray(llr)
        if llr.dtype == np.int8:
            q = qmax_of(msg_bits)
            return np.clip(llr.astype(np.int64), -q, q).reshape(-1, self.nc)
        return quantize(llr.astype(np.float64), msg_bits, step).reshape(-1, self.nc)

    def _unmet(self, hard, syn):
        """[n] the check nodes whose XOR of the decisions over the row differs from the syndrome bit."""
        bad = np.zeros(hard.shape[0], np.int64)
        for rows, cols in zip(self.step_rows, self.steps):
            bad += ((hard[:, cols].sum(axis=2) & 1) != syn[:, rows]).sum(axis=1)
        return bad

    def decode_toward(self, llr, syndrome, msg_bits, app_bits, step, scale=1.0, offset=0.0, early_term=True, iterations=50):
        """llr[n][nc] (any element type of the call), syndrome[n][mc] bytes in file row order (None = all zero) ->
        dict(iters, hard, total, llr_out, weight)."""
        L = self.input_values(llr, msg_bits, step)
        n = L.shape[0]
        syn = np.zeros((n, self.mc), np.int64) if syndrome is None else (np.asarray(syndrome) != 0).astype(np.int64).reshape(n, self.mc)
        assert msg_bits <= app_bits <= 16
        qmax, pmax = qmax_of(msg_bits), (1 << (app_bits - 1)) - 1
        lut = correction_table(msg_bits, step, scale, offset)
        iters = np.full(n, iterations, np.int64)
        total = L.copy()  # iterations == 0: the quantized input
        hard = (L <= 0).astype(np.uint8)
        active = np.arange(n)
        T, s_act = L.copy(), syn
        M = [np.zeros((n,) + cols.shape, np.int64) for cols in self.steps]
        for it in range(iterations):
            for si, (rows, cols) in enumerate(zip(self.step_rows, self.steps)):
                t = T[:, cols] - M[si]
                u = np.clip(t, -qmax, qmax)
                m = self._check_nodes_fixed(u, lut)  # negative iff an odd number of the others is ...
                m = np.where(s_act[:, rows, None] != 0, -m, m)  # ... and iff that number + s[c] is odd
                M[si], T[:, cols] = m, np.clip(t + m, -pmax, pmax)
            hb = (T <= 0).astype(np.uint8)
            total[active] = T
            hard[active] = hb
            if early_term:
                done = self._unmet(hb, s_act) == 0
                if done.any():
                    iters[active[done]] = it
                    keep = ~done
                    active, T, M, s_act = active[keep], T[keep], [m[keep] for m in M], s_act[keep]
                    if active.size == 0:
                        break
        return {"iters": iters, "hard": hard, "total": total, "llr_out": total.astype(np.float64) * np.float64(step),
                "weight": self._unmet(hard, syn)}

    def expected(self, *args, **kwargs):
        """decode_toward in the dtypes and layouts of the call's outputs."""
        r = self.decode_toward(*args, **kwargs)
        return {"hard_bits": gf2_ref.pack(r["hard"]), "iters": r["iters"].astype(np.uint32), "weight": r["weight"].astype(np.uint32),
                "llr_out": r["llr_out"]}


class Codes(sd.Codes):
    """sd.Codes with the layered mirror, this file's code and its operating points."""

    def path(self, name):
        if name == "sdl_odd" and name not in self.files:  # written as sd.write_code writes the others
            self.files[name] = os.path.join(str(self.directory), name + ".txt")
            make_code_by_degrees(self.files[name], *SDL_ODD, np.random.default_rng(zlib.crc32(name.encode())))
        return super().path(name)

    def mirror(self, name):
        if name not in self._mirror:
            self._mirror[name] = SyndromeDecodeLayeredMirror(self.path(name))
        return self._mirror[name]

    def frames(self, name, eps=None, n=None, **kw):
        return super().frames(name, POINTS[name][0] if eps is None else eps, POINTS[name][1] if n is None else n, **kw)
