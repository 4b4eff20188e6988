"""numpy restatement of ldpc_hip_syndrome_decode_batch as include/ldpc_amd.h states it: quantized min-sum decoding toward a
given syndrome — the mirror kernels_syndrome_decode.hip is held against, bit for bit.  QuantizedMinSumMirror
(tests/quantized_minsum_ref.py) with the two changes (a check node's sign parity starts at its syndrome bit; the stop test
asks for the syndrome) and the two additions (weight; iterations == 0 returns the quantized input).  Does not import the
library; the codes of the tests, their augmented forms [H | I] and the inputs live here too, computed once per process."""
import os
import types
import zlib

import numpy as np

import channel_ref as cr
import gf2_ref
import orc
from quantized_minsum_ref import QuantizedMinSumMirror, correction_table, qmax_of, quantize
from test_gpu_random_codes import make_code_by_degrees

KEYS = ("hard_bits", "iters", "weight", "llr_out")
NP_MIX = ([1] * 70 + [2] * 200 + [3] * 330 + [4] * 100 + [6] * 50 + [9] * 30 + [17] * 10,
          [2] * 50 + [3] * 100 + [4] * 100 + [5] * 80 + [6] * 100 + [7] * 40 + [8] * 65)
CODES = {
    # name: (column degrees, check degrees)
    "sd_r36": ([3] * 576, [6] * 288),     # mc a whole number of syndrome words
    "sd_mix": NP_MIX,                     # check degrees 2..8, column degrees 1..17, a partial last word on both sides
    "sd_wide": ([3] * 800, [20] * 120),   # several words per row
    "sd_small": ([2] * 40, [4] * 20),     # fewer nodes than threads, one partial syndrome word
}
NAMES = tuple(CODES) + ("golden",)
# (q_bits, step, scale, offset)
SETTINGS = ((6, 0.25, 0.8125, 0.0), (8, 0.125, 1.0, 0.0), (2, 2.0, 1.0, 0.0), (5, 0.5, 0.75, 0.25))
# the BSC point and the frames per code at which, under SETTINGS[0], some frames reach their syndrome and some do not
POINTS = {"sd_r36": (0.06, 256), "sd_mix": (0.02, 256), "sd_wide": (0.005, 256), "sd_small": (0.06, 128), "golden": (0.15, 64)}
X_SEED, NOISE_SEED = 5, 9
SHORTEN = 99999.9


def write_code(name, directory):
    """The code's parity-check file in `directory` (tests/golden/h.txt for "golden")."""
    if name == "golden":
        return orc.H_TXT
    path = os.path.join(str(directory), name + ".txt")
    if not os.path.exists(path):
        vn, cn = CODES[name]
        make_code_by_degrees(path, vn, cn, np.random.default_rng(zlib.crc32(name.encode())))
    return path


def write_augmented(path, out):
    """[H | I] of the code in `path` as a file in (row, column) order: column nc + r in row r alone.  Header lines are dropped:
    the augmented code serves decode calls on caller-supplied LLRs only."""
    g = gf2_ref.Gf2Code(path)
    rows = np.concatenate((g.h_rows, np.arange(g.mc)))
    cols = np.concatenate((g.h_cols, g.nc + np.arange(g.mc)))
    order = np.lexsort((cols, rows))
    open(out, "w").write("\n".join(f"{r} {c}" for r, c in zip(rows[order], cols[order])))
    return out


def graph(path):
    """What MinSumMirror reads of a code (edge order = file line order), from the file alone."""
    g = gf2_ref.Gf2Code(path)
    return types.SimpleNamespace(nc=g.nc, mc=g.mc, nnz=g.h_rows.size, edge_row=g.h_rows, edge_col=g.h_cols, bit_pos=g.bit_pos)


class SyndromeDecodeMirror(QuantizedMinSumMirror):
    def input_values(self, llr, bits, step):
        """L[n][nc]: an int8 k counts steps, clamp(k); every other type is widened exactly and quantized."""
        llr = np.asarray(llr)
        if llr.dtype == np.int8:
            q = qmax_of(bits)
            return np.clip(llr.astype(np.int64), -q, q).reshape(-1, self.nc)
        return quantize(llr.astype(np.float64), bits, step).reshape(-1, self.nc)

    def decode_toward(self, llr, syndrome, bits, step, scale=1.0, offset=0.0, early_term=True, iterations=50):
        """llr[n][nc] (any element type of the call), syndrome[n][mc] bytes in file row order (None = all zero) ->
        dict(iters, hard, total, llr_out, weight)."""
        L = self.input_values(llr, bits, step)
        n = L.shape[0]
        syn = np.zeros((n, self.mc), np.int64) if syndrome is None else (np.asarray(syndrome) != 0).astype(np.int64).reshape(n, self.mc)
        q = qmax_of(bits)
        lut = correction_table(bits, step, scale, offset)
        iters = np.full(n, iterations, np.int64)
        total = L.copy()                         # iterations == 0: the quantized input
        hard = (L <= 0).astype(np.uint8)
        active = np.arange(n)
        v2c = L[:, self.ecol].copy()
        s_act = syn
        for it in range(iterations):
            mag, neg = np.abs(v2c), v2c < 0
            c2v = np.empty_like(v2c)
            for idx in self.rows:
                a = mag[:, idx]
                s = neg[:, idx]
                k = np.argmin(a, axis=2)[..., None]
                m1 = np.take_along_axis(a, k, 2)
                a2 = a.copy()
                np.put_along_axis(a2, k, 1 << 20, 2)
                m2 = a2.min(axis=2, keepdims=True)
                out_mag = lut[np.where(np.arange(idx.shape[1])[None, None, :] == k, m2, m1)]
                rows = self.row_of_edge[idx[:, 0]]
                # negative iff (the others that are < 0) + s[c] is odd
                out_neg = np.logical_xor.reduce(s, axis=2, keepdims=True) ^ s ^ (s_act[:, rows, None] != 0)
                c2v[:, idx] = np.where(out_neg, -out_mag, out_mag)
            out = L.copy()
            for cols, e in self.vpos:
                out[:, cols] += c2v[:, e]
            for cols, e in self.vpos:
                v2c[:, e] = np.clip(out[:, cols] - c2v[:, e], -q, q)
            hb = (out <= 0).astype(np.uint8)
            total[active] = out
            hard[active] = hb
            if early_term:
                done = ~(self._syndrome(hb) != s_act).any(axis=1)
                if done.any():
                    iters[active[done]] = it
                    keep = ~done
                    active, v2c, L, s_act = active[keep], v2c[keep], L[keep], s_act[keep]
                    if active.size == 0:
                        break
        weight = (self._syndrome(hard) != syn).sum(axis=1)
        return {"iters": iters, "hard": hard, "total": total, "llr_out": total.astype(np.float64) * np.float64(step), "weight": weight}

    def expected(self, *args, **kwargs):
        """decode_toward in the dtypes and layouts of the call's outputs."""
        r = self.decode_toward(*args, **kwargs)
        return {"hard_bits": gf2_ref.pack(r["hard"]), "iters": r["iters"].astype(np.uint32), "weight": r["weight"].astype(np.uint32),
                "llr_out": r["llr_out"]}


class Codes:
    """Files, mirrors, decoders and inputs of the test codes, each made at the first question and never changed."""

    def __init__(self, directory):
        self.directory = directory
        self.files, self._mirror, self._gf2, self._dec, self._frames = {}, {}, {}, {}, {}

    def path(self, name):
        if name not in self.files:
            if name.endswith("+I"):
                self.files[name] = write_augmented(self.path(name[:-2]), os.path.join(str(self.directory), name[:-2] + "_aug.txt"))
            else:
                self.files[name] = write_code(name, self.directory)
        return self.files[name]

    def mirror(self, name):
        if name not in self._mirror:
            self._mirror[name] = SyndromeDecodeMirror(graph(self.path(name)))
        return self._mirror[name]

    def gf2(self, name):
        if name not in self._gf2:
            self._gf2[name] = gf2_ref.Gf2Code(self.path(name))
        return self._gf2[name]

    def decoder(self, name):
        if name not in self._dec:
            import libldpc_amd
            self._dec[name] = libldpc_amd.HipDecoder(self.path(name))
        return self._dec[name]

    def frames(self, name, eps=None, n=None, x_seed=X_SEED, noise_seed=NOISE_SEED):
        """dict(x, s, llr): n random words x (not codewords), s = H x, and the LLRs of x through the BSC mirror."""
        eps, n = POINTS[name][0] if eps is None else eps, POINTS[name][1] if n is None else n
        key = (name, eps, n, x_seed, noise_seed)
        if key not in self._frames:
            code = self.gf2(name)
            x = np.random.default_rng(x_seed).integers(0, 2, (n, code.nc), dtype=np.uint8)
            s, _ = code.syndrome(x)
            _, llr = cr.bsc(code, eps, noise_seed, np.arange(n), x)
            out = {"x": x, "s": s, "llr": llr}
            for v in out.values():
                v.setflags(write=False)
            self._frames[key] = out
        return self._frames[key]
