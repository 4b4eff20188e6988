"""numpy restatement of ldpc_hip_relay_decode_batch as include/ldpc_amd.h states it (items 1..10): quantized min-sum with
memory, run as a relay of legs, toward a given syndrome — the mirror kernels_relay_decode.hip is held against, bit for bit.
SyndromeDecodeMirror (tests/syndrome_decode_ref.py) supplies the quantizer, the graph and the syndrome; the iteration is
written here in the order of the header (memory term, variable nodes, check nodes, totals, test), not in the fused order of
the kernel.  Does not import the library.  Also here: the gamma table on tests/philox_ref.py (tag 4), the toric X-check
code's file, and the inputs of the tests, computed once per process.

The seed of the gamma table: GAMMA_SEED = 3 (the first tried).  On toric6 (256 frames, p = 0.09, default_rng(11), 12 legs,
first 8, lo -16, hi 42, first_iterations 50, leg_iterations 30) the mirror gives all four conditions of
tests/test_relay_decode_host.py, test_the_conditions_on_toric6, which asserts them before any kernel is compared."""
import os

import numpy as np

import gf2_ref
import philox_ref
import syndrome_decode_ref as sd
from quantized_minsum_ref import correction_table, qmax_of

KEYS = ("hard_bits", "iters", "weight", "solutions", "best_leg", "cost")
NONE = 0xFFFFFFFF
TAG_RELAY = 4
NAMES = sd.NAMES + ("toric6",)
SETTINGS = sd.SETTINGS
TORIC_P, TORIC_SEED, TORIC_FRAMES = 0.09, 11, 256
GAMMA_SEED = 3
# the relay of the toric tests: (legs, first, lo, hi, first_iterations, leg_iterations)
TORIC_RELAY = dict(legs=12, first=8, lo=-16, hi=42, first_iterations=50, leg_iterations=30)


def gammas(nc, legs, lo, hi, seed, first=0):
    """int8 [legs][nc]: row 0 is `first`; row l >= 1, column v is lo + ((draw * (hi - lo + 1)) >> 32), the draw word v & 3 of
    Philox block v >> 2 of frame l under tag 4."""
    g = np.full((legs, nc), first, np.int64)
    if legs > 1:
        w = philox_ref.blocks(seed, TAG_RELAY, np.arange(1, legs), np.arange((nc + 3) // 4)).reshape(legs - 1, -1)[:, :nc]
        g[1:] = lo + ((w.astype(np.uint64) * np.uint64(hi - lo + 1)) >> np.uint64(32)).astype(np.int64)
    assert g.min() >= -128 and g.max() <= 127
    return g.astype(np.int8)


def write_toric(path, size):
    """The X-checks of the size x size toric code as `row col` lines: 2 size^2 columns, h(i, j) = i size + j and
    v(i, j) = size^2 + i size + j; vertex (i, j), row i size + j, touches h(i, j), h(i, j - 1), v(i, j), v(i - 1, j)."""
    if not os.path.exists(path):
        lines = []
        for i in range(size):
            for j in range(size):
                cols = (i * size + j, i * size + (j - 1) % size, size * size + i * size + j, size * size + ((i - 1) % size) * size + j)
                lines += [f"{i * size + j} {c}" for c in sorted(cols)]
        open(path, "w").write("\n".join(lines))
    return path


def memory_term(g, A, L):
    """Lambda of item 4 (int64 arrays that broadcast): clamp(L + sign(p) ((|p| + 32) >> 6), +-32767), p = clamp(g) (A - L)."""
    p = np.clip(np.asarray(g, np.int64), -64, 64) * (np.asarray(A, np.int64) - np.asarray(L, np.int64))
    assert np.abs(p).max(initial=0) < 2**31
    return np.clip(L + np.sign(p) * ((np.abs(p) + 32) >> 6), -32767, 32767)


class RelayDecodeMirror(sd.SyndromeDecodeMirror):
    def _check_nodes(self, v2c, syn, lut):
        """Item 6: c2v of v2c[f][nnz] toward syn[f][mc]."""
        mag, neg = np.abs(v2c), v2c < 0
        c2v = np.zeros_like(v2c)
        for idx in self.rows:
            a, s = mag[:, idx], neg[:, idx]
            k = np.argmin(a, axis=2)[..., None]
            m1 = np.take_along_axis(a, k, 2)
            a2 = a.copy()
            np.put_along_axis(a2, k, 1 << 20, 2)
            m2 = a2.min(axis=2, keepdims=True)
            out_mag = lut[np.where(np.arange(idx.shape[1])[None, None, :] == k, m2, m1)]
            rows = self.row_of_edge[idx[:, 0]]
            out_neg = np.logical_xor.reduce(s, axis=2, keepdims=True) ^ s ^ (syn[:, rows, None] != 0)
            c2v[:, idx] = np.where(out_neg, -out_mag, out_mag)
        return c2v

    def _column_sums(self, base, c2v):
        out = base.copy()
        for cols, e in self.vpos:
            out[:, cols] += c2v[:, e]
        return out

    def relay(self, llr, syndrome, gamma, bits, step, scale=1.0, offset=0.0, *, legs, first_iterations=50, leg_iterations=30, stop_after=1):
        """llr[n][nc] (any element type of the call; one row is NOT repeated here: pass n rows), syndrome[n][mc] bytes (None =
        all zero), gamma[legs][nc] (None = all zero) -> dict(hard, iters, weight, solutions, best_leg, cost, first_leg)."""
        L = self.input_values(llr, bits, step)
        n = L.shape[0]
        syn = np.zeros((n, self.mc), np.int64) if syndrome is None else (np.asarray(syndrome) != 0).astype(np.int64).reshape(n, self.mc)
        gamma = np.zeros((legs, self.nc), np.int64) if gamma is None else np.asarray(gamma).astype(np.int64).reshape(legs, self.nc)
        q, lut = qmax_of(bits), correction_table(bits, step, scale, offset)
        y, r = L <= 0, np.abs(L)
        A = L.copy()                                        # item 2
        hard = y.astype(np.uint8)
        kept = np.zeros((n, self.nc), np.uint8)
        iters, solutions = np.zeros(n, np.int64), np.zeros(n, np.int64)
        best_leg, cost, first_leg = np.full(n, NONE, np.int64), np.full(n, NONE, np.int64), np.full(n, NONE, np.int64)
        for leg in range(legs):
            act = np.flatnonzero(solutions < stop_after)    # item 9
            if act.size == 0:
                break
            T = first_iterations if leg == 0 else leg_iterations
            c2v = np.zeros((act.size, self.nnz), np.int64)  # item 3
            for i in range(T):
                lam = memory_term(gamma[leg][None, :], A[act], L[act])          # item 4
                total = self._column_sums(lam, c2v)
                v2c = np.empty_like(c2v)
                for cols, e in self.vpos:                                       # item 5
                    v2c[:, e] = np.clip(total[:, cols] - c2v[:, e], -q, q)
                c2v = self._check_nodes(v2c, syn[act], lut)                     # item 6
                A[act] = self._column_sums(lam, c2v)                            # item 7
                hb = (A[act] <= 0).astype(np.uint8)
                hard[act] = hb
                done = ~(self._syndrome(hb) != syn[act]).any(axis=1)            # item 8
                if done.any():
                    f, word = act[done], hb[done]
                    iters[f] += i
                    solutions[f] += 1
                    first_leg[f] = np.where(first_leg[f] == NONE, leg, first_leg[f])
                    c = (r[f] * (word != y[f])).sum(axis=1)
                    better = (best_leg[f] == NONE) | (c < cost[f])
                    kept[f[better]], cost[f[better]], best_leg[f[better]] = word[better], c[better], leg
                    act, c2v = act[~done], c2v[~done]
                    if act.size == 0:
                        break
            iters[act] += T
        found = best_leg != NONE
        word = np.where(found[:, None], kept, hard)         # item 10
        weight = (self._syndrome(word) != syn).sum(axis=1)
        assert np.array_equal(weight == 0, found)           # (the last iteration run was tested and failed)
        return {"hard": word, "iters": iters, "weight": weight, "solutions": solutions, "best_leg": best_leg, "cost": cost, "first_leg": first_leg}

    def expected(self, *args, **kwargs):
        """relay in the dtypes and layouts of the call's outputs."""
        r = self.relay(*args, **kwargs)
        out = {k: r[k].astype(np.uint32) for k in KEYS[1:]}
        out["hard_bits"] = gf2_ref.pack(r["hard"])
        return out


class Codes(sd.Codes):
    """The codes of syndrome_decode_ref with the BSC frames of that module, and toric6 with Bernoulli(p) errors and one shared
    prior row."""

    def path(self, name):
        if name.startswith("toric") and name not in self.files:
            self.files[name] = write_toric(os.path.join(str(self.directory), name + ".txt"), int(name[5:]))
        return super().path(name)

    def mirror(self, name):
        if name not in self._mirror:
            self._mirror[name] = RelayDecodeMirror(sd.graph(self.path(name)))
        return self._mirror[name]

    def toric(self, name="toric6", n=TORIC_FRAMES, p=TORIC_P, seed=TORIC_SEED):
        """dict(x, s, llr): n errors x ~ Bernoulli(p) of default_rng(seed), s = H x, and the ONE prior row log((1 - p) / p)."""
        key = (name, p, n, seed)
        if key not in self._frames:
            code = self.gf2(name)
            x = (np.random.default_rng(seed).random((n, code.nc)) < p).astype(np.uint8)
            s, _ = code.syndrome(x)
            out = {"x": x, "s": s, "llr": np.full(code.nc, np.log((1.0 - p) / p))}
            for v in out.values():
                v.setflags(write=False)
            self._frames[key] = out
        return self._frames[key]

    def toric_gamma(self, name="toric6"):
        t = TORIC_RELAY
        return gammas(self.gf2(name).nc, t["legs"], t["lo"], t["hi"], GAMMA_SEED, t["first"])

    def toric_expected(self, setting, stop_after, name="toric6"):
        """The mirror's outputs on the toric frames under the relay of the tests, once per (setting, stop_after)."""
        key = ("expected", name, setting, stop_after)
        if key not in self._frames:
            f, t = self.toric(name), TORIC_RELAY
            n = f["s"].shape[0]
            self._frames[key] = self.mirror(name).expected(
                np.repeat(f["llr"][None, :], n, 0), f["s"], self.toric_gamma(name), *setting, legs=t["legs"],
                first_iterations=t["first_iterations"], leg_iterations=t["leg_iterations"], stop_after=stop_after)
        return self._frames[key]
