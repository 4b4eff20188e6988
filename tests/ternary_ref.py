"""numpy restatement of ternary min-sum (Gallager's Algorithm E; include/ldpc_amd.h, ldpc_hip_set_min_sum_ternary, items
1-7) — the mirror the bit-sliced kernel (kernels_ternary.hip) is held against, bit for bit.

All integer: r = the sign of the decoder input (0 for +-0 and NaN), v2c starts as r of the edge's column, a check node's
output is the product of its other inputs, a variable node forms A = w r + the sum of its inputs, sends sgn(A - input) and
decides 1 iff 2 A + r <= 0.  Flooding, the syndrome early stop and the iteration count are those of MinSumMirror
(tests/minsum_ref.py), whose grouping of check nodes by degree and of columns by edge position is reused.  Vectorised over
frames; a frame that stops leaves the working set, so no frame sees another.
"""
import numpy as np

from minsum_ref import MinSumMirror


def received(llr_in):
    """Item 1: +1 where llr > 0, -1 where llr < 0, 0 for +-0 and NaN."""
    with np.errstate(invalid="ignore"):
        return (llr_in > 0).astype(np.int32) - (llr_in < 0).astype(np.int32)


class TernaryMirror(MinSumMirror):
    def decode(self, llr_in, weight, early_term=True, iterations=50, codeword=None):
        """llr_in[n][nc] -> dict(iters, hard, llr_out, bit_errors) as the C ABI returns them, and "c2v": the check nodes'
        messages of the last iteration, for the frames still decoding then (tests)."""
        assert 1 <= weight <= 7
        llr_in = np.ascontiguousarray(llr_in, np.float64).reshape(-1, self.nc)
        n = llr_in.shape[0]
        iters = np.full(n, iterations, np.int64)
        llr_out = np.zeros((n, self.nc))
        hard = np.zeros((n, self.nc), np.uint8)
        active = np.arange(n)
        r = received(llr_in)
        v2c = r[:, self.ecol].copy()
        c2v = np.zeros_like(v2c)
        for it in range(iterations):
            # ---- check nodes: zero if another input is zero, else the product of the others ----
            c2v = np.zeros_like(v2c)
            for idx in self.rows:
                a = v2c[:, idx]                                   # [f, rows, d]
                zero = a == 0
                others_zero = zero.sum(axis=2, keepdims=True) - zero
                unit = np.where(zero, 1, a)
                prod = unit.prod(axis=2, keepdims=True) * unit    # the product of the other non-zero inputs (unit = +-1)
                c2v[:, idx] = np.where(others_zero == 0, prod, 0)
            # ---- variable nodes ----
            A = weight * r
            for cols, e in self.vpos:
                A[:, cols] += c2v[:, e]
            for cols, e in self.vpos:
                v2c[:, e] = np.sign(A[:, cols] - c2v[:, e])
            hb = (2 * A + r <= 0).astype(np.uint8)
            llr_out[active] = A
            hard[active] = hb
            if early_term:
                done = ~self._syndrome(hb).any(axis=1)
                if done.any():
                    iters[active[done]] = it
                    keep = ~done
                    active, v2c, r = active[keep], v2c[keep], r[keep]
                    if active.size == 0:
                        break
        cw = np.zeros((n, self.nc), np.uint8) if codeword is None else np.asarray(codeword, np.uint8).reshape(n, self.nc)
        bit_errors = (hard[:, self.bit_pos] != cw[:, self.bit_pos]).sum(axis=1)
        return {"iters": iters, "hard": hard, "llr_out": llr_out, "bit_errors": bit_errors, "c2v": c2v}


# the two inputs the host and GPU tests share: (dv, dc)-regular codes of tools/gen_regular_code.generate, all-zero codeword,
# +-1.0 LLRs flipped with probability eps by numpy's generator: (nc, dv, dc, code seed, weight, eps, frames, numpy seed)
CASES = {"r36": (512, 3, 6, 1, 1, 0.04, 200, 11), "r48": (1024, 4, 8, 2, 2, 0.03, 200, 12)}


def flipped_llrs(nc, eps, n, seed):
    return np.where(np.random.default_rng(seed).random((n, nc)) < eps, -1.0, 1.0)
