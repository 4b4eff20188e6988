"""numpy restatement of quantized (fixed-point) min-sum decoding as include/ldpc_amd.h states it
(ldpc_hip_set_min_sum_quantization) — the mirror the quantized kernel is held against, bit for bit.

bits q in 2..8, step D > 0, Qmax = 2^(q-1) - 1 (symmetric), inv = fl(1 / D).  The channel LLRs are quantized once,
L = clamp(rint(fl(llr * inv)), -Qmax, +Qmax) with the clamp in binary64 (numpy's rint is round-half-to-even; a NaN gives 0);
everything after that is integer arithmetic (int64 here, far from any overflow): v2c starts as L of the edge's column; a check
node's output magnitude is lut[the smallest |v2c| over its other edges], negative iff an odd number of the others is < 0 (an
integer zero is not negative); A = L + the sum of the c2v, v2c = clamp(A - c2v, -Qmax, +Qmax), hard = (A <= 0); the
flooding schedule, the early stop and the iteration count of MinSumMirror; llr_out = fl(A * D).  The correction enters
through lut[m] = max(0, rint(fl(fl(scale * m) - fl(offset * inv)))) only.  Does not import the library.
"""
import numpy as np

from minsum_ref import MinSumMirror


def qmax_of(bits):
    assert 2 <= bits <= 8
    return (1 << (bits - 1)) - 1


def correction_table(bits, step, scale=1.0, offset=0.0):
    """lut[0..Qmax] as the host builds it: binary64, every operation rounded once (numpy has no fused multiply-add)."""
    inv = np.float64(1.0) / np.float64(step)
    m = np.arange(qmax_of(bits) + 1, dtype=np.float64)
    r = np.rint((np.float64(scale) * m) - (np.float64(offset) * inv))
    return np.maximum(r, 0.0).astype(np.int64)


def quantize(llr, bits, step):
    """L = clamp(rint(fl(llr * inv)), -Qmax, +Qmax), the clamp before the conversion to an integer."""
    q = float(qmax_of(bits))
    inv = np.float64(1.0) / np.float64(step)
    with np.errstate(invalid="ignore"):
        x = np.rint(np.asarray(llr, np.float64) * inv)
    x = np.where(np.isnan(x), 0.0, np.clip(x, -q, q))
    return x.astype(np.int64)


class QuantizedMinSumMirror(MinSumMirror):
    def decode(self, llr_in, bits, step, scale=1.0, offset=0.0, early_term=True, iterations=50, codeword=None):
        """llr_in[n][nc] -> dict(iters, hard, llr_out, bit_errors) as the C ABI returns them."""
        llr_in = np.ascontiguousarray(llr_in, np.float64).reshape(-1, self.nc)
        n = llr_in.shape[0]
        q = qmax_of(bits)
        lut = correction_table(bits, step, scale, offset)
        iters = np.full(n, iterations, np.int64)
        total = np.zeros((n, self.nc), np.int64)
        hard = np.zeros((n, self.nc), np.uint8)
        active = np.arange(n)
        L = quantize(llr_in, bits, step)
        v2c = L[:, self.ecol].copy()
        for it in range(iterations):
            # ---- check nodes ----
            mag, neg = np.abs(v2c), v2c < 0
            c2v = np.empty_like(v2c)
            for idx in self.rows:
                a = mag[:, idx]                      # [f, rows, d]
                s = neg[:, idx]
                k = np.argmin(a, axis=2)[..., None]  # an edge holding the smallest magnitude
                m1 = np.take_along_axis(a, k, 2)
                a2 = a.copy()
                np.put_along_axis(a2, k, 1 << 20, 2)
                m2 = a2.min(axis=2, keepdims=True)
                out_mag = lut[np.where(np.arange(idx.shape[1])[None, None, :] == k, m2, m1)]
                out_neg = np.logical_xor.reduce(s, axis=2, keepdims=True) ^ s
                c2v[:, idx] = np.where(out_neg, -out_mag, out_mag)
            # ---- variable nodes: exact integer sums ----
            out = L.copy()
            for cols, e in self.vpos:
                out[:, cols] += c2v[:, e]
            for cols, e in self.vpos:
                v2c[:, e] = np.clip(out[:, cols] - c2v[:, e], -q, q)
            hb = (out <= 0).astype(np.uint8)
            total[active] = out
            hard[active] = hb
            if early_term:
                done = ~self._syndrome(hb).any(axis=1)
                if done.any():
                    iters[active[done]] = it
                    keep = ~done
                    active, v2c, L = active[keep], v2c[keep], L[keep]
                    if active.size == 0:
                        break
        cw = np.zeros((n, self.nc), np.uint8) if codeword is None else np.asarray(codeword, np.uint8).reshape(n, self.nc)
        bit_errors = (hard[:, self.bit_pos] != cw[:, self.bit_pos]).sum(axis=1)
        llr_out = total.astype(np.float64) * np.float64(step)
        return {"iters": iters, "hard": hard, "llr_out": llr_out, "bit_errors": bit_errors}
