"""numpy restatement of fixed-point layered min-sum decoding as include/ldpc_amd.h states it
(ldpc_hip_set_min_sum_layered_fixed, items 1-7) — the mirror the kernel is held against, bit for bit.

q = msg_bits in 2..8, p = app_bits in q..16, step D, Qmax = 2^(q-1) - 1, Pmax = 2^(p-1) - 1.  The channel LLRs are quantized
once with quantized_minsum_ref.quantize (item 1); the totals start as T = L and every message as 0 (item 2); the correction
enters through quantized_minsum_ref.correction_table only (item 3).  A sweep visits the steps of the layered plan in order
(LayeredMinSumMirror builds them from orc.Code.layer_steps()): t = T - m, u = clamp(t, +-Qmax), output magnitude = lut[the
smallest |u| of the node's other edges], negative iff an odd number of the others is < 0 (an integer zero is not negative),
T = clamp(t + m, +-Pmax) (item 4).  After every sweep hard = (T <= 0); early termination on a zero syndrome, iters = sweeps
completed before the sweep whose syndrome passed (item 5); llr_out = fl(T * D) (item 6); no iteration: all zero (item 7).
Everything after the quantizer is int64.  Does not import the library.
"""
import numpy as np

from layered_minsum_ref import LayeredMinSumMirror
from quantized_minsum_ref import correction_table, qmax_of, quantize


class LayeredFixedMinSumMirror(LayeredMinSumMirror):
    @staticmethod
    def _check_nodes_fixed(u, lut):
        """u[..., d] = a check node's inputs at message width -> its new messages."""
        a, s = np.abs(u), u < 0
        k = np.argmin(a, axis=-1)[..., None]  # an edge holding the smallest magnitude
        m1 = np.take_along_axis(a, k, -1)
        a2 = a.copy()
        np.put_along_axis(a2, k, 1 << 20, -1)
        m2 = a2.min(axis=-1, keepdims=True)
        r = lut[np.where(np.arange(u.shape[-1]) == k, m2, m1)]
        neg = np.logical_xor.reduce(s, axis=-1, keepdims=True) ^ s
        return np.where(neg, -r, r)

    def decode(self, llr_in, msg_bits, app_bits, step, scale=1.0, offset=0.0, early_term=True, iterations=50, codeword=None,
               row_order=None):
        """llr_in[n][nc] -> dict(iters, hard, llr_out, bit_errors) as the C ABI returns them, and clamp_share: the share of
        the total updates (one per edge and sweep, over the sweeps each frame ran) that hit +-Pmax.  app_bits None: the
        totals are not clamped.  row_order: None = a step's check nodes together; "forward" / "reversed" = one after the
        other in that order (the same result)."""
        llr_in = np.ascontiguousarray(llr_in, np.float64).reshape(-1, self.nc)
        n = llr_in.shape[0]
        qmax = qmax_of(msg_bits)
        if app_bits is None:
            pmax = None
        else:
            assert msg_bits <= app_bits <= 16
            pmax = (1 << (app_bits - 1)) - 1
        lut = correction_table(msg_bits, step, scale, offset)
        iters = np.full(n, iterations, np.int64)
        total = np.zeros((n, self.nc), np.int64)
        hard = np.zeros((n, self.nc), np.uint8)
        active = np.arange(n)
        T = quantize(llr_in, msg_bits, step)
        M = [np.zeros((n,) + cols.shape, np.int64) for cols in self.steps]
        updates = clamped = 0

        def update(t):
            """t[..., d] -> the new messages, the new totals, how many of those were clamped"""
            u = np.clip(t, -qmax, qmax)
            m = self._check_nodes_fixed(u, lut)
            x = t + m
            if pmax is None:
                return m, x, 0
            y = np.clip(x, -pmax, pmax)
            return m, y, int((y != x).sum())

        for it in range(iterations):
            for si, cols in enumerate(self.steps):
                if row_order is None:
                    t = T[:, cols] - M[si]
                    M[si], T[:, cols], c = update(t)
                    clamped += c
                    updates += t.size
                else:
                    rows = range(cols.shape[0]) if row_order == "forward" else range(cols.shape[0] - 1, -1, -1)
                    for r in rows:
                        t = T[:, cols[r]] - M[si][:, r]
                        M[si][:, r], T[:, cols[r]], c = update(t)
                        clamped += c
                        updates += t.size
            hb = (T <= 0).astype(np.uint8)
            total[active] = T
            hard[active] = hb
            if early_term:
                bad = np.zeros(T.shape[0], bool)
                for cols in self.steps:
                    bad |= (hb[:, cols].sum(axis=2) & 1).any(axis=1)
                done = ~bad
                if done.any():
                    iters[active[done]] = it
                    keep = ~done
                    active, T, M = active[keep], T[keep], [m[keep] for m in M]
                    if active.size == 0:
                        break
        cw = np.zeros((n, self.nc), np.uint8) if codeword is None else np.asarray(codeword, np.uint8).reshape(n, self.nc)
        bit_errors = (hard[:, self.bit_pos] != cw[:, self.bit_pos]).sum(axis=1)
        llr_out = total.astype(np.float64) * np.float64(step)
        return {"iters": iters, "hard": hard, "llr_out": llr_out, "bit_errors": bit_errors,
                "clamp_share": clamped / updates if updates else 0.0}
