"""numpy restatement of layered (row-serial) min-sum decoding as include/ldpc_amd.h states it
(ldpc_hip_set_min_sum_schedule) — the mirror the layered min-sum kernel is held against, bit for bit.

One total T[v] per variable node, one message m[c][j] per edge, all binary64 and every operation rounded once (numpy has
no fused multiply-add).  A sweep visits the steps of the layered plan in order — taken from orc.Code.layer_steps(), the
oracle's own restatement of the plan, which test_host.py holds equal to the product's; the check nodes of a step share no
variable node, so they are updated together here (vectorised over frames and over the step's check nodes):
t = T - m, output magnitude = the corrected smallest |t| over the node's other edges, output sign = XOR of the other edges'
sign bits, T = t + m.  After every sweep hard = (T <= 0); early termination on a zero syndrome, iters = sweeps completed
before the sweep whose syndrome passed.
"""
import numpy as np

from minsum_ref import correct


class LayeredMinSumMirror:
    def __init__(self, code):
        """code: tests/orc.py Code (edge order = file line order)."""
        er, ec = np.asarray(code.edge_row, np.int64), np.asarray(code.edge_col, np.int64)
        self.nc, self.mc = code.nc, code.mc
        self.bit_pos = np.asarray(code.bit_pos, np.int64)
        n_steps, step_of = code.layer_steps()
        assert n_steps > 0, "the layered plan does not take this code"
        order = np.argsort(er, kind="stable")  # edges by row, file order within a row
        rdeg = np.bincount(er, minlength=self.mc)
        rstart = np.concatenate(([0], np.cumsum(rdeg)))
        # steps[s] = columns [rows of the step in file order, d]
        self.steps = []
        for s in range(n_steps):
            rows = np.nonzero(np.asarray(step_of) == s)[0]
            d = rdeg[rows[0]]
            assert (rdeg[rows] == d).all() and 2 <= d <= 8 and rows.size <= 64
            cols = ec[order[rstart[rows][:, None] + np.arange(d)[None, :]]]
            assert np.unique(cols).size == cols.size, "the check nodes of a step share no variable node"
            self.steps.append(cols)

    @staticmethod
    def _check_nodes(t, scale, offset):
        """t[..., d] = a check node's inputs -> its new messages."""
        a, s = np.abs(t), np.signbit(t)
        k = np.argmin(a, axis=-1)[..., None]  # the first edge holding the smallest magnitude
        m1 = np.take_along_axis(a, k, -1)
        a2 = a.copy()
        np.put_along_axis(a2, k, np.inf, -1)
        m2 = a2.min(axis=-1, keepdims=True)
        r = correct(np.where(np.arange(t.shape[-1]) == k, m2, m1), scale, offset)
        neg = np.logical_xor.reduce(s, axis=-1, keepdims=True) ^ s
        return np.where(neg, -r, r)  # (-(+0.0) = -0.0: a zero carries its sign bit)

    def decode(self, llr_in, scale=1.0, offset=0.0, early_term=True, iterations=50, codeword=None, row_order=None):
        """llr_in[n][nc] -> dict(iters, hard, llr_out, bit_errors) as the C ABI returns them.  row_order: None = a step's
        check nodes together; "forward" / "reversed" = one after the other in that order (the same result)."""
        llr_in = np.ascontiguousarray(llr_in, np.float64).reshape(-1, self.nc)
        n = llr_in.shape[0]
        iters = np.full(n, iterations, np.int64)
        llr_out = np.zeros((n, self.nc))
        hard = np.zeros((n, self.nc), np.uint8)
        active = np.arange(n)
        T = llr_in.copy()
        M = [np.zeros((n,) + cols.shape) for cols in self.steps]  # every message +0.0
        for it in range(iterations):
            for si, cols in enumerate(self.steps):
                if row_order is None:
                    t = T[:, cols] - M[si]
                    M[si] = self._check_nodes(t, scale, offset)
                    T[:, cols] = t + M[si]
                else:
                    rows = range(cols.shape[0]) if row_order == "forward" else range(cols.shape[0] - 1, -1, -1)
                    for r in rows:
                        t = T[:, cols[r]] - M[si][:, r]
                        M[si][:, r] = self._check_nodes(t, scale, offset)
                        T[:, cols[r]] = t + M[si][:, r]
            hb = (T <= 0).astype(np.uint8)
            llr_out[active] = T
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
        return {"iters": iters, "hard": hard, "llr_out": llr_out, "bit_errors": bit_errors}
