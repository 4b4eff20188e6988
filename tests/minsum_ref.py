"""numpy restatement of BP_MS decoding with the min-sum correction of include/ldpc_amd.h
(ldpc_hip_set_min_sum_correction) — the mirror the corrected kernels are held against, bit for bit.

The reference's orders are kept (decoder.cpp:11-78): v2c starts as the channel LLR of the edge's
column; a check node's output magnitude is the smallest corrected |v2c| over its other edges, its sign bit the XOR of
their sign bits (exact, so the row order does not matter); a variable node sums its c2v messages onto the channel LLR in
column file order, v2c = out - c2v, hard decision out <= 0; early termination when the decisions satisfy every row.
Vectorised over frames, over check nodes of one degree, and over columns by edge position.
"""
import numpy as np


def correct(mag, scale, offset):
    """max(fl(fl(scale * m) - offset), +0.0) of non-negative magnitudes m (numpy rounds every operation: no fma)."""
    r = (mag * np.float64(scale)) - np.float64(offset)
    return np.where(r > 0.0, r, 0.0)


class MinSumMirror:
    def __init__(self, code):
        """code: tests/orc.py Code (edge order = file line order)."""
        er, ec = np.asarray(code.edge_row, np.int64), np.asarray(code.edge_col, np.int64)
        self.nc, self.mc, self.nnz = code.nc, code.mc, code.nnz
        self.ecol = ec
        self.bit_pos = np.asarray(code.bit_pos, np.int64)
        # check nodes grouped by degree: idx[rows, d] = edge indices in row file order
        order = np.argsort(er, kind="stable")
        rdeg = np.bincount(er, minlength=self.mc)
        rstart = np.concatenate(([0], np.cumsum(rdeg)))
        self.rows = []
        for d in np.unique(rdeg):
            if d == 0:
                continue
            assert d >= 2, "a check node of degree 1 has no other edges"
            rs = np.nonzero(rdeg == d)[0]
            self.rows.append(order[rstart[rs][:, None] + np.arange(d)[None, :]])
        # columns by edge position p: cols_p, edge of (col, p) in column file order
        corder = np.argsort(ec, kind="stable")
        cdeg = np.bincount(ec, minlength=self.nc)
        cstart = np.concatenate(([0], np.cumsum(cdeg)))
        self.vpos = []
        for p in range(int(cdeg.max()) if self.nnz else 0):
            cols = np.nonzero(cdeg > p)[0]
            self.vpos.append((cols, corder[cstart[cols] + p]))
        self.row_of_edge = er

    def decode(self, llr_in, scale=1.0, offset=0.0, early_term=True, iterations=50, codeword=None):
        """llr_in[n][nc] -> dict(iters, hard, llr_out, bit_errors) as the C ABI returns them."""
        llr_in = np.ascontiguousarray(llr_in, np.float64).reshape(-1, self.nc)
        n = llr_in.shape[0]
        iters = np.full(n, iterations, np.int64)
        llr_out = np.zeros((n, self.nc))
        hard = np.zeros((n, self.nc), np.uint8)
        active = np.arange(n)
        v2c = llr_in[:, self.ecol].copy()
        L = llr_in
        for it in range(iterations):
            # ---- check nodes ----
            mag = correct(np.abs(v2c), scale, offset)
            neg = np.signbit(v2c)
            c2v = np.empty_like(v2c)
            for idx in self.rows:
                a = mag[:, idx]                      # [f, rows, d]
                s = neg[:, idx]
                k = np.argmin(a, axis=2)             # the first edge holding the smallest magnitude
                m1 = np.take_along_axis(a, k[..., None], 2)
                a2 = a.copy()
                np.put_along_axis(a2, k[..., None], np.inf, 2)
                m2 = a2.min(axis=2, keepdims=True)
                pos = np.arange(idx.shape[1])[None, None, :]
                out_mag = np.where(pos == k[..., None], m2, m1)
                out_neg = np.logical_xor.reduce(s, axis=2, keepdims=True) ^ s
                c2v[:, idx] = np.where(out_neg, -out_mag, out_mag)
            # ---- variable nodes, column file order ----
            out = L.copy()
            for cols, e in self.vpos:
                out[:, cols] += c2v[:, e]
            for cols, e in self.vpos:
                v2c[:, e] = out[:, cols] - c2v[:, e]
            hb = (out <= 0).astype(np.uint8)
            llr_out[active] = out
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
        return {"iters": iters, "hard": hard, "llr_out": llr_out, "bit_errors": bit_errors}

    def _syndrome(self, hb):
        bits = hb[:, self.ecol].astype(np.int64)  # [f, nnz]
        synd = np.zeros((hb.shape[0], self.mc), np.int64)
        for idx in self.rows:
            rows = self.row_of_edge[idx[:, 0]]
            synd[:, rows] = bits[:, idx].sum(axis=2) & 1
        return synd
