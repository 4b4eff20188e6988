"""A numpy mirror of the three batch calls on frames of bits (include/ldpc_amd.h: ldpc_hip_encode_batch, _syndrome_batch,
_bit_errors_batch) and of their packed layout.  A plain module, numpy only: it parses the parity-check and generator files
itself and imports neither the library nor the oracle.  test_transmit_batch_host.py pins it against encode() and syndrome() of
Part 1; test_gpu_transmit_batch.py holds the kernels to it bit for bit."""
import numpy as np


def _entries(lines):
    rows, cols = [], []
    for line in lines:
        parts = line.split()
        if len(parts) >= 2:
            rows.append(int(parts[0]))
            cols.append(int(parts[1]))
    return np.asarray(rows, np.int64), np.asarray(cols, np.int64)


def _xor_groups(src, gather, group, n_groups):
    """out[g] = XOR over the entries e with group[e] == g of src[gather[e]] (rows of 0 / 1 bytes); an entry listed twice
    cancels, a group without entries stays 0.  Sums of bytes modulo 256 keep the parity."""
    out = np.zeros((n_groups, src.shape[1]), np.uint8)
    order = np.argsort(group, kind="stable")
    g = group[order]
    if g.size:
        starts = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
        out[g[starts]] = np.add.reduceat(src[gather[order]], starts, axis=0, dtype=np.uint8) & 1
    return out


class Gf2Code:
    """H (and G) as entry lists in file order; the sizes, puncture / shorten lists and bit_pos as the library derives them:
    leading lines with a ':' are the header, dimensions are the largest index + 1, kc = nc - mc."""

    def __init__(self, pc_file, gen_file=""):
        lines = open(pc_file).read().split("\n")
        self.puncture, self.shorten = [], []
        skip = 0
        for line in lines:
            if ":" not in line:
                break
            token, rest = line.split(":", 1)
            if "puncture" in token:
                self.puncture += [int(v) for v in rest.split()]
            elif "shorten" in token:
                self.shorten += [int(v) for v in rest.split()]
            skip += 1
        self.h_rows, self.h_cols = _entries(lines[skip:])
        self.mc, self.nc = int(self.h_rows.max()) + 1, int(self.h_cols.max()) + 1
        self.kc = self.nc - self.mc
        left_out = set(self.puncture) | set(self.shorten)
        self.bit_pos = np.asarray([c for c in range(self.nc) if c not in left_out], np.int64)
        self.nct = self.bit_pos.size
        self.kct = self.nct - (self.mc - len(self.puncture))
        self.has_g = bool(gen_file)
        if self.has_g:
            self.g_rows_idx, self.g_cols_idx = _entries(open(gen_file).read().split("\n"))
            self.g_rows, self.g_cols = int(self.g_rows_idx.max()) + 1, int(self.g_cols_idx.max()) + 1

    def encode(self, info):
        """info[n][kc] (any non-zero = 1) -> codeword[n][nc], column order: codeword[f][j] = XOR of info[f][i] over the
        entries (i, j) of G (an entry listed twice cancels; columns from G.cols on stay 0; no running sum)."""
        u = (np.asarray(info) != 0).astype(np.uint8)
        assert u.ndim == 2 and u.shape[1] == self.kc and self.g_rows <= self.kc
        keep = self.g_cols_idx < self.nc
        return np.ascontiguousarray(_xor_groups(np.ascontiguousarray(u.T), self.g_rows_idx[keep], self.g_cols_idx[keep], self.nc).T)

    def syndrome(self, word):
        """word[n][nc] -> (syndrome[n][mc], weight[n]): XOR of word[f][c] over the entries (r, c) of H."""
        w = (np.asarray(word) != 0).astype(np.uint8)
        assert w.ndim == 2 and w.shape[1] == self.nc
        s = np.ascontiguousarray(_xor_groups(np.ascontiguousarray(w.T), self.h_cols, self.h_rows, self.mc).T)
        return s, s.sum(1, dtype=np.uint32)

    def bit_errors(self, a, b):
        """The transmitted positions at which rows f of a and b differ, uint32 [n]."""
        a, b = np.asarray(a) != 0, np.asarray(b) != 0
        return (a[:, self.bit_pos] != b[:, self.bit_pos]).sum(1, dtype=np.uint32)

    def column_degree(self, c):
        return int((self.h_cols == c).sum())


def pack(bits):
    """[n][L] (any non-zero = 1) -> uint32 [n][ceil(L / 32)]: bit i & 31 of word i >> 5, the unused high bits zero."""
    b = (np.asarray(bits) != 0).astype(np.uint8)
    n, length = b.shape
    words = (length + 31) // 32
    padded = np.zeros((n, words * 32), np.uint8)
    padded[:, :length] = b
    return np.ascontiguousarray(np.packbits(padded.reshape(n, words, 32), axis=2, bitorder="little")).view(np.uint32).reshape(n, words)


def unpack(words, length):
    """The inverse of pack(): uint8 [n][length]."""
    w = np.ascontiguousarray(np.asarray(words, np.uint32))
    return np.ascontiguousarray(np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :length])


def high_bits(words, length):
    """The bits of each row's last word from `length` on (all zero where the layout is kept)."""
    w = np.asarray(words, np.uint32)
    if length % 32 == 0:
        return np.zeros(w.shape[0], np.uint32)
    return w[:, -1] >> np.uint32(length % 32)
