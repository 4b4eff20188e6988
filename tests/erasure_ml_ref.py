"""numpy mirrors of ldpc_hip_erasure_solve_batch, written from the text of include/ldpc_amd.h on top of erasure_ref.incidence:
solve() by Gauss-Jordan elimination over GF(2), and solve_by_enumeration() from the definition alone — all 2^|E| assignments of
the erased columns, those with zero syndrome kept.  A plain module, numpy only.  solve() takes the unknowns from the last to
the first and the last row that offers itself as the pivot; the kernel takes the first of both: what the two agree on does
not depend on the order of the pivots.  test_erasure_solve_host.py holds the two functions against each other;
test_gpu_erasure_solve.py holds the kernel to solve() bit for bit."""
import numpy as np

import erasure_ref as er
import gf2_ref

SOLVED, PARTIAL, INCONSISTENT, TOO_LARGE = 0, 1, 2, 3


def matrix(code):
    """M[mc][nc] over GF(2): an entry of H listed twice cancels."""
    return (er.incidence(code) & 1).astype(np.uint8)


def _reduce(a):
    """The reduced row echelon form of a[rows][k + 1] (k unknowns and the right-hand side; 0 / 1 bytes) and its rank over
    the first k columns.  Rows are packed 64 columns to a word for the XORs."""
    rows, k = a.shape[0], a.shape[1] - 1
    words = (k + 1 + 63) // 64
    padded = np.zeros((rows, 64 * words), np.uint8)
    padded[:, :k + 1] = a
    p = np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(rows, words)
    used = np.zeros(rows, bool)
    rank = 0
    for j in range(k - 1, -1, -1):
        has = ((p[:, j >> 6] >> np.uint64(j & 63)) & np.uint64(1)).astype(bool)
        offers = np.flatnonzero(has & ~used)
        if offers.size == 0:
            continue
        pivot = offers[-1]
        used[pivot] = True
        rank += 1
        has[pivot] = False
        p[has] ^= p[pivot]
    out = np.unpackbits(p.view(np.uint8).reshape(rows, 8 * words), axis=1, bitorder="little")[:, :k + 1]
    return out, rank


def _inputs(word, erased):
    e = np.asarray(erased) != 0
    return (np.asarray(word) != 0) & ~e, e


def _packed(v, e, unresolved, rank, status):
    return {"word": gf2_ref.pack(v), "erased": gf2_ref.pack(e), "unresolved": np.asarray(unresolved, np.uint32),
            "rank": np.asarray(rank, np.uint32), "status": np.asarray(status, np.uint32)}


def solve(code, word, erased, max_unknowns):
    """The contract of ldpc_hip_erasure_solve_batch on word[n][nc], erased[n][nc] (any non-zero = 1): a dict of word and
    erased (packed, padding bits 0), unresolved, rank and status (uint32 [n])."""
    assert max_unknowns > 0
    m = matrix(code).astype(np.int64)
    v, e = _inputs(word, erased)
    v, e = v.copy(), e.copy()
    n = e.shape[0]
    rank, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for f in range(n):
        cols = np.flatnonzero(e[f])
        if cols.size > min(max_unknowns, code.nc):
            status[f] = TOO_LARGE
            continue
        rhs = (m @ v[f].astype(np.int64)) & 1  # (every check node, those without an erased column included)
        red, rank[f] = _reduce(np.concatenate([m[:, cols], rhs[:, None]], 1).astype(np.uint8))
        unknowns, rhs = red[:, :-1], red[:, -1]
        weight = unknowns.sum(1)
        if ((weight == 0) & (rhs == 1)).any():
            status[f] = INCONSISTENT
            continue
        single = np.flatnonzero(weight == 1)  # a row with one unknown left determines it
        found = cols[np.argmax(unknowns[single], 1)] if single.size else np.zeros(0, np.int64)
        e[f, found] = False
        v[f, found] = rhs[single] == 1
        status[f] = SOLVED if found.size == cols.size else PARTIAL
    return _packed(v, e, e.sum(1), rank, status)


def solve_by_enumeration(code, word, erased, max_unknowns):
    """The same contract from the definition: S is found by trying every assignment of the erased columns; the rank is
    |E| - log2 of the number of assignments x with M x = 0 on the erased columns alone."""
    assert max_unknowns > 0
    m = matrix(code).astype(np.int64)
    v, e = _inputs(word, erased)
    v, e = v.copy(), e.copy()
    n = e.shape[0]
    rank, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for f in range(n):
        cols = np.flatnonzero(e[f])
        k = cols.size
        if k > min(max_unknowns, code.nc):
            status[f] = TOO_LARGE
            continue
        assert k <= 16, "enumeration is for small frames"
        tries = ((np.arange(2 ** k)[:, None] >> np.arange(k)[None, :]) & 1).astype(np.int64)  # [2^k][k]
        homogeneous = (tries @ m[:, cols].T) & 1                                                   # [2^k][mc]
        kernel = int((~homogeneous.any(1)).sum())
        assert kernel & (kernel - 1) == 0
        rank[f] = k - (kernel.bit_length() - 1)
        syndrome = (homogeneous + ((m @ v[f].astype(np.int64)) & 1)[None, :]) & 1
        s = tries[~syndrome.any(1)]
        if s.shape[0] == 0:
            status[f] = INCONSISTENT
            continue
        assert s.shape[0] == kernel
        agree = (s == s[0]).all(0)
        e[f, cols[agree]] = False
        v[f, cols[agree]] = s[0, agree] == 1
        status[f] = SOLVED if agree.all() else PARTIAL
    return _packed(v, e, e.sum(1), rank, status)
