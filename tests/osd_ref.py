"""A numpy mirror of ldpc_hip_osd_batch, written from the text of include/ldpc_amd.h on top of erasure_ref.incidence: the
contract restated step by step, and order0_by_enumeration() from the definition alone for codes small enough to list every
codeword.  A plain module, numpy only.  Rows are packed 64 columns to a word for the XORs; the pivot of a column is the LAST
unused row that offers itself, the kernel takes the first: what the two agree on does not depend on the order of the pivots.
The metric of every candidate is summed from the definition (the kernel adds up signed differences from order 0).
test_osd_host.py holds the mirror against enumeration and against the identities of the header; test_gpu_osd.py holds the
kernel to decode() bit for bit.

Contract (per frame; everything after step 1 is integer or GF(2) arithmetic):
  1. W[c] = the element widened exactly to binary64 (int8: the integer itself); z[c] = (W[c] <= 0), a NaN gives 0;
     q[c] = min(floor(|W[c]| * 4096), 2^31 - 1), a NaN gives 0, an infinity 2^31 - 1.
  2. M[r][c] = the number of times (r, c) is listed in H, mod 2.
  3. The order pi: the columns by (q ascending, column index ascending).
  4. Scan pi: a column joins P iff its column of M is independent of those already in P; K = the others, in the order of pi.
  5. x0 = the unique x with M x = 0 and x = z on K.
  6. metric(x) = the sum of q over the columns where x != z.
  7. For the t-th column j of K, t < min(candidates, |K|): x_j = the solution that agrees with z on K except at j.  The winner
     is x0 unless some x_j has a strictly smaller metric; the smallest metric wins, among equal metrics the smallest t.
  8. word = the winner, flips = the columns where it differs from z, metric, flipped_column = j or 0xFFFFFFFF,
     status = CODEWORD if M z = 0, else REPROCESSED if an x_j won, else ORDER0."""
import numpy as np

import erasure_ref as er
import gf2_ref

CODEWORD, ORDER0, REPROCESSED = 0, 1, 2
NO_COLUMN = 0xFFFFFFFF
Q_MAX = 2**31 - 1
KEYS = ("word", "flips", "metric", "flipped_column", "status")


def matrix(code):
    """M[mc][nc] over GF(2): an entry of H listed twice cancels."""
    return (er.incidence(code) & 1).astype(np.uint8)


def values(llr):
    """(z, q) of llr[n][nc] of dtype float64, float32, float16 or int8: uint8 and int64 [n][nc]."""
    w = np.asarray(llr).astype(np.float64)  # exact for every one of the four
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.floor(np.abs(w) * 4096.0)
    q = np.where(np.isnan(s), 0.0, np.minimum(s, float(Q_MAX))).astype(np.int64)
    return (w <= 0).astype(np.uint8), q


def order_of(q):
    """pi of one frame: by (q, column)."""
    return np.lexsort((np.arange(q.size), q))


def _pack_rows(m):
    rows, nc = m.shape
    words = (nc + 63) // 64
    padded = np.zeros((rows, 64 * words), np.uint8)
    padded[:, :nc] = m
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(rows, words)


def _unpack_rows(p, nc):
    return np.unpackbits(np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1), axis=1, bitorder="little")[:, :nc]


def reduce(m, order):
    """Gauss-Jordan over the columns in `order`: (solved, kept, rows) — the columns of P and of K in the order met, and
    rows[i][nc] = the reduced row whose pivot is solved[i] (it holds solved[i], no other column of P, and its part on K)."""
    p = _pack_rows(m)
    used = np.zeros(m.shape[0], bool)
    solved, kept, pivots = [], [], []
    for c in order:
        has = ((p[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1)).astype(bool)
        offers = np.flatnonzero(has & ~used)
        if offers.size == 0:
            kept.append(c)
            continue
        pivot = offers[-1]
        used[pivot] = True
        has[pivot] = False
        p[has] ^= p[pivot]
        solved.append(c)
        pivots.append(pivot)
    rows = _unpack_rows(p[np.asarray(pivots, np.int64)], m.shape[1]) if pivots else np.zeros((0, m.shape[1]), np.uint8)
    return np.asarray(solved, np.int64), np.asarray(kept, np.int64), rows


def frame(m, z, q, candidates):
    """One frame, for every T in `candidates`: {T: (word uint8 [nc], flips, metric, flipped_column, status)}."""
    z = z.astype(np.uint8)
    is_codeword = not ((m.astype(np.int64) @ z.astype(np.int64)) & 1).any()
    solved, kept, rows = reduce(m, order_of(q))
    x0 = z.copy()
    if solved.size:
        x0[solved] = (rows[:, kept].astype(np.int64) @ z[kept].astype(np.int64)) & 1
    assert not ((m.astype(np.int64) @ x0.astype(np.int64)) & 1).any()

    def metric(x):
        return int(q[x != z].sum())

    out = {}
    tried = []  # (metric, word) of x_j for the t-th column of K, filled as far as the largest T asks
    for cap in sorted(set(int(t) for t in candidates)):
        for t in range(len(tried), min(cap, kept.size)):
            j = kept[t]
            x = x0.copy()
            x[j] ^= 1
            x[solved[rows[:, j] == 1]] ^= 1
            tried.append((metric(x), x))
        best, word, column = metric(x0), x0, NO_COLUMN
        for t in range(min(cap, kept.size)):
            if tried[t][0] < best:  # (strictly: among equal metrics the smallest t stays)
                best, word, column = tried[t][0], tried[t][1], int(kept[t])
        status = CODEWORD if is_codeword else REPROCESSED if column != NO_COLUMN else ORDER0
        out[cap] = (word, int((word != z).sum()), best, column, status)
    return out


def decode_many(code, llr, candidates):
    """The contract on llr[n][nc] for every T in `candidates`, sharing each frame's elimination: {T: the dict of decode()}."""
    m = matrix(code)
    z, q = values(llr)
    n = z.shape[0]
    caps = sorted(set(int(t) for t in candidates))
    per_frame = [frame(m, z[f], q[f], caps) for f in range(n)]
    out = {}
    for cap in caps:
        r = [pf[cap] for pf in per_frame]
        out[cap] = {"word": gf2_ref.pack(np.asarray([x[0] for x in r], np.uint8).reshape(n, code.nc)),
                    "flips": np.asarray([x[1] for x in r], np.uint32), "metric": np.asarray([x[2] for x in r], np.uint64),
                    "flipped_column": np.asarray([x[3] for x in r], np.uint32), "status": np.asarray([x[4] for x in r], np.uint32)}
    return out


def decode(code, llr, candidates):
    """The contract of ldpc_hip_osd_batch on llr[n][nc]: word (packed, padding bits 0), flips, flipped_column, status (uint32
    [n]) and metric (uint64 [n])."""
    return decode_many(code, llr, (candidates,))[int(candidates)]


def codewords(m):
    """Every x with M x = 0, uint8 [count][nc] (nc <= 16)."""
    nc = m.shape[1]
    assert nc <= 16
    x = ((np.arange(2**nc)[:, None] >> np.arange(nc)[None, :]) & 1).astype(np.int64)
    return x[~((x @ m.T.astype(np.int64)) & 1).any(1)].astype(np.uint8)


def solved_set_by_rank(m, order):
    """(P, K) from the definition: a column joins P iff it raises the rank of the columns taken so far, the rank counted from
    the number of solutions (nc <= 16 and mc small)."""
    def rank(cols):
        if not cols:
            return 0
        sub = m[:, cols].astype(np.int64)
        x = ((np.arange(2**len(cols))[:, None] >> np.arange(len(cols))[None, :]) & 1).astype(np.int64)
        kernel = int((~((x @ sub.T) & 1).any(1)).sum())
        return len(cols) - (kernel.bit_length() - 1)

    solved, kept = [], []
    for c in order:
        (solved if rank(solved + [int(c)]) > len(solved) else kept).append(int(c))
    return solved, kept
