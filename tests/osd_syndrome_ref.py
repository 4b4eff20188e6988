"""A numpy mirror of ldpc_hip_osd_syndrome_batch, written from the text of include/ldpc_amd.h on top of osd_ref (matrix,
values, order_of, reduce).  A plain module, numpy only.  The right-hand side rides through osd_ref.reduce as one more column,
r = s + M z, put LAST in the order: if it finds a pivot, r is independent of the columns of M and the frame is infeasible;
otherwise the reduced rows hold in that column what order 0 flips at their pivot columns.  reduce takes the LAST unused row
that offers itself as the pivot, the kernel the first; nothing the contract states depends on that.  The metric of every
candidate is summed from the definition, over the columns where the candidate differs from z (the kernel adds signed
differences from order 0).

Contract (per frame; z, q, M, pi, P, K and the metric as in osd_ref):
  a. M z = s: status CODEWORD, the word is z, metric 0, 0 flips, both columns none.
  b. s outside the column space of M: status INFEASIBLE, the word is z, metric 0, 0 flips, both columns none.
  c. x0 = the unique x with M x = s and x = z on K.
  d. T = min(candidates, |K|): x_t agrees with z on K except at K[t]; candidate index e = t.
  e. L = min(pair_depth, |K|): for t1 < t2 < L, x_{t1,t2} agrees with z on K except at K[t1] and K[t2]; e = T + the
     lexicographic rank of (t1, t2).
  f. The winner is x0 unless a candidate has a strictly smaller metric; the smallest metric wins, then the smallest e.
  g. status ORDER0 / REPROCESSED / REPROCESSED_PAIR; flipped_columns (K[t], none), (K[t1], K[t2]) or (none, none)."""
import numpy as np

import gf2_ref
import osd_ref as osd

CODEWORD, ORDER0, REPROCESSED, REPROCESSED_PAIR, INFEASIBLE = 0, 1, 2, 3, 4
NO_COLUMN = osd.NO_COLUMN
MAX_PAIR_DEPTH = 256
KEYS = ("word", "flips", "metric", "flipped_columns", "status")


def frame(m, z, q, s, settings):
    """One frame for every (candidates, pair_depth) in `settings`:
    {(candidates, pair_depth): (word uint8 [nc], flips, metric, (column, column), status)}."""
    z = z.astype(np.uint8)
    nc = m.shape[1]
    r = (((m.astype(np.int64) @ z.astype(np.int64)) & 1) ^ (np.asarray(s) != 0)).astype(np.uint8)
    nothing = (z, 0, 0, (NO_COLUMN, NO_COLUMN))
    if not r.any():
        return {key: nothing + (CODEWORD,) for key in settings}
    solved, kept, rows = osd.reduce(np.concatenate((m, r[:, None]), axis=1), np.append(osd.order_of(q), nc))
    if solved.size and solved[-1] == nc:
        return {key: nothing + (INFEASIBLE,) for key in settings}
    assert kept[-1] == nc
    kept = kept[:-1]
    e0 = np.zeros(nc, np.uint8)  # x0 + z: nothing on K, the reduced right-hand side at the pivot columns
    e0[solved] = rows[:, nc]
    assert np.array_equal((m.astype(np.int64) @ e0.astype(np.int64)) & 1, r)
    singles = min(max(t for t, _ in settings), kept.size)
    depth = min(max(d for _, d in settings), kept.size)
    # toggles[t] = what flipping K[t] toggles: the column itself and the pivot column of every reduced row that holds it
    toggles = np.zeros((max(singles, depth), nc), np.uint8)
    toggles[np.arange(toggles.shape[0]), kept[:toggles.shape[0]]] = 1
    toggles[:, solved] = rows[:, kept[:toggles.shape[0]]].T
    weight = q.astype(np.int64)
    metric0 = int(weight[e0 == 1].sum())
    single_metric = ((e0[None, :] ^ toggles[:singles]).astype(np.int64) @ weight) if singles else np.zeros(0, np.int64)
    pair_metric = np.zeros((depth, depth), np.int64)
    for t1 in range(depth - 1):
        pair_metric[t1, t1 + 1:] = (e0[None, :] ^ toggles[t1][None, :] ^ toggles[t1 + 1:depth]).astype(np.int64) @ weight
    out = {}
    for key in settings:
        t_count, l_count = min(key[0], kept.size), min(key[1], kept.size)
        a, b = np.triu_indices(l_count, 1)  # (t1, t2) in lexicographic order
        metrics = np.concatenate((single_metric[:t_count], pair_metric[a, b]))
        e, columns, status = e0, (NO_COLUMN, NO_COLUMN), ORDER0
        if metrics.size and metrics.min() < metric0:
            best = int(np.argmin(metrics))  # (the first of the smallest: the smallest candidate index)
            if best < t_count:
                e, columns, status = e0 ^ toggles[best], (int(kept[best]), NO_COLUMN), REPROCESSED
            else:
                t1, t2 = int(a[best - t_count]), int(b[best - t_count])
                e, columns, status = e0 ^ toggles[t1] ^ toggles[t2], (int(kept[t1]), int(kept[t2])), REPROCESSED_PAIR
        out[key] = (z ^ e, int(e.sum()), int(weight[e == 1].sum()), columns, status)
    return out


def decode_many(code, llr, syndrome, settings):
    """The contract on llr[n][nc] and syndrome[n][mc] bytes (None = all zero) for every (candidates, pair_depth) in
    `settings`, sharing each frame's elimination: {(candidates, pair_depth): the dict of decode()}."""
    m = osd.matrix(code)
    z, q = osd.values(llr)
    n = z.shape[0]
    syn = np.zeros((n, code.mc), np.uint8) if syndrome is None else np.asarray(syndrome).reshape(n, code.mc)
    settings = sorted(set((int(t), int(d)) for t, d in settings))
    assert all(d <= MAX_PAIR_DEPTH for _, d in settings)
    per_frame = [frame(m, z[f], q[f], syn[f], settings) for f in range(n)]
    out = {}
    for key in settings:
        r = [pf[key] for pf in per_frame]
        out[key] = {"word": gf2_ref.pack(np.asarray([x[0] for x in r], np.uint8).reshape(n, code.nc)),
                    "flips": np.asarray([x[1] for x in r], np.uint32), "metric": np.asarray([x[2] for x in r], np.uint64),
                    "flipped_columns": np.asarray([x[3] for x in r], np.uint32).reshape(n, 2),
                    "status": np.asarray([x[4] for x in r], np.uint32)}
    return out


def decode(code, llr, syndrome=None, candidates=0, pair_depth=0):
    """The contract of ldpc_hip_osd_syndrome_batch: word (packed, padding bits 0), flips, status (uint32 [n]),
    flipped_columns (uint32 [n][2]) and metric (uint64 [n])."""
    return decode_many(code, llr, syndrome, ((candidates, pair_depth),))[(int(candidates), int(pair_depth))]
