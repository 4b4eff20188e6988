"""Pairs of a parity-check file and a generator file whose generator is known by construction — what the tests of the encoder
and of the decoders' transmitted-codeword paths share (test_generator_codes_host.py, test_gpu_generator_codes.py).  A plain
module, like orc.py and minsum_common.py; numpy only, no import of the library or of the oracle.  Everything is generated
from fixed seeds (crc32 of the pair's name) into a directory the caller names.

Systematic pairs, write_systematic():  H = [A | I_mc | T],  G = [I_k | A^T]
  A is mc x k with prescribed row or column weights, I_mc gives every check node a leaf, T is a tail of `tail` columns listed
  in `shorten`, each joined to two check nodes, which G never touches.  Row i of G is e_i followed by column i of A, so
  H G^T = A + A = 0: every row of G is a codeword.  The tail makes the generator narrower and shorter than the code at once:
  G.cols = k + mc < nc and G.rows = k < kc = nc - mc = k + tail.  `duplicate` writes one entry G does NOT have twice: the
  library's column masks cancel it with ^=, its column walk and the oracle add it twice — the pair encodes like the plain one.

Null-space pairs, write_null_space():  a (dv, dc)-regular H without leaves (the totals-form register kernel refuses
  degree-1 columns) and a few hundred vectors of its null space, found by bit-packed elimination over GF(2), as rows of G
  spread over 0..kc-1.  The rows between them are absent, which the file format and the encoder allow.
"""
import os
import zlib

import numpy as np


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _match_sockets(row_degs, col_degs, rng):
    """Random bipartite graph with these row and column degrees (socket matching, repeated edges repaired by swaps):
    (rows, cols) of the edges, sorted by row then column."""
    assert sum(row_degs) == sum(col_degs)
    rows = np.repeat(np.arange(len(row_degs)), row_degs)
    cols = np.repeat(np.arange(len(col_degs)), col_degs)
    rng.shuffle(cols)
    for _ in range(500):
        key = rows.astype(np.int64) * len(col_degs) + cols
        _, first = np.unique(key, return_index=True)
        dup = np.setdiff1d(np.arange(key.size), first)
        if dup.size == 0:
            break
        other = rng.integers(0, key.size, dup.size)
        cols[dup], cols[other] = cols[other].copy(), cols[dup].copy()
    else:
        raise AssertionError("could not repair repeated edges")
    order = np.lexsort((cols, rows))
    return rows[order], cols[order]


def _balanced(total, n):
    """n degrees that differ by at most one and sum to total."""
    return [total // n + (i < total % n) for i in range(n)]


def systematic_matrix(name, k, mc, row_weights=None, col_weight=None):
    """The edges (rows, cols) of A, mc x k: every column of weight col_weight, or row i of weight row_weights[i % len] (a
    pool dealt round the rows); the other side's degrees balanced."""
    rng = _rng(name)
    if row_weights is not None:
        rdeg = [row_weights[i % len(row_weights)] for i in range(mc)]
        cdeg = _balanced(sum(rdeg), k)
    else:
        cdeg = [col_weight] * k
        rdeg = _balanced(sum(cdeg), mc)
    assert min(rdeg) >= 1 and min(cdeg) >= 1, "every row and column of A takes part"
    return _match_sockets(rdeg, cdeg, rng)


def write_systematic(directory, name, k, mc, tail=0, row_weights=None, col_weight=None, duplicate=False):
    """Files name.h.txt / name.g.txt of H = [A | I | T], G = [I | A^T]; returns (h_path, g_path).  With `duplicate`, the
    A of the pair is that of name without its "_dup" suffix, so that the two pairs differ in the repeated entry alone."""
    base = name[:-4] if name.endswith("_dup") else name
    ar, ac = systematic_matrix(base, k, mc, row_weights, col_weight)
    rng = np.random.default_rng(zlib.crc32((base + "/tail").encode()))
    per_row = [[] for _ in range(mc)]
    for r, c in zip(ar, ac):
        per_row[r].append(int(c))
    for i in range(mc):
        per_row[i].append(k + i)
    tail_cols = [k + mc + t for t in range(tail)]
    for c in tail_cols:
        for r in rng.choice(mc, size=2, replace=False):
            per_row[int(r)].append(c)
    lines = [f"shorten [{tail}]: " + " ".join(map(str, tail_cols))] if tail else []
    lines += [f"{i} {c}" for i, cs in enumerate(per_row) for c in cs]
    h_path = os.path.join(str(directory), name + ".h.txt")
    open(h_path, "w").write("\n".join(lines))
    g = [(i, i) for i in range(k)] + [(int(c), k + int(r)) for r, c in zip(ar, ac)]
    g.sort()
    if duplicate:
        have = set(g)
        extra = next((i, k + j) for i in range(k // 2, k) for j in range(mc // 2, mc) if (i, k + j) not in have)
        g += [extra, extra]
        g.sort()
    g_path = os.path.join(str(directory), name + ".g.txt")
    open(g_path, "w").write("\n".join(f"{r} {c}" for r, c in g))
    return h_path, g_path


def null_space_rows(h_rows, h_cols, mc, nc, n_rows):
    """n_rows independent vectors v with H v = 0, [n_rows, nc] uint8: H is reduced to row echelon form over GF(2) (64 columns
    to a word); every free column f gives the vector with v[f] = 1 and v[pivot column of row i] = entry (i, f)."""
    words = (nc + 63) // 64
    m = np.zeros((mc, words), np.uint64)
    np.bitwise_xor.at(m, (h_rows, h_cols // 64), np.uint64(1) << (h_cols % 64).astype(np.uint64))
    pivots, rk = [], 0
    for c in range(nc):
        if rk == mc:
            break
        w, b = c // 64, np.uint64(c % 64)
        has = ((m[:, w] >> b) & np.uint64(1)).astype(bool)
        below = np.nonzero(has[rk:])[0]
        if below.size == 0:
            continue
        p = rk + int(below[0])
        if p != rk:
            m[[rk, p]] = m[[p, rk]]
            has[[rk, p]] = has[[p, rk]]
        has[rk] = False
        m[has] ^= m[rk]
        pivots.append(c)
        rk += 1
    free = np.setdiff1d(np.arange(nc), pivots)
    assert free.size >= n_rows
    take = free[np.linspace(0, free.size - 1, n_rows).astype(np.int64)]
    out = np.zeros((n_rows, nc), np.uint8)
    out[np.arange(n_rows), take] = 1
    piv = np.asarray(pivots, np.int64)
    for i, f in enumerate(take):
        out[i, piv] = ((m[:rk, f // 64] >> np.uint64(f % 64)) & np.uint64(1)).astype(np.uint8)
    return out


def write_null_space(directory, name, nc, dv, dc, n_rows):
    """Files of a (dv, dc)-regular H and of n_rows null-space vectors as rows 0, ..., kc - 1 (evenly spread) of G; returns
    (h_path, g_path)."""
    assert nc * dv % dc == 0
    mc = nc * dv // dc
    hr, hc = _match_sockets([dc] * mc, [dv] * nc, _rng(name))
    h_path = os.path.join(str(directory), name + ".h.txt")
    open(h_path, "w").write("\n".join(f"{r} {c}" for r, c in zip(hr, hc)))
    vecs = null_space_rows(hr, hc, mc, nc, n_rows)
    kc = nc - mc
    row_of = np.linspace(0, kc - 1, n_rows).astype(np.int64)  # (the last one is kc - 1: G.rows == kc)
    assert np.unique(row_of).size == n_rows
    vi, vj = np.nonzero(vecs)
    g_path = os.path.join(str(directory), name + ".g.txt")
    open(g_path, "w").write("\n".join(f"{row_of[i]} {j}" for i, j in zip(vi, vj)))
    return h_path, g_path


# ---- the pairs the tests use: name -> (builder arguments, what test_generator_codes_host.py holds them to) ----
# encoder path: "dense<W>" = encode_cw_dense_kernel<W> (sim_kernels.hip), "walk" = encode_cw_kernel
SYSTEMATIC = {
    # name: dict(k, mc, tail, weights), expected (nc, mc, kc, g_rows, g_cols, encoder path)
    "s40x60": (dict(k=40, mc=60, col_weight=3), (100, 60, 40, 40, 100, "dense1")),
    "s64x100": (dict(k=64, mc=100, col_weight=3), (164, 100, 64, 64, 164, "dense1")),
    "s129x150t5": (dict(k=129, mc=150, tail=5, col_weight=3), (284, 150, 134, 129, 279, "dense3")),
    "s256x1792": (dict(k=256, mc=1792, row_weights=[1, 2]), (2048, 1792, 256, 256, 2048, "dense4")),
    "s200x1849": (dict(k=200, mc=1849, row_weights=[1, 2]), (2049, 1849, 200, 200, 2049, "walk")),
    "s257x200": (dict(k=257, mc=200, col_weight=3), (457, 200, 257, 257, 457, "walk")),
    "s300x250t3": (dict(k=300, mc=250, tail=3, row_weights=[2, 3, 4, 5, 6]), (553, 250, 303, 300, 550, "walk")),
    "s40x60_dup": (dict(k=40, mc=60, col_weight=3, duplicate=True), (100, 60, 40, 40, 100, "dense1")),
    # the decoder residencies (with s300x250t3: LDS-resident, not fused)
    "s192x128": (dict(k=192, mc=128, row_weights=[3]), (320, 128, 192, 192, 320, "dense3")),
    "s6000x3600": (dict(k=6000, mc=3600, row_weights=[5]), (9600, 3600, 6000, 6000, 9600, "walk")),
    "s800x100": (dict(k=800, mc=100, row_weights=[8, 11, 15, 19]), (900, 100, 800, 800, 900, "walk")),
}
NULL_SPACE = {
    # name: dict(nc, dv, dc, n_rows), expected (nc, mc, kc, g_rows, encoder path); g_cols is whatever the vectors reach
    "n7200": (dict(nc=7200, dv=3, dc=6, n_rows=200), (7200, 3600, 3600, 3600, "walk")),
}
ENCODER_PAIRS = ("s40x60", "s64x100", "s129x150t5", "s256x1792", "s200x1849", "s257x200", "s300x250t3", "s40x60_dup")
COUNTER_PAIRS = ("s40x60", "s129x150t5", "s257x200")
SHARDED_PAIRS = ("s300x250t3", "s129x150t5")

# the decoder cases: residency -> (pair, register form, fused, sliced erasure kernel,
#                                  channel points {case: x}; chosen in test_generator_codes_host.py)
FRAMES, SEED, SKIP = 8, 7, 3
DECODERS = {
    "lds": ("s300x250t3", None, False, True),
    "lds_fused": ("s192x128", None, True, True),
    "registers_messages": ("s6000x3600", "messages", False, False),
    "registers_totals": ("n7200", "totals", False, False),
    "memory": ("s800x100", None, False, True),
}
# (channel, decoding, early termination, iterations, erasure compatibility) of the parity cases
CASES = {
    "bp_early": ("AWGN", "BP", True, 50, False),
    "bp_full": ("AWGN", "BP", False, 12, False),
    "min_sum": ("AWGN", "BP_MS", True, 50, False),
    "bsc": ("BSC", "BP", True, 50, False),
    "bec": ("BEC", "BP", True, 50, False),
    "bec_compat": ("BEC", "BP", True, 50, True),
}


def encoder_path(nc, kc, g_rows):
    """Which kernel launch_encode_codewords (sim_kernels.hip) takes, from sizes alone: the column masks exist iff
    ceil(kc / 64) <= 4 and G.rows <= kc (engine.cpp), the dense kernel provides for nc <= 8 * 256 columns."""
    words = (kc + 63) // 64
    return f"dense{words}" if words <= 4 and nc <= 2048 and g_rows <= kc else "walk"


def write_pair(directory, name):
    if name in SYSTEMATIC:
        return write_systematic(directory, name, **SYSTEMATIC[name][0])
    return write_null_space(directory, name, **NULL_SPACE[name][0])


# ---- the opt-in min-sum settings: name -> (channel, the residencies whose pair the setting takes) ----
OPT_IN = {
    "corrected": ("AWGN", ("lds", "lds_fused", "registers_messages", "registers_totals", "memory")),
    "layered": ("AWGN", ("lds", "lds_fused", "registers_messages", "registers_totals")),  # (memory: a check node wider than 8)
    "quantized": ("AWGN", ("lds", "lds_fused", "registers_messages", "registers_totals", "memory")),
    "ternary": ("BSC", ("lds", "lds_fused", "memory")),  # (the register-size codes: 32 frames do not fit LDS)
}
OPT_IN_ITERATIONS = 30


def switch_on(dec, setting):
    """Puts the opt-in `setting` in force on a HipDecoder (raises where the code is not taken)."""
    if setting == "corrected":
        dec.set_min_sum_correction(0.8125, 0)
    elif setting == "layered":
        dec.set_min_sum_schedule("layered")
    elif setting == "quantized":
        dec.set_min_sum_quantization(6, 0.25)
    else:
        dec.set_min_sum_ternary(1)


def switch_off(dec):
    dec.set_min_sum_correction()
    dec.set_min_sum_schedule("flooding")
    dec.set_min_sum_quantization(0)
    dec.set_min_sum_ternary(0)


def mirror_decode(code, setting, llr_in, codeword, early=True, iterations=OPT_IN_ITERATIONS):
    """The numpy mirror of `setting` (as switch_on sets it) on llr_in with the transmitted codewords."""
    from layered_minsum_ref import LayeredMinSumMirror
    from minsum_ref import MinSumMirror
    from quantized_minsum_ref import QuantizedMinSumMirror
    from ternary_ref import TernaryMirror
    kw = dict(early_term=early, iterations=iterations, codeword=codeword)
    if setting == "corrected":
        return MinSumMirror(code).decode(llr_in, 0.8125, 0.0, **kw)
    if setting == "layered":
        return LayeredMinSumMirror(code).decode(llr_in, **kw)
    if setting == "quantized":
        return QuantizedMinSumMirror(code).decode(llr_in, 6, 0.25, **kw)
    return TernaryMirror(code).decode(llr_in, 1, **kw)


# ---- channel points: residency -> {case or setting: x}, chosen with the oracle (and the mirrors) alone so that the FRAMES
# frames from SKIP on of seed SEED hold frames that converge without a bit error on a non-zero codeword AND frames with bit
# errors (test_generator_codes_host.py asserts it and prints the counts) ----
# Oracle / mirror counts at these points, converged / failed of 8 frames, in the order of the entries below:
#   lds                 2/6 2/6 2/6 6/2 6/2 7/1 | 2/6 2/6 2/6 1/7      lds_fused           5/3 5/3 5/3 5/3 6/2 7/1 | 3/5 5/3 5/3 1/7
#   registers_messages  4/4 4/4 4/4 4/4 2/5 4/2 | 4/4 4/4 3/5          registers_totals    7/1 7/1 7/1 5/3 4/4 4/4 | 7/1 7/1 7/1
#   memory              2/6 2/6 4/4 3/5 5/3 5/2 | 2/6 4/4 3/5          (the registers / messages pair fails every frame at 4 dB)
POINTS = {
    "lds": {"bp_early": 3.0, "bp_full": 3.0, "min_sum": 3.0, "bsc": 0.02, "bec": 0.2, "bec_compat": 0.2,
            "corrected": 3.0, "layered": 3.0, "quantized": 3.0, "ternary": 0.01},
    "lds_fused": {"bp_early": 4.0, "bp_full": 4.0, "min_sum": 4.0, "bsc": 0.02, "bec": 0.1, "bec_compat": 0.1,
                  "corrected": 4.0, "layered": 4.0, "quantized": 4.0, "ternary": 0.01},
    "registers_messages": {"bp_early": 5.5, "bp_full": 5.5, "min_sum": 5.5, "bsc": 0.005, "bec": 0.1, "bec_compat": 0.1,
                           "corrected": 6.0, "layered": 5.5, "quantized": 5.5},
    "registers_totals": {"bp_early": 1.5, "bp_full": 2.0, "min_sum": 2.0, "bsc": 0.084, "bec": 0.42, "bec_compat": 0.42,
                         "corrected": 1.6, "layered": 2.0, "quantized": 2.0},
    "memory": {"bp_early": 7.0, "bp_full": 7.0, "min_sum": 7.0, "bsc": 0.004, "bec": 0.03, "bec_compat": 0.05,
               "corrected": 7.0, "quantized": 7.0, "ternary": 0.004},
}


def mixed(iters, bit_errors, codeword, early, iterations):
    """(frames that converge without a bit error on a non-zero codeword, frames with bit errors, frames whose codeword is not
    all-zero); without early termination every frame runs all iterations and "converges" means no bit error."""
    nz = np.asarray(codeword).any(axis=1)
    be, it = np.asarray(bit_errors), np.asarray(iters)
    good = (be == 0) & nz & ((it < iterations) if early else True)
    return int(good.sum()), int((be > 0).sum()), int(nz.sum())


def check_mixed(iters, bit_errors, codeword, early, iterations, what):
    good, bad, nz = mixed(iters, bit_errors, codeword, early, iterations)
    assert good >= 1 and bad >= 1 and nz > 0.9 * len(np.asarray(iters)), (what, good, bad, nz)
    return good, bad, nz
