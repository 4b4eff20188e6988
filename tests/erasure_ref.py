"""numpy mirrors of ldpc_hip_erasure_channel_batch and ldpc_hip_erasure_decode_batch, written from the text of
include/ldpc_amd.h on top of philox_ref.py and gf2_ref.Gf2Code, and beside them an independent message-passing erasure
decoder with per-edge messages over {0, 1, erased}: decoder.cpp:91-192 of the reference without its genie (a variable node
never looks at the transmitted bit; an erased variable node of degree 1 sends an erasure).  A plain module, numpy only.
test_erasure_batch_host.py holds the two decoders against each other pass by pass; test_gpu_erasure_batch.py holds the
kernels to the mirror bit for bit."""
import numpy as np

import gf2_ref
import philox_ref

EARLY_TERM, STOP_STALLED = 1, 2


def nct(code):
    """The transmitted positions the library counts: nc - |puncture| - |shorten|, at most the entries of bit_pos (a column
    in both lists leaves bit_pos longer)."""
    return min(code.nc - len(code.puncture) - len(code.shorten), len(code.bit_pos))


def channel(code, eps, seed, frames, codeword=None):
    """(word, erased), bool [n][nc]: the contract of ldpc_hip_erasure_channel_batch for the frames `frames`."""
    n = len(frames)
    t = nct(code)
    cw = np.zeros((n, code.nc), bool) if codeword is None else np.asarray(codeword) != 0
    erased = np.zeros((n, code.nc), bool)
    erased[:, code.bit_pos[:t]] = philox_ref.draws(seed, np.asarray(frames, np.uint64), t, eps)
    for c in code.puncture:  # a column in both lists counts as shortened: known
        if 0 <= c < code.nc and c not in code.shorten:
            erased[:, c] = True
    return cw & ~erased, erased


def repeat_entries(h_file, out_file, which=(0, 7, 7)):
    """A copy of a parity-check file with the entries `which` (indices into its entry lines) listed once more each: two
    edges between one check node and one column, and three."""
    lines = open(h_file).read().split("\n")
    entries = [line for line in lines if ":" not in line and line.strip()]
    open(out_file, "w").write("\n".join(lines + [entries[i] for i in which]))
    return out_file


def incidence(code):
    """A[mc][nc], the number of times (r, c) is listed in H."""
    a = np.zeros((code.mc, code.nc), np.int32)
    np.add.at(a, (code.h_rows, code.h_cols), 1)
    return a


def decode(code, word, erased, iterations=50, flags=EARLY_TERM, trace=None):
    """The contract of ldpc_hip_erasure_decode_batch on word[n][nc], erased[n][nc] (any non-zero = 1): a dict of word and
    erased (bool [n][nc]), iters and unresolved (uint32 [n]).  trace: a list that receives (E, V) after every pass."""
    a = incidence(code).astype(np.float32)  # (counts far below 2^24: the products are exact, and BLAS does them)
    e = np.asarray(erased) != 0
    v = (np.asarray(word) != 0) & ~e
    n = e.shape[0]
    early, stalled = bool(flags & EARLY_TERM), bool(flags & STOP_STALLED)
    active = np.full(n, iterations > 0)
    iters = np.zeros(n, np.uint32)
    for _ in range(iterations):
        if not active.any():
            break
        count = e.astype(np.float32) @ a.T                      # erased edges of every check node
        one = count == 1                                         # c0 & ~c1
        xa = ((v.astype(np.float32) @ a.T).astype(np.int64) & 1).astype(bool)
        res = (one.astype(np.float32) @ a) > 0
        val = ((one & xa).astype(np.float32) @ a) > 0
        moved = e & res & active[:, None]
        e = e & ~moved
        v = v | (moved & val)
        holds = e.any(1)
        iters += (active & holds) if early else active
        active = active & (holds if early else True) & (moved.any(1) if stalled else True)
        if trace is not None:
            trace.append((e.copy(), v.copy()))
    return {"word": v, "erased": e, "iters": iters, "unresolved": e.sum(1, dtype=np.uint32)}


def decode_packed(code, word, erased, iterations=50, flags=EARLY_TERM):
    """decode() with the outputs as the library returns them: word and erased packed, padding bits 0."""
    r = decode(code, word, erased, iterations, flags)
    return {"word": gf2_ref.pack(r["word"]), "erased": gf2_ref.pack(r["erased"]), "iters": r["iters"], "unresolved": r["unresolved"]}


ERASED = 2  # a message: 0, 1 or ERASED


def _per_node(index, size, values):
    """[n][size]: the sum of values[n][edges] over the edges of every node (a node without edges: 0)."""
    out = np.zeros((size, values.shape[0]), np.int64)
    np.add.at(out, index, values.T)
    return out.T


def message_passing(code, word, erased, passes):
    """Flooding message passing with one message per edge and direction, decoder.cpp:91-192 without the genie.  Per pass:
    check node, edge j: erased if another input is erased, else the XOR of the others; variable node whose received symbol
    is known: every output and its value are that symbol; received symbol erased: its value is a known input if there is
    one (the OR of the known inputs where they disagree), else erased; its output on edge j the same over the OTHER inputs —
    for degree 1 therefore an erasure.  Returns [(E, V)] after each pass: the nodes still erased, the values of the others."""
    rows, cols = code.h_rows, code.h_cols
    se = np.asarray(erased) != 0
    sv = (np.asarray(word) != 0) & ~se
    v2c = np.where(se[:, cols], ERASED, sv[:, cols].astype(np.int8)).astype(np.int8)  # decoder.cpp:96-99
    out = []
    for _ in range(passes):
        is_e = v2c == ERASED
        bit = np.where(is_e, 0, v2c).astype(np.int64)
        n_e = _per_node(rows, code.mc, is_e.astype(np.int64))[:, rows]
        x = _per_node(rows, code.mc, bit)[:, rows] & 1
        c2v = np.where((n_e - is_e) > 0, ERASED, x ^ bit).astype(np.int8)
        known = c2v != ERASED
        ones = known & (c2v == 1)
        k_node, o_node = _per_node(cols, code.nc, known.astype(np.int64)), _per_node(cols, code.nc, ones.astype(np.int64))
        k_other, o_other = k_node[:, cols] - known, o_node[:, cols] - ones
        from_others = np.where(k_other > 0, (o_other > 0).astype(np.int8), ERASED)
        v2c = np.where(se[:, cols], from_others, sv[:, cols].astype(np.int8)).astype(np.int8)
        e = se & (k_node == 0)
        v = np.where(se, o_node > 0, sv) & ~e
        out.append((e, v))
    return out
