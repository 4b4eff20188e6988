"""What the tests of the min-sum variants (layered: test_*layered_min_sum*.py, quantized: test_*quantized_min_sum*.py) and
of the decoder choice share: comparing results bit for bit, dumping a stream's LLRs, the split-batch and the no-iteration
checks, writing a small parity-check file, and the launch stages while a variant is on.  A plain module, like orc.py."""
import numpy as np

WANT = ("iters", "hard", "llr_out", "bit_errors")


def same(r, m, what, rows=slice(None)):
    """Results r equal rows `rows` of the results m: iters, hard, bit_errors, and llr_out as uint64."""
    for k in WANT:
        a, b = r[k], np.asarray(m[k])[rows].astype(r[k].dtype)
        if k == "llr_out":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (what, k)


def dumped(d, switch_off, ch, x, n, seed=3):
    """llr_in of n frames of the reference stream, dumped with the variant switched off (switch_off(d)) and plain min-sum."""
    switch_off(d)
    d.set_min_sum_correction()
    d.stream_begin(ch, seed, x)
    return d.stream_decode(n, decoding="BP_MS", want=("llr_in",))["llr_in"]


def against_mirror(settings, runs, decode, mirror):
    """decode(setting, early, iterations) against mirror(setting, early, iterations) for every setting (a tuple) and every
    (early, iterations) of runs; returns the mirror's results by setting + (early,)."""
    out = {}
    for st in settings:
        for early, iters in runs:
            m = out[st + (early,)] = mirror(st, early, iters)
            same(decode(st, early, iters), m, (st, early))
    return out


def check_split_batch(run, llr, cut=20):
    """run(llr) equals run on the first `cut` frames followed by run on the rest; returns run(llr)."""
    one = run(llr)
    a, b = run(llr[:cut]), run(llr[cut:])
    for k in WANT:
        assert np.array_equal(np.concatenate((a[k], b[k])), one[k]), k
    return one


def check_no_iteration(z):
    """Results of a decode with iterations = 0: decisions, outputs and counts all zero."""
    assert not z["hard"].any() and not z["llr_out"].view(np.uint64).any() and not z["iters"].any()
    assert np.array_equal(z["bit_errors"], np.zeros(len(z["iters"]), np.uint32))


def write(path, rows):
    """rows: list of column lists -> a parity-check file of "row col" lines."""
    open(path, "w").write("\n".join(f"{i} {c}" for i, cs in enumerate(rows) for c in cs))
    return str(path)


def check_decode_stages(d, switch_on, switch_off):
    """One `whole` launch for BP_MS while the variant is on; BP keeps its stages; everything back when it is off."""
    before = {(dec, early, it): d.decode_stages(early, it, dec) for dec in ("BP", "BP_MS") for early in (True, False)
              for it in (50, 0)}
    switch_on(d)
    for (dec, early, it), st in before.items():
        now = d.decode_stages(early, it, dec)
        if dec == "BP_MS":
            assert now == ["whole"], (early, it)
        else:
            assert now == st, (early, it)
    switch_off(d)
    assert all(d.decode_stages(e, i, dec) == st for (dec, e, i), st in before.items())
