"""Layered min-sum (include/ldpc_amd.h, ldpc_hip_set_min_sum_schedule) without a GPU: the setter's validity check, the
launch stages it reports, and the numpy mirror (tests/layered_minsum_ref.py) by itself.

A code with a check node of degree 1 never reaches the setter: ldpc_hip_create already refuses it, so the setter's own refusal
of such a row (build_layer_plan takes degrees 2..8) cannot be reached through the C ABI, and the test checks the creation
error instead."""
import numpy as np
import pytest

import orc
from layered_minsum_ref import LayeredMinSumMirror
from minsum_common import check_decode_stages, write
from minsum_ref import MinSumMirror


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


def test_setter_accepts_and_rejects(lib, tmp_path, h8k_file):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    assert d.min_sum_schedule == "flooding"  # off by default
    d.set_min_sum_schedule("layered")
    assert d.min_sum_schedule == "layered"
    for bad in (2, -1, 7, "rowwise"):
        with pytest.raises(RuntimeError, match="ldpc_hip_set_min_sum_schedule"):
            d.set_min_sum_schedule(bad)
        assert lib.ldpc_hip_last_error()
        assert d.min_sum_schedule == "layered"  # unchanged
    d.set_min_sum_schedule("flooding")
    assert d.min_sum_schedule == "flooding"
    assert lib.ldpc_hip_set_min_sum_schedule(d.ctx, 1) == 0 and lib.ldpc_hip_set_min_sum_schedule(d.ctx, 0) == 0
    # LDS per frame: 8 nc bytes of totals + 20 bytes per check node, each step rounded up to an even number of nodes
    code = orc.Code(orc.H_TXT)
    n, step_of = code.layer_steps()
    counts = np.bincount(step_of, minlength=n)
    want = (8 * code.nc + 20 * int(((counts + 1) // 2 * 2).sum()) + 15) // 16 * 16
    assert d.layered_min_sum_lds_bytes() == want and 5 * want <= 160 * 1024 < 6 * want  # five frames per CU
    # the 8k (3,6) code: the frame that nearly fills a CU's LDS, and is taken
    d8 = libldpc_amd.HipDecoder(h8k_file)
    assert 140 * 1024 < d8.layered_min_sum_lds_bytes() <= 160 * 1024
    d8.set_min_sum_schedule("layered")
    assert d8.min_sum_schedule == "layered"
    # codes outside what the layered plan takes
    base = [[0, 1, 2], [2, 3, 4], [4, 5, 0], [1, 3, 5]]
    ok = libldpc_amd.HipDecoder(write(tmp_path / "ok.txt", base))
    ok.set_min_sum_schedule("layered")
    cases = {
        "isolated_column": [[0, 1, 2], [2, 3, 5], [5, 6, 0], [1, 3, 6]],  # column 4 has no edge
        "degree9_row": base + [list(range(9))],
        "degree1_row": base + [[3]],
    }
    for name, rows in cases.items():
        path = write(tmp_path / f"{name}.txt", rows)
        if name == "degree1_row":
            # the library takes no such code at all (a check node of degree 1 is undefined in the reference decoder): there is
            # no context to set anything on; should that ever change, the setter's own check (build_layer_plan) still applies
            ctx = lib.ldpc_hip_create(path.encode(), b"", 0)
            if not ctx:
                assert b"degree" in lib.ldpc_hip_last_error()
                continue
            lib.ldpc_hip_destroy(ctx)
        dd = libldpc_amd.HipDecoder(path)
        with pytest.raises(RuntimeError, match="ldpc_hip_set_min_sum_schedule"):
            dd.set_min_sum_schedule("layered")
        assert lib.ldpc_hip_set_min_sum_schedule(dd.ctx, 1) == -1 and len(lib.ldpc_hip_last_error()) > 0, name
        assert dd.min_sum_schedule == "flooding", name
    # beyond 160 KB of LDS: 16384 columns of totals alone are 128 KB, 8192 check nodes another 160 KB
    rows = [[(3 * i + j) % 16384 for j in range(3)] + [(5 * i + 7) % 16384] for i in range(8192)]
    rows = [sorted(set(r)) for r in rows]
    rows += [[c, (c + 1) % 16384] for c in range(0, 16384, 2)]  # every column has an edge
    big = libldpc_amd.HipDecoder(write(tmp_path / "big.txt", rows))
    assert big.layered_min_sum_lds_bytes() > 160 * 1024
    with pytest.raises(RuntimeError, match="LDS"):
        big.set_min_sum_schedule("layered")
    assert big.min_sum_schedule == "flooding"


def test_decode_stages(lib, h8k_file):
    """One `whole` launch for BP_MS while the schedule is set; BP keeps its stages."""
    import libldpc_amd
    for path in (orc.H_TXT, h8k_file):
        check_decode_stages(libldpc_amd.HipDecoder(path), lambda d: d.set_min_sum_schedule("layered"),
                            lambda d: d.set_min_sum_schedule("flooding"))


def _awgn_llrs(code, snr_db, n, seed):
    """All-zero codewords over AWGN with numpy's normals: LLR 2 y / sigma^2, punctured columns 0."""
    rng = np.random.default_rng(seed)
    sigma2 = 10.0 ** (-snr_db / 10.0)
    llr = np.zeros((n, code.nc))
    llr[:, code.bit_pos] = 2.0 * (1.0 + np.sqrt(sigma2) * rng.standard_normal((n, code.nct))) / sigma2
    return llr


def _bits(r):
    return r["iters"].tolist(), r["hard"].tobytes(), r["llr_out"].view(np.uint64).tobytes(), r["bit_errors"].tolist()


def test_mirror_row_order_within_a_step_does_not_matter():
    """The check nodes of a step share no variable node: visiting them together, one by one, or one by one in reversed
    order gives the same bits."""
    code = orc.Code(orc.H_TXT)
    mir = LayeredMinSumMirror(code)
    llr = _awgn_llrs(code, -4.5, 6, seed=1)
    for early, iters in ((True, 50), (False, 8)):
        ref = mir.decode(llr, 1.0, 0.0, early_term=early, iterations=iters)
        fwd = mir.decode(llr, 1.0, 0.0, early_term=early, iterations=iters, row_order="forward")
        rev = mir.decode(llr, 1.0, 0.0, early_term=early, iterations=iters, row_order="reversed")
        assert _bits(ref) == _bits(fwd) == _bits(rev), early
    assert 0 < ref["bit_errors"].max() or ref["iters"].min() < 8


def test_mirror_layered_needs_fewer_sweeps():
    """h.txt, AWGN -3.5 dB, 256 frames, plain min-sum, 50 iterations with early termination: over the frames both
    schedules converge on, mean layered sweeps < 0.7 x mean flooding iterations (0.56 on 1 500 frames)."""
    code = orc.Code(orc.H_TXT)
    llr = _awgn_llrs(code, -3.5, 256, seed=2)
    lay = LayeredMinSumMirror(code).decode(llr)
    flo = MinSumMirror(code).decode(llr)
    both = (lay["iters"] < 50) & (flo["iters"] < 50) & (lay["bit_errors"] == 0) & (flo["bit_errors"] == 0)
    assert both.sum() >= 200
    ratio = lay["iters"][both].mean() / flo["iters"][both].mean()
    print("sweep ratio", ratio, "frames", int(both.sum()))
    assert ratio < 0.7
