"""Ternary min-sum (include/ldpc_amd.h, ldpc_hip_set_min_sum_ternary) without a GPU: the setter and what it refuses (how it
excludes the other variants: test_layered_fixed_min_sum_host.py), the decoder choice and launch stages it reports, and the
numpy mirror (tests/ternary_ref.py) by itself — its symmetry, what it decodes, and h.txt, where it cannot start."""
import os
import sys

import numpy as np
import pytest

import orc
from minsum_common import check_decode_stages, write
from ternary_ref import CASES, TernaryMirror, flipped_llrs, received

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


def regular_code(tmp_path, nc, dv, dc, seed):
    import gen_regular_code
    path = tmp_path / f"r{nc}_{dv}_{dc}_{seed}.txt"
    path.write_text(gen_regular_code.generate(nc, dv, dc, seed))
    return str(path)


def _lds_bytes(code):
    """The formula beside ldpc_hip_ternary_lds_bytes."""
    vdeg = int(np.bincount(code.edge_col, minlength=code.nc).max())
    planes = 1 + (vdeg + 7).bit_length()
    words = 64 + 2 * max(code.nnz, code.nc) + 3 * code.nc + planes * code.nc
    return (4 * words + 4 * code.nnz + 15) // 16 * 16


def test_setter_and_codes(lib, tmp_path, h8k_file):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    assert d.min_sum_ternary == 0  # off by default
    for w in range(8):
        d.set_min_sum_ternary(w)
        assert d.min_sum_ternary == w
    d.set_min_sum_ternary(3)
    for w in (-1, 8):
        with pytest.raises(RuntimeError, match="ldpc_hip_set_min_sum_ternary"):
            d.set_min_sum_ternary(w)
        assert lib.ldpc_hip_set_min_sum_ternary(d.ctx, w) == -1 and b"ldpc_hip_set_min_sum_ternary" in lib.ldpc_hip_last_error()
        assert d.min_sum_ternary == 3  # unchanged
    d.set_min_sum_ternary()
    assert d.min_sum_ternary == 0
    # the codes it takes: h.txt (degree-15 columns, leaves, punctured columns), the two regular codes of the mirror tests,
    # a column of degree 56, an isolated column
    star = lambda n: [[0, i + 1] for i in range(n)]  # column 0 has degree n
    taken = [orc.H_TXT] + [regular_code(tmp_path, *c[:4]) for c in CASES.values()]
    taken += [write(tmp_path / "deg56.txt", star(56)), write(tmp_path / "isolated.txt", [[0, 1, 2], [2, 3, 5], [5, 6, 0], [1, 3, 6]])]
    for path in taken:
        dd = libldpc_amd.HipDecoder(path)
        assert 0 < dd.ternary_lds_bytes() <= 160 * 1024, path
        assert dd.ternary_lds_bytes() == _lds_bytes(orc.Code(path)), path
        dd.set_min_sum_ternary(7)
        assert dd.min_sum_ternary == 7
    # refused: a column of degree 57 (|A| could reach 64), and the 8k code (24 576 edges: 192 KB of messages per group)
    for path, text in ((write(tmp_path / "deg57.txt", star(57)), "56"), (h8k_file, "LDS")):
        dd = libldpc_amd.HipDecoder(path)
        assert dd.ternary_lds_bytes() == -1
        with pytest.raises(RuntimeError, match="ldpc_hip_set_min_sum_ternary.*" + text):
            dd.set_min_sum_ternary(1)
        assert lib.ldpc_hip_set_min_sum_ternary(dd.ctx, 1) == -1 and len(lib.ldpc_hip_last_error()) > 0
        assert dd.min_sum_ternary == 0
        assert dd.decoder_choice(True, 50, "BP_MS") == "resident"


def test_choice_and_stages(lib, tmp_path):
    import libldpc_amd
    for path in (orc.H_TXT, regular_code(tmp_path, 512, 3, 6, 1)):
        d = libldpc_amd.HipDecoder(path)
        bp = {(e, i): d.decoder_choice(e, i, "BP") for e in (True, False) for i in (50, 0)}
        assert all(v == "resident" for v in bp.values()) and d.decoder_choice(True, 50, "BP_MS") == "resident"
        d.set_min_sum_ternary(1)
        assert libldpc_amd.HipDecoder.DECODERS[6] == "ternary"
        for (e, i), v in bp.items():
            assert d.decoder_choice(e, i, "BP_MS") == "ternary" and d.decoder_choice(e, i, "BP") == v
        d.set_fast_mode(1)  # min-sum ignores the fast mode
        assert d.decoder_choice(True, 50, "BP_MS") == "ternary" and d.decoder_choice(True, 50, "BP") == "fast32"
        d.set_fast_mode(0)
        d.set_min_sum_ternary(0)
        assert d.decoder_choice(True, 50, "BP_MS") == "resident"
        check_decode_stages(d, lambda d: d.set_min_sum_ternary(1), lambda d: d.set_min_sum_ternary(0))


def test_received():
    x = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 99999.9, -1e-300, 5e-324])
    assert received(x).tolist() == [0, 0, 0, 1, -1, 1, -1, 1]


def _null_vector(code):
    """A nonzero codeword: GF(2) elimination of H, one free column set."""
    H = np.zeros((code.mc, code.nc), np.uint8)
    H[code.edge_row, code.edge_col] ^= 1
    pivots, row = [], 0
    for col in range(code.nc):
        hit = np.nonzero(H[row:, col])[0]
        if hit.size == 0:
            continue
        H[[row, row + hit[0]]] = H[[row + hit[0], row]]
        others = np.nonzero(H[:, col])[0]
        others = others[others != row]
        H[others] ^= H[row]
        pivots.append(col)
        row += 1
        if row == code.mc:
            break
    free = [c for c in range(code.nc) if c not in set(pivots)]
    c = np.zeros(code.nc, np.uint8)
    c[free[len(free) // 2]] = 1
    for i, p in enumerate(pivots):  # row i reads: x_p + sum of its free columns = 0
        c[p] = H[i, free[len(free) // 2]]
    return c


def test_mirror_is_symmetric(tmp_path):
    """Decoding r and r (-1)^c for a codeword c gives hard XOR c, the same iteration counts, and A with its signs flipped
    on c: what keeps all-zero-codeword simulation valid (ties A = 0 go to the received bit)."""
    code = orc.Code(regular_code(tmp_path, 256, 3, 6, 1))
    c = _null_vector(code)
    assert c.any()
    H = np.zeros((code.mc, code.nc), np.int64)
    H[code.edge_row, code.edge_col] = 1
    assert not ((H @ c) & 1).any()
    mir = TernaryMirror(code)
    llr = flipped_llrs(code.nc, 0.05, 64, seed=5)
    sign = 1.0 - 2.0 * c
    for w in (1, 2):
        for early in (True, False):
            a = mir.decode(llr, w, early_term=early, iterations=12)
            b = mir.decode(llr * sign, w, early_term=early, iterations=12, codeword=np.tile(c, (64, 1)))
            assert np.array_equal(b["hard"], a["hard"] ^ c) and np.array_equal(a["iters"], b["iters"])
            assert np.array_equal(b["llr_out"], a["llr_out"] * sign) and np.array_equal(a["bit_errors"], b["bit_errors"])
        assert (a["llr_out"] == 0).any()  # ties occur


@pytest.mark.parametrize("case", sorted(CASES))
def test_mirror_what_it_is_for(tmp_path, case):
    """The two inputs the GPU tests decode as well: converged and failed frames both occur."""
    nc, dv, dc, cseed, w, eps, n, seed = CASES[case]
    mir = TernaryMirror(orc.Code(regular_code(tmp_path, nc, dv, dc, cseed)))
    m = mir.decode(flipped_llrs(nc, eps, n, seed), w)
    converged, failed = (m["iters"] < 50) & (m["bit_errors"] == 0), m["bit_errors"] > 0
    print(case, "decoded", int(converged.sum()), "failed", int(failed.sum()), "of", n)
    assert converged.sum() >= n // 10 and failed.sum() >= n // 10
    assert np.abs(m["llr_out"]).max() <= dv + w and m["llr_out"].dtype == np.float64


def test_h_txt_decodes_next_to_nothing():
    """h.txt's 128 degree-15 columns are punctured (r = 0).  Of its 1024 check nodes 512 see one of them, 128 two and 384
    three: a check node with two or more sends zeros on every edge for as long as those columns stay at zero, one with exactly
    one sends the punctured column the product of its other inputs and zero to everybody else.  So the messages are not all
    zero, but the mode decodes next to nothing there: no frame of these converges (measured on 100 frames each at eps = 0.01,
    0.02, 0.03 and weights 1..3: one frame in 900 converged)."""
    code = orc.Code(orc.H_TXT)
    er, ec = np.asarray(code.edge_row), np.asarray(code.edge_col)
    llr = np.zeros((24, code.nc))
    llr[:, code.bit_pos] = flipped_llrs(code.nct, 0.05, 24, seed=3)
    punctured = np.ones(code.nc, bool)
    punctured[code.bit_pos] = False
    assert punctured.sum() == 128 and (np.bincount(ec, minlength=code.nc)[punctured] == 15).all()
    seen = np.bincount(er[punctured[ec]], minlength=code.mc)
    assert np.bincount(seen).tolist() == [0, 512, 128, 384]
    mir = TernaryMirror(code)
    m = mir.decode(llr, 3, iterations=1)
    c2v = m["c2v"]
    assert c2v.shape == (24, code.nnz)
    assert not c2v[:, seen[er] >= 2].any()                       # two or more zeros among the inputs: zeros out
    assert not c2v[:, (seen[er] == 1) & ~punctured[ec]].any()    # one: zero to every other neighbour ...
    to_p = c2v[:, (seen[er] == 1) & punctured[ec]]
    assert (np.abs(to_p) == 1).all() and (to_p == -1).any()      # ... and a sign to the punctured column
    assert np.array_equal(m["llr_out"][:, ~punctured], 3.0 * received(llr)[:, ~punctured])
    for iters in (1, 7):
        m = mir.decode(llr, 3, iterations=iters)
        assert (m["iters"] == iters).all() and (m["bit_errors"] > 0).all()
