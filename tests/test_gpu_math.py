"""The kernels' arithmetic against values that do not come from libldpc_amd/csrc/detmath.h.

Tier 1 of the parity argument compares the HIP kernels with an oracle mode that includes the same
header; an error in dm_exp / dm_log / dm_ratio_* / the check-node forms would be invisible there.  These tests close
that: every function is evaluated on the device (ldpc_hip_selftest_math) and held against
  * the committed fixture tests/golden/math_ref.npz — glibc libm / x87 long double values (make_math.py),
  * the same reference computed live on >= 2^20 fresh points, and
  * detmath.h compiled for the host, bit for bit (the claim "same source, same bits" behind tier 1).
Tolerances are stated per function in TOL below, in units of the reference value's ulp plus an absolute floor.

The fused form's check nodes (cnf2, cnf3, cnf4: shared reciprocals as under early termination; cnf3d, cnf4d: every output
divided on its own, the hand-over form) run one class (flip, leaf) per block of rows — the nineteen classes fused_rule.h
admits, dispatched on the device with literal arguments as the kernels' cnf_call does — against the plain divided recursion
in long double (oracle/ldpc_oracle.c ref_cnf_ld, which uses neither detmath.h nor fused_rule.h): check_cnf below.  The range
predicates are held against comparisons written out here (predicates_ref).
"""
import glob
import os

import numpy as np
import pytest

import orc

# math_ref.npz: the functions up to cn_ratio6s; math_ref_*.npz: the later ones, one file per group (make_math.py)
GOLD = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "math_ref*.npz")))

# |device - reference| <= ulps * ulp(reference) + floor(a, b)
#   exp family / log: both sides are < 1 ulp routines                                   -> 2 ulp
#   boxplus: sign*min + log term: an ulp of min(|x|,|y|) from the sum; the log term's argument (1+e^-s)/(1+e^-d) is
#            rounded three times on BOTH sides (1.1e-16 each, relative to a value in [0.5, 2]), measured 4.4e-16 apart
#   ratio forms: three roundings (numerator, denominator, quotient) against the exact value -> 3 ulp
#   check nodes in ratio form: D-2 steps of that, measured 5 ulp at D = 8                -> 8 ulp
#   shared-reciprocal forms (degree 3, 4): a product of up to four factors and a reciprocal in place of a quotient -> 8 ulp
#   check nodes in the LLR domain: results up to |L| = 600, 1 ulp(600) = 1.1e-13 per step  -> 4 ulp of the largest input
TOL = {"exp": (2, 0.0), "log": (2, 1e-300), "boxplus": (2, 6e-16), "ratio_div": (0, 0.0), "ratio_rho": (3, 0.0),
       "ratio_lambda": (3, 0.0), "e_combine": (3, 0.0), "exp_clamped": (2, 0.0), "boxplus_exp": (2, 0.0),
       "boxplus_log": (0, 3.5e-16), "cn_ratio3": (8, 0.0), "cn_ratio4": (8, 0.0), "cn_ratio5": (8, 0.0), "cn_ratio6": (8, 0.0),
       "cn_ratio8": (8, 0.0), "cn_llr4": (0, 0.0), "cn_llr6": (0, 0.0), "cn_ratio3s": (8, 0.0), "cn_ratio4s": (8, 0.0),
       "cn_ratio6s": (10, 0.0), "cn_llr3": (0, 0.0), "cn_llr5": (0, 0.0), "cn_llr16": (0, 0.0), "predicates": (0, 0.0),
       #   fused form, messages: cnf3 / cnf4 are the operation chains of cn_ratio3s / cn_ratio4s, cnf3d / cnf4d those of
       #   cn_ratio3 / cn_ratio4 (a flipped output exchanges numerator and denominator: the same count of roundings) -> 8 ulp;
       #   cnf2: an unflipped output is the correctly rounded quotient 1 / x (ratio_div's rule), a flipped one a copy -> 0 ulp
       "cnf2": (0, 0.0), "cnf3": (8, 0.0), "cnf4": (8, 0.0), "cnf3d": (8, 0.0), "cnf4d": (8, 0.0)}
# a leaf's total n / (rho_ch d): numerator, denominator, the product rho_ch d and the quotient round once each (<= 2^-53
# relative, <= 1 ulp each); half an ulp more for the reference's own rounding to binary64.  (Degree 4 forms numerator and
# denominator from nF and dF, rounded themselves: six roundings of 2^-53 in all, every term positive.  Measured on the points
# of these tests: 3 ulp at degree 3, 4 ulp at degree 4; the messages 5 ulp at most.)
LEAF_TOT_ULPS = 5
# a leaf's decision n >= rho_ch d against lambda_leaf >= rho_ch in long double: the same four roundings can turn it only where
# lambda_leaf / rho_ch is within a few 2^-53 of 1; rows within 2^-48 are not compared but counted, and only the exact ties
# the points contain on purpose (v_0 = 1, rho_ch = 1: both sides of the comparison are equal, the decision must be 1) may
# be among them
LEAF_BIT_NEAR = 2.0**-48
# The probe rows of the shared forms (every input e^+160 = 2^230.8): which classes must report an overflow.  An unflipped
# output's denominator is 1 + a b = 2^461.7 (degree 3) or nB v + dB = 2^692.5 (degree 4), a flipped one's a + b = 2^231.8
# or dB v + nB = 2^463.2.  Degree 3 inverts the product of all its message outputs' denominators: 2^1385, 2^1155, 2^925 with
# 0, 1, 2 of three flipped — beyond 2^897 — and 2^695 with all three flipped; with a leaf, of two: 2^923 with none flipped,
# 2^693 and 2^464 otherwise.  Degree 4 inverts outputs 0 and 1 together: 2^1385, 2^1155 or 2^926 in every class.
PROBE_OVERFLOWS = {"cnf3": {(0, 0), (4, 0), (6, 0), (0, 1)}, "cnf4": set(orc.CNF_CLASSES[4])}


def predicates_ref(x):
    """The range predicates of detmath.h as what they mean, bit i of the mask in this order: dm_ratio_out_of_range,
    DM_RATIO_ESCAPED(dm_ratio_key), dm_box_escaped on the upper word (all three: outside [2^-240, 2^240), and zero, denormals,
    negative values, infinities and NaN are outside), DM_SHARED_OVERFLOW and `upper word >= DM_FUSED_P_HI` (>= 2^897, or a
    bit pattern that compares above it: a set sign bit, -0 included, and NaN), DM_HANDOVER_DUE(dm_handover_key) (outside
    [2^-220, 2^220)), dm_ratio_llr_refused (|x| beyond 166, NaN, or tiny) and dm_llr_tiny(|x|) (0 < |x| < 2^-52)."""
    with np.errstate(all="ignore"):
        out_box = ~((x >= 2.0**-240) & (x < 2.0**240))
        over = (x >= 2.0**897) | np.signbit(x) | np.isnan(x)
        handover = ~((x >= 2.0**-220) & (x < 2.0**220))
        tiny = (np.abs(x) < 2.0**-52) & (x != 0)
        refused = ~(np.abs(x) <= 166.0) | tiny
    bits = (out_box, out_box, out_box, over, over, handover, refused, tiny)
    return sum(b.astype(np.float64) * 2**i for i, b in enumerate(bits))


def reference(fn, a, b):
    return predicates_ref(a) if fn == "predicates" else orc.math_eval(fn, a, b)


def points_per_function(fn, n_scalar, n_rows, n_class):
    return n_class if fn in orc.CNF_DEGREE else n_rows if fn.startswith("cn_") else n_scalar


def check_cnf(fn, a, got, ref):
    """Rows of a fused check node (orc.CNF_CLASSES): messages within TOL of the reference, a leaf's entry untouched, its total
    within LEAF_TOT_ULPS, its decision equal wherever the total is not within LEAF_BIT_NEAR of 1, exact ties decided as 1,
    and the probe rows of the shared forms flagged (all NaN) exactly where PROBE_OVERFLOWS says."""
    d = orc.CNF_DEGREE[fn]
    ulps, floor = TOL[fn]
    mode = a[:, d].astype(np.int64)
    flip, leaf = mode & 15, (mode >> 4 & 1).astype(bool)
    assert {(int(f), int(l)) for f, l in zip(flip, leaf)} == set(orc.CNF_CLASSES[d])
    with np.errstate(all="ignore"):
        L = np.log(a[:, :d])
        probe = (np.abs(np.abs(L) - orc.CNF_OVERFLOW_L) < 1e-9).all(axis=1) if fn in PROBE_OVERFLOWS else np.zeros(len(a), bool)
        if fn in PROBE_OVERFLOWS:
            must = probe & (L[:, 0] > 0) & np.array([(int(f), int(l)) in PROBE_OVERFLOWS[fn] for f, l in zip(flip, leaf)])
            assert must.sum() >= 2 * len(PROBE_OVERFLOWS[fn]) and (probe & ~must).any()
            assert np.isnan(got[must]).all(), fn
            assert np.isfinite(got[probe & ~must][:, :d + 1]).all(), fn
        rows = ~probe  # the probe rows take no part in the comparison with the reference
        assert np.isfinite(got[rows][:, :d + 1]).all(), fn
        for k in range(d):
            is_leaf = leaf & (k == d - 1)
            m = rows & ~is_leaf
            tol = ulps * np.spacing(np.abs(ref[m, k])) + floor
            bad = ~(np.abs(got[m, k] - ref[m, k]) <= tol)
            assert not bad.any(), (fn, k, int(bad.sum()), a[m][bad][:3], got[m][bad][:3], ref[m][bad][:3])
            assert np.array_equal(got[rows & is_leaf, k], a[rows & is_leaf, k]), (fn, "leaf entry")
        lf, tot = rows & leaf, ref[:, d + 1]
        assert np.isnan(got[rows & ~leaf, d + 1]).all() and np.isnan(tot[rows & ~leaf]).all() and not got[rows & ~leaf, d].any()
        bad = ~(np.abs(got[lf, d + 1] - tot[lf]) <= LEAF_TOT_ULPS * np.spacing(np.abs(tot[lf])))
        assert not bad.any(), (fn, "leaf_tot", int(bad.sum()), a[lf][bad][:3], got[lf][bad][:3], ref[lf][bad][:3])
        near = lf & (np.abs(tot - 1.0) <= LEAF_BIT_NEAR)
        tie = lf & (a[:, 0] == 1.0) & (a[:, d - 1] == 1.0)
        assert np.array_equal(got[lf & ~near, d], ref[lf & ~near, d]), (fn, "leaf_bit")
        assert int((near & ~tie).sum()) == 0, (fn, "rows too close to a tie to compare", int((near & ~tie).sum()))
        n_leaf_classes = sum(l for _, l in orc.CNF_CLASSES[d])
        assert tie.sum() == orc.CNF_TIE_ROWS * n_leaf_classes and (tot[tie] == 1.0).all() and (ref[tie, d] == 1.0).all() and (got[tie, d] == 1.0).all(), (fn, "ties")


def check(fn, a, b, got, ref):
    if fn in orc.CNF_DEGREE:
        return check_cnf(fn, a, got, ref)
    ulps, floor = TOL[fn]
    with np.errstate(all="ignore"):
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), fn
        assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), fn  # infinities as libm returns them
        tol = ulps * np.spacing(np.abs(ref)) + floor
        if fn == "boxplus":
            tol = tol + np.spacing(np.minimum(np.abs(a), np.abs(b)))
        if fn.startswith("cn_llr"):
            tol = 4 * np.spacing(np.abs(a).max(axis=1, keepdims=True)) + 2e-15
        bad = fin & ~(np.abs(got - ref) <= tol)
    assert not bad.any(), (fn, int(bad.sum()), a[bad][:3], got[bad][:3], ref[bad][:3])


@pytest.fixture(scope="module")
def gold():
    out = {}
    for path in GOLD:
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


@pytest.mark.parametrize("fn", orc.MATH_FNS)
def test_fixture_is_what_libm_says_here(gold, fn):
    """The committed values against the same computation on this machine (glibc picks exp/log variants per CPU: they
    may differ in the last bit), and detmath.h on the host within the stated tolerance of them."""
    a, b, ref = gold[f"{fn}/a"], gold[f"{fn}/b"] if f"{fn}/b" in gold else None, gold[f"{fn}/ref"]
    with np.errstate(all="ignore"):
        live = reference(fn, a, b)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(live), fin)
        assert (np.abs(live[fin] - ref[fin]) <= 4 * np.spacing(np.abs(ref[fin])) + 4e-16).all()
    check(fn, a, b, orc.math_eval(fn, a, b, det=True), ref)


@pytest.mark.parametrize("fn", ["boxplus", "cn_llr4", "cn_llr6", "cn_llr3", "cn_llr5", "cn_llr16", "cnf2", "cnf3", "cnf4", "cnf3d", "cnf4d",
                                "predicates"])
def test_host_header_vs_libm_on_live_points(fn):
    """detmath.h compiled for the host against libm / the libm box-plus chain / long double on fresh points — saturated
    check nodes (magnitudes to 1e13, the edges of the rule: smallest input around 40, spread around 600), inputs below 2^-52,
    saturated box-plus operands and every class of the fused form's check nodes (2^15 rows each) included
    (orc.math_points).  The device side of the same comparison needs a GPU (below)."""
    a, b = orc.math_points(fn, points_per_function(fn, 1 << 18, 1 << 15, 1 << 15), seed=11)
    with np.errstate(all="ignore"):
        check(fn, a, b, orc.math_eval(fn, a, b, det=True), reference(fn, a, b))
    if fn.startswith("cn_"):
        tiny = (np.abs(a) < 2.0**-52) & (a != 0)
        assert tiny.any(axis=1).sum() >= 16
        mu, amax = np.abs(a).min(axis=1), np.abs(a).max(axis=1)
        sat = (mu >= 40) & (amax - mu <= 600)
        assert 0.2 < sat.mean() < 0.7 and ((amax > 600) & ~sat).any() and ((amax <= 600) & ~sat).any()  # all three forms taken


@pytest.fixture(scope="module")
def dec():
    import libldpc_amd
    return libldpc_amd.HipDecoder(orc.H_TXT)


@pytest.mark.gpu
@pytest.mark.parametrize("fn", orc.MATH_FNS)
def test_device_arithmetic_vs_fixture(dec, gold, fn):
    a, b, ref = gold[f"{fn}/a"], gold[f"{fn}/b"] if f"{fn}/b" in gold else None, gold[f"{fn}/ref"]
    check(fn, a, b, dec.selftest_math(fn, a, b), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("fn", orc.MATH_FNS)
def test_device_arithmetic_vs_live_libm_and_host_header(dec, fn):
    """2^20 fresh points per scalar function (2^17 rows per check-node function, 2^15 per class of a fused check node):
    within tolerance of libm / long double, and bit-identical to detmath.h compiled for the host."""
    a, b = orc.math_points(fn, points_per_function(fn, 1 << 20, 1 << 17, 1 << 15), seed=7)
    got = dec.selftest_math(fn, a, b)
    with np.errstate(all="ignore"):
        check(fn, a, b, got, reference(fn, a, b))
        host = orc.math_eval(fn, a, b, det=True)
    same = (got == host) | (np.isnan(got) & np.isnan(host))
    assert same.all(), (fn, int((~same).sum()), a[~same][:3] if a.ndim == 1 else a[~same.all(axis=1)][:1])
    assert np.array_equal(np.signbit(got), np.signbit(host))  # signed zeros included
