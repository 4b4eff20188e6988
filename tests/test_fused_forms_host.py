"""Host twin of tests/test_gpu_shapes.py::test_fused_codes_vs_reference_arithmetic: no GPU.

The fused kernels are held bit for bit to the det-mode oracle, and both take their check-node arithmetic from the same three
functions of detmath.h (dm_cnf2, dm_cnf3, dm_cnf4).  What says that those formulas mean the reference's check node is the
comparison with the libm-mode oracle — and it says so only on frames that FINISH in the fused form: a frame that leaves it is
decoded again from scratch, and a wrong value then shows only if it changes whether the frame leaves.  This file states, on
the oracle alone, that at the points the GPU tests use the det-mode oracle (the kernels' arithmetic) agrees with the libm-mode
oracle (the reference's) by the parity rule of test_gpu_shapes.py, and that the points keep fused results where
check_fused_counts says they must.
"""
import numpy as np
import pytest

import orc
from test_gpu_random_codes import FUSED_CASES, FUSED_NINE_LEAF_CALLS, check_fused_counts, fused_code, fused_oracle_run
from test_gpu_shapes import FUSED_REFERENCE_POINTS, assert_reference_parity


def test_rule_and_plan_agree_on_which_codes_are_fused(tmp_path):
    """The oracle decides by fused_rule.h alone, the kernels by their plan: a code one side takes and the other does not is
    decoded by two different forms (equal decisions, LLR-out apart in the last bits).  Every fused test code is taken by
    both; the code with nine calls on check nodes with a leaf — one more than four waves of two take — by neither."""
    import libldpc_amd
    for case in FUSED_CASES:
        path = fused_code(case, tmp_path)
        assert orc.Code(path).fused == 1 == libldpc_amd.HipDecoder(path).fused_plan()["ok"], case[0]
    path = fused_code(FUSED_NINE_LEAF_CALLS, tmp_path)
    code = orc.Code(path)
    deg = np.bincount(code.edge_col, minlength=code.nc)
    leaf_classes = {}
    for r in range(code.mc):
        c = code.edge_col[code.edge_row == r]
        if (deg[c] == 1).any():
            key = (len(c), int((deg[c] == 2).sum()))
            leaf_classes[key] = leaf_classes.get(key, 0) + 1
    calls = sum((n // 64 + 1) // 2 + (n % 64 != 0) for n in leaf_classes.values())
    blocks = sum((n + 63) // 64 for n in leaf_classes.values())
    assert calls == 9 and blocks <= 16, leaf_classes  # (sixteen blocks was the rule's earlier bound)
    assert code.fused == 0 == libldpc_amd.HipDecoder(path).fused_plan()["ok"]


@pytest.mark.parametrize("case", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_fused_points_det_vs_reference_arithmetic(case, tmp_path):
    import libldpc_amd
    path = fused_code(case, tmp_path)
    code = orc.Code(path)
    plan = libldpc_amd.HipDecoder(path).fused_plan()  # the plan is built on the host
    assert plan["ok"] == 1, plan
    counts = {}
    for point in FUSED_REFERENCE_POINTS:
        _, _, _, early, iters, _ = point
        det = fused_oracle_run(code, point, orc.MATH_DET, counts)
        ref = fused_oracle_run(code, point, orc.MATH_LIBM)
        assert assert_reference_parity(code, det, ref, early, iters, (case[0],) + point) >= 3, point  # converged frames
    check_fused_counts(case[0], code, plan, counts)
