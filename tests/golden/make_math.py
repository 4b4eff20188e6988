#!/usr/bin/env python3
"""Fixture for the arithmetic tests (tests/test_gpu_math.py): operands and the values the functions of
libldpc_amd/csrc/detmath.h / device_cn.hpp are MEANT to return, computed without that header — glibc libm in binary64
for exp, log and the reference's jacobian expression (src/decoding/decoder.h:12-15), x87 long double for the rational
expressions and for the plain divided forward/backward check-node recursion (src/decoding/decoder.cpp:31-44).

The values come from oracle/liboracle.so's orc_math_ref (oracle/ldpc_oracle.c) on operands drawn by
tests/orc.py:math_points(fn, n, seed=2026): 4096 points per scalar function, 1024 rows per check-node function (per class
of a fused check node), box edges (|L| = 166, 600, 700, 709) and special operands included.

math_ref.npz holds the functions up to cn_ratio6s and is never written again: glibc picks exp / log variants per CPU, so
recomputing it elsewhere would move last bits of values the suite has been held to.  Later functions go into files of
their own, one per group of GROUPS, each below the size a committed file may have; a file that exists is left alone.
usage: python tests/golden/make_math.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc  # noqa: E402
from test_gpu_math import reference  # noqa: E402  (the predicates' reference is written out there)

SEED = 2026
FIRST = orc.MATH_FNS[:orc.MATH_FNS.index("cn_ratio6s") + 1]
GROUPS = {"math_ref.npz": FIRST, "math_ref_cnf23.npz": ("cnf2", "cnf3", "cnf3d"), "math_ref_cnf4.npz": ("cnf4",),
          "math_ref_cnf4d.npz": ("cnf4d",), "math_ref_llr.npz": ("cn_llr3", "cn_llr5", "cn_llr16", "predicates")}
MAX_BYTES = 1 << 20


def main():
    assert sorted(sum(map(list, GROUPS.values()), [])) == sorted(orc.MATH_FNS)
    for name, fns in GROUPS.items():
        path = os.path.join(HERE, name)
        if os.path.exists(path):
            print("kept", name)
            continue
        out = {}
        for fn in fns:
            a, b = orc.math_points(fn, 4096 if fn in orc.MATH_FNS[:10] else 1024, SEED)
            with np.errstate(all="ignore"):
                ref = reference(fn, a, b)
            out[f"{fn}/a"] = a
            if b is not None:
                out[f"{fn}/b"] = b
            out[f"{fn}/ref"] = ref
        np.savez_compressed(path, **out)
        print("wrote", name, "functions", len(fns), "bytes", os.path.getsize(path))
        assert name == "math_ref.npz" or os.path.getsize(path) <= MAX_BYTES, name  # (the first file is older than the limit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
