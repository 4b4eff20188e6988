"""The matcher of compile-time wave programs (libldpc_amd/csrc/fused_program.hpp; plan.cpp, match_fused_program) through the
host query ldpc_hip_fused_program: the reference's n = 1024 test code has the shape of program 0, other codes the fused rule
takes have none — their plans stay interpreted.  No GPU."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd


def _without_last_row(path, drop_leaf_column):
    """h.txt without its last check row (1023: three punctured columns of degree 15 and the leaf 1056).  drop_leaf_column:
    the leaf's column, which that row alone touched, goes too (the columns above it move down by one) — otherwise it stays
    as an isolated column."""
    head, edges = [], []
    for line in open(orc.H_TXT).read().splitlines():
        (edges if line[:1].isdigit() else head).append(line)
    edges = [tuple(map(int, e.split())) for e in edges]
    last = max(r for r, _ in edges)
    gone = [c for r, c in edges if r == last]
    leaf = max(gone)
    assert last == 1023 and len(gone) == 4 and sum(1 for _, c in edges if c == leaf) == 1
    edges = [(r, c) for r, c in edges if r != last]
    sizes = {"nc": 1152, "mc": 1023, "nct": 1152, "mct": 1023, "nnz": len(edges)}
    if drop_leaf_column:
        edges = [(r, c - (c > leaf)) for r, c in edges]
        sizes["nc"] = sizes["nct"] = 1151
    out = []
    for line in head:
        key = line.split(":")[0]
        out.append(f"{key}: {sizes[key]}" if key in sizes else line)
    open(path, "w").write("\n".join(out + [f"{r} {c}" for r, c in edges]) + "\n")
    return path


def test_the_test_code_has_a_program(lib):
    d = lib.HipDecoder(orc.H_TXT)
    assert d.fused_plan()["ok"] == 1 and d.fused_plan()["small"] == 1
    assert d.fused_program() == 0


def test_other_fused_shapes_have_none(lib, tmp_path):
    """The first two shapes of test_gpu_random_codes.FUSED_CASES (both take the small instantiation): interpreted."""
    from test_gpu_random_codes import FUSED_CASES, make_fused_code
    for name, cn_spec, vn_degs, punct, short in FUSED_CASES[:2]:
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        d = lib.HipDecoder(make_fused_code(str(tmp_path / f"{name}.txt"), rng, cn_spec, vn_degs, punct, short))
        assert d.fused_plan()["ok"] == 1 and d.fused_plan()["small"] == 1, (name, d.fused_plan())
        assert d.fused_program() == -1, name


def test_a_partly_filled_block_has_none(lib, tmp_path):
    """h.txt without its last check row: one block of degree-4 check nodes holds 63 nodes, three columns have degree 14.
    As the file stands after the deletion the row's leaf is an isolated column and the fused form does not take the code at
    all; with that column removed too the fused form takes it, on a plan of another shape."""
    d = lib.HipDecoder(_without_last_row(str(tmp_path / "h_less_row.txt"), False))
    assert (d.mc, d.nnz) == (1023, 3452)
    assert d.fused_program() == -1
    d = lib.HipDecoder(_without_last_row(str(tmp_path / "h_less_row_col.txt"), True))
    assert (d.nc, d.mc, d.nnz) == (1151, 1023, 3452)
    assert d.fused_plan()["ok"] == 1, d.fused_plan()
    assert d.fused_program() == -1


def test_program_kernel_register_budget(lib):
    """decode_fused_prog<0> runs six frames per CU like decode_fused_small: at most 80 VGPRs (512 / 6 waves per SIMD,
    allocated in eights) and no scratch in the compiler's resource report of the last build."""
    from libldpc_amd import build
    fused = build.kernel_resources("kernels_fused.hip")
    if fused is None:
        pytest.skip("no resource report (library built by something other than libldpc_amd.build)")
    key = [k for k in fused if "decode_fused_progILi0E" in k]
    assert len(key) == 1, key
    r = fused[key[0]]
    assert r["VGPRs"] <= 80 and r["ScratchSize [bytes/lane]"] == 0 and r["Occupancy [waves/SIMD]"] >= 6, r


def test_the_off_switch(lib):
    """A library whose plan.cpp was compiled with -DLDPC_AMD_FUSED_PROGRAM=0 (tools/build_variant.sh noprog plan.cpp
    "-DLDPC_AMD_FUSED_PROGRAM=0" -> ab/libldpc_noprog.so) matches nothing."""
    variant = os.path.join(ROOT, "ab", "libldpc_noprog.so")
    if not os.path.exists(variant):
        pytest.skip("no ab/libldpc_noprog.so")
    code = ("import libldpc_amd, sys; d = libldpc_amd.HipDecoder(sys.argv[1]); "
            "print('program', d.fused_program(), 'fused', d.fused_plan()['ok'])")
    p = subprocess.run([sys.executable, "-c", code, orc.H_TXT], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, LDPC_AMD_LIB=variant), timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.split()[-4:] == ["program", "-1", "fused", "1"], p.stdout
