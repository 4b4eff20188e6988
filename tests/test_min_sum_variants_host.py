"""The four min-sum variants that exclude each other (engine.hpp, MsVariant: the layered schedule, quantization, ternary and
fixed-point layered min-sum) without a GPU: the texts of the setters' and ldpcsim's refusals against the record of
tests/golden/make_min_sum_variants.py, byte for byte.  (What a refusal leaves behind, over every ordered pair of the setters:
test_layered_fixed_min_sum_host.py, test_excludes_the_other_variants.)"""
import itertools
import json
import os
import subprocess

import pytest

import orc
from minsum_common import EXCLUSIVE, ROOT, VARIANTS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


PAIRS = list(itertools.permutations(EXCLUSIVE, 2))


def test_setter_refusals_are_the_recorded_texts(lib):
    import libldpc_amd
    rec = json.load(open(os.path.join(GOLDEN, "min_sum_refusals.json")))
    assert sorted(rec["cross"]) == sorted("-then-".join(p) for p in PAIRS)
    for key, text in rec["cross"].items():
        first, second = key.split("-then-")
        d = libldpc_amd.HipDecoder(orc.H_TXT)
        VARIANTS[first].on(d)
        with pytest.raises(RuntimeError) as e:
            VARIANTS[second].on(d)
        assert lib.ldpc_hip_last_error().decode() == text and str(e.value).endswith(text), key
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    calls = {"quantized (9, 1.0)": lambda: lib.ldpc_hip_set_min_sum_quantization(d.ctx, 9, 1.0),
             "quantized (6, nan)": lambda: lib.ldpc_hip_set_min_sum_quantization(d.ctx, 6, float("nan")),
             "ternary 8": lambda: lib.ldpc_hip_set_min_sum_ternary(d.ctx, 8),
             "layered-fixed (6, 5, 0.25)": lambda: lib.ldpc_hip_set_min_sum_layered_fixed(d.ctx, 6, 5, 0.25)}
    assert sorted(calls) == sorted(rec["invalid"])
    for key, call in calls.items():
        assert call() == -1 and lib.ldpc_hip_last_error().decode() == rec["invalid"][key], key
    assert not any(VARIANTS[k].state(d) for k in EXCLUSIVE) and d.decoder_choice(decoding="BP_MS") == "resident"


def test_ldpcsim_refusals_are_the_recorded_output(lib, tmp_path):
    """Exit status and stdout of every recorded command line, and no result file."""
    rec = json.load(open(os.path.join(GOLDEN, "ldpcsim_refusals.json")))
    exe, out = os.path.join(ROOT, "libldpc_amd", "ldpcsim"), tmp_path / "out.txt"
    assert len(rec["cases"]) >= 21
    for case in rec["cases"]:
        p = subprocess.run([exe, orc.H_TXT, str(out), "-4.5", "-3.5", "0.5"] + case["args"], stdout=subprocess.PIPE, text=True, timeout=60)
        assert (p.returncode, p.stdout) == (case["status"], case["message"] + "\n" + rec["usage"]), case["args"]
    assert not os.listdir(tmp_path)
