"""Which decoder runs a batch (engine.hpp, Decoder and choose_decoder; include/ldpc_amd.h, ldpc_hip_decoder_choice) and the
launch stages that follow from it, without a GPU, over every combination of the switches.

tests/golden/decode_stages.json holds the stage lists that the library reported for the same combinations before the choice
became one enum (recorded on the CPU from a build of that commit: HipDecoder.decode_stages under every combination below,
keyed "fast<mode>/<variant>/<decoding>/<early|full>/<iterations>"; the keys of "ternary" and "layered-fixed" from a build of
the commit before the variant in force became one value, tests/golden/make_min_sum_variants.py): the stages are compared
against that record, not only against the rule the test shares with the code."""
import itertools
import json
import os

import numpy as np
import pytest

import orc
from minsum_common import EXCLUSIVE, VARIANTS as MS

VARIANTS = ("flooding",) + tuple(EXCLUSIVE)
# (ternary min-sum with weight 1, as the record was taken; its decoder does not take the 8k code: the setter refuses)
ON = {**{k: MS[k].on for k in EXCLUSIVE}, "ternary": lambda d: d.set_min_sum_ternary(1)}
COMBOS = list(itertools.product(range(4), VARIANTS, ("BP", "BP_MS"), (True, False), (50, 0)))


@pytest.fixture(scope="module")
def lib():
    import libldpc_amd
    from libldpc_amd import build
    build.build()
    return libldpc_amd.load_library()


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "decode_stages.json")))


def _rule(fast, variant, dec, taken):
    if dec == "BP_MS":  # min-sum ignores the fast mode
        return MS[variant].choice if variant != "flooding" and taken else "resident"
    return ("resident", "fast32", "layered32", "layered16")[fast]  # sum-product ignores the min-sum settings


def _set(d, fast, variant, refused=False):
    """The fast mode and at most one min-sum variant; False if the variant's setter refuses the code (nothing is then on)."""
    d.set_fast_mode(fast)
    for k in EXCLUSIVE:
        MS[k].off(d)
    if variant == "flooding":
        return True
    if refused:
        with pytest.raises(RuntimeError, match=MS[variant].setter):
            ON[variant](d)
        return False
    ON[variant](d)
    return True


@pytest.mark.parametrize("name", ["h.txt", "h8k"])
def test_choice_and_stages(lib, recorded, h8k_file, name):
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT if name == "h.txt" else h8k_file)
    _set(d, 0, "flooding")
    off = {(dec, early, it): d.decode_stages(early, it, dec) for _, _, dec, early, it in COMBOS}
    assert len(recorded[name]) == len(COMBOS)
    for fast, variant, dec, early, it in COMBOS:
        what = (name, fast, variant, dec, early, it)
        taken = _set(d, fast, variant, refused=(name, variant) == ("h8k", "ternary"))
        choice = d.decoder_choice(early, it, dec)
        assert choice == _rule(fast, variant, dec, taken), what
        stages = d.decode_stages(early, it, dec)
        assert stages == recorded[name][f"fast{fast}/{variant}/{dec}/{'early' if early else 'full'}/{it}"], what
        if choice != "resident" or off[(dec, early, it)] == ["whole"]:
            assert stages == ["whole"], what
        else:
            assert stages == off[(dec, early, it)] != ["whole"], what
    # every sequence the two codes have with the switches off is in the record (the comparison above is not vacuous)
    assert {tuple(s) for s in off.values()} >= {("whole",), ("ratio-first", "list-chain") if name == "h.txt" else ("ratio-first",)}


def test_layer_plan_is_built_once(lib):
    """The LDS figure, the setter's check and the plan self-test share one layer plan: ldpc_hip_selftest_layer_plan with a
    null output reports how often the context has run build_layer_plan."""
    import libldpc_amd
    d = libldpc_amd.HipDecoder(orc.H_TXT)
    assert lib.ldpc_hip_selftest_layer_plan(d.ctx, None) == 0  # lazy: nothing has asked yet
    assert d.layered_min_sum_lds_bytes() > 0
    d.set_min_sum_schedule("layered")
    steps = np.zeros(d.mc, np.int32)
    assert lib.ldpc_hip_selftest_layer_plan(d.ctx, steps.ctypes.data) > 0
    d.set_fast_mode(2)
    assert d.decode_stages() == ["whole"] and d.decoder_choice() == "layered32"
    d.set_min_sum_schedule("flooding")
    d.set_min_sum_schedule("layered")
    assert d.layered_min_sum_lds_bytes() > 0
    assert lib.ldpc_hip_selftest_layer_plan(d.ctx, None) == 1
    # a context that never asks never builds
    other = libldpc_amd.HipDecoder(orc.H_TXT)
    assert other.decode_stages(decoding="BP_MS") == ["whole"] and lib.ldpc_hip_selftest_layer_plan(other.ctx, None) == 0
