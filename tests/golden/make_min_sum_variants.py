#!/usr/bin/env python3
"""Fixtures of the min-sum variants' host side, recorded on the CPU (setters and ldpcsim's argument checks touch no GPU) from
a build of the commit BEFORE the variants' state became one value:

  min_sum_refusals.json   ldpc_hip_last_error after each of the 12 cross-variant refusals on h.txt ("<first>-then-<second>")
                          and after one invalid tuple per setter
  ldpcsim_refusals.json   exit status and stdout of ldpcsim for the refused command lines below (`args` follow
                          "ldpcsim h.txt <output-file> -4.5 -3.5 0.5"; stdout is the message, a newline and the usage text,
                          which the file holds once)
  decode_stages.json      gains the keys of the variants "ternary" and "layered-fixed" on both codes; the keys it has stay

tests/test_min_sum_variants_host.py and tests/test_decoder_choice_host.py compare the library against them verbatim.
LDPC_AMD_LIB and LDPCSIM select the build to record from (default: the one in the tree).
usage: python tests/golden/make_min_sum_variants.py
"""
import itertools
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
H = os.path.join(HERE, "h.txt")
HEAD = ["-4.5", "-3.5", "0.5"]

INVALID = {
    "quantized (9, 1.0)": lambda lib, ctx: lib.ldpc_hip_set_min_sum_quantization(ctx, 9, 1.0),
    "quantized (6, nan)": lambda lib, ctx: lib.ldpc_hip_set_min_sum_quantization(ctx, 6, float("nan")),
    "ternary 8": lambda lib, ctx: lib.ldpc_hip_set_min_sum_ternary(ctx, 8),
    "layered-fixed (6, 5, 0.25)": lambda lib, ctx: lib.ldpc_hip_set_min_sum_layered_fixed(ctx, 6, 5, 0.25),
}
FLAGS = {
    "schedule": ["--ms-schedule", "layered"],
    "bits": ["--ms-bits", "6", "--ms-step", "0.25"],
    "ternary": ["--ms-ternary", "2"],
    "layered-fixed": ["--ms-layered-fixed", "6,8,0.25"],
}
MS = ["--decoding", "BP_MS"]
CLI_CASES = [["--decoding", "BP"] + f for f in FLAGS.values()]
CLI_CASES += [["--ms-schedule", "flooding"], ["--ms-step", "0.25"], ["--ms-scale", "0.75"]]  # (BP is the default)
CLI_CASES += [MS + FLAGS[a] + FLAGS[b] for a, b in itertools.permutations(FLAGS, 2)]
CLI_CASES += [MS + f for f in (
    ["--ms-step", "0.5"], ["--ms-ternary", "2", "--ms-scale", "0.75"], ["--ms-ternary", "2", "--ms-offset", "0.5"],
    ["--ms-layered-fixed", "6,8"], ["--ms-layered-fixed", "6,5,0.25"], ["--ms-bits", "9"], ["--ms-ternary", "8"],
    ["--ms-schedule", "sideways"], ["--ms-layered-fixed", "6,8,x"], ["--ms-layered-fixed", "6,8,0.25", "--ms-scale", "0.75", "--ms-bits", "1"],
    # three at once, and a refusal of one flag ahead of a malformed later one: the blocks report in their own order
    FLAGS["ternary"] + FLAGS["bits"] + FLAGS["schedule"], FLAGS["layered-fixed"] + FLAGS["ternary"] + FLAGS["schedule"],
    ["--ms-ternary", "2", "--ms-scale", "0.75", "--ms-layered-fixed", "6,8"], ["--ms-step", "0.5", "--ms-ternary", "2"])]

STAGE_VARIANTS = {"ternary": lambda d: d.set_min_sum_ternary(1), "layered-fixed": lambda d: d.set_min_sum_layered_fixed(6, 8, 0.25)}


def setter_texts():
    import libldpc_amd
    from minsum_common import EXCLUSIVE, VARIANTS  # (the settings the tests switch on)
    lib = libldpc_amd.load_library()
    cross = {}
    for first, second in itertools.permutations(EXCLUSIVE, 2):
        d = libldpc_amd.HipDecoder(H)
        VARIANTS[first].on(d)
        try:
            VARIANTS[second].on(d)
            raise AssertionError((first, second))
        except RuntimeError:
            cross[f"{first}-then-{second}"] = lib.ldpc_hip_last_error().decode()
    d = libldpc_amd.HipDecoder(H)
    invalid = {}
    for name, call in INVALID.items():
        assert call(lib, d.ctx) == -1
        invalid[name] = lib.ldpc_hip_last_error().decode()
    return {"cross": cross, "invalid": invalid}


def cli_texts():
    exe = os.environ.get("LDPCSIM") or os.path.join(ROOT, "libldpc_amd", "ldpcsim")
    usage = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, text=True, timeout=60, check=True).stdout
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for args in CLI_CASES:
            p = subprocess.run([exe, H, os.path.join(tmp, "out.txt")] + HEAD + args, stdout=subprocess.PIPE, text=True, timeout=60)
            assert p.returncode != 0 and not os.listdir(tmp) and p.stdout.endswith("\n" + usage), args
            cases.append({"args": args, "status": p.returncode, "message": p.stdout[:-len(usage) - 1]})
    return {"usage": usage, "cases": cases}  # (stdout of a case: its message, a newline, the usage text)


def stages():
    """The two later variants added to the recorded keys, which stay as they are, in the file's own layout."""
    import gen_regular_code
    import libldpc_amd
    path = os.path.join(HERE, "decode_stages.json")
    rec = json.load(open(path))
    meta = json.load(open(os.path.join(HERE, "ref_sim.json")))["h8k"]
    with tempfile.TemporaryDirectory() as tmp:
        h8k = os.path.join(tmp, "h8k.txt")
        open(h8k, "w").write(gen_regular_code.generate(meta["nc"], meta["dv"], meta["dc"], meta["seed"]))
        for name, code in (("h.txt", H), ("h8k", h8k)):
            for variant, on in STAGE_VARIANTS.items():
                for fast, dec, early, it in itertools.product(range(4), ("BP", "BP_MS"), (True, False), (50, 0)):
                    d = libldpc_amd.HipDecoder(code)
                    d.set_fast_mode(fast)
                    try:
                        on(d)
                    except RuntimeError:  # (ternary min-sum does not take the 8k code: the resident decoder's stages)
                        assert (name, variant) == ("h8k", "ternary")
                    rec[name][f"fast{fast}/{variant}/{dec}/{'early' if early else 'full'}/{it}"] = d.decode_stages(early, it, dec)
    body = ",\n".join(' "%s": {\n%s\n }' % (name, ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in sorted(keys.items())))
                      for name, keys in rec.items())
    open(path, "w").write("{\n" + body + "\n}\n")


def main():
    json.dump(setter_texts(), open(os.path.join(HERE, "min_sum_refusals.json"), "w"), indent=1)
    json.dump(cli_texts(), open(os.path.join(HERE, "ldpcsim_refusals.json"), "w"), indent=1)
    stages()
    print("ok")


if __name__ == "__main__":
    main()
