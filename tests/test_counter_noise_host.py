"""Counter-based noise mode (include/ldpc_amd.h, ldpc_hip_set_noise), host side: the Python restatement of Philox4x32-10
against the published known answers, the mode switch's argument check on a context that never touched a GPU, and the
CLI flag."""
import os
import subprocess

import numpy as np
import pytest

import orc
import philox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "libldpc_amd", "ldpcsim")


@pytest.mark.parametrize("case", range(len(philox_ref.KNOWN_ANSWERS)))
def test_restatement_reproduces_known_answers(case):
    c, k, out = philox_ref.KNOWN_ANSWERS[case]
    assert tuple(int(v) for v in philox_ref.philox4x32_10(c, k)) == out


def test_restatement_layout():
    """The key / counter layout: (seed, frame) split into 32-bit halves; tags select independent words."""
    seed, frame = 0x0123456789ABCDEF, (5 << 32) | 7
    w = philox_ref.blocks(seed, 2, [frame], [3])[0, 0]
    assert tuple(int(v) for v in w) == tuple(int(v) for v in philox_ref.philox4x32_10((3, 7, 5, 2), (0x89ABCDEF, 0x01234567)))
    n, r = philox_ref.awgn_normals(1, [0, 1], 1024)
    assert n.shape == (2, 1024) and np.all(np.abs(n) <= r + 1e-12) and r.max() <= np.sqrt(66 * np.log(2)) + 1e-9


def test_set_noise_rejects_unknown_mode_without_gpu():
    import libldpc_amd
    dec = libldpc_amd.HipDecoder(orc.H_TXT)  # (parses the code only: no GPU is touched)
    assert dec.lib.ldpc_hip_set_noise(dec.ctx, 7) == -1
    assert "noise" in dec.lib.ldpc_hip_last_error().decode()
    with pytest.raises(RuntimeError, match="noise"):
        dec.set_noise("bogus")
    with pytest.raises(RuntimeError, match="noise"):
        dec.set_noise(2)
    dec.set_noise("counter")
    dec.set_noise("reference")
    assert dec.lib.ldpc_hip_set_noise(dec.ctx, 1) == 0 and dec.lib.ldpc_hip_set_noise(dec.ctx, 0) == 0


def test_cli_help_lists_noise_and_rejects_bogus(tmp_path):
    out = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "--noise" in out and "counter" in out and "NON-PARITY" in out
    p = subprocess.run([CLI, orc.H_TXT, str(tmp_path / "o.txt"), "0", "1", "1", "--noise", "bogus"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert p.returncode != 0 and "--noise" in p.stdout
    assert not (tmp_path / "o.txt").exists()
