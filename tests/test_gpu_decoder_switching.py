"""One context walked through all six decoders in an interleaved order (engine.hpp, Decoder): the layer plan and its upload
are shared between the layered sum-product modes and layered min-sum, and every plan is uploaded at the first launch that
needs it, in whatever order the caller gets there.  Each result equals, bit for bit, that of a fresh context given only
the setting in force."""
import pytest

import orc
from minsum_common import WANT, dumped, same

pytestmark = pytest.mark.gpu


def _apply(d, fast=0, schedule="flooding", quantization=(0, 1.0), correction=(1.0, 0.0)):
    d.set_fast_mode(fast)
    d.set_min_sum_quantization(0)  # (it and the layered schedule exclude each other: off before either is set)
    d.set_min_sum_schedule(schedule)
    d.set_min_sum_quantization(*quantization)
    d.set_min_sum_correction(*correction)


def test_interleaved_walk_equals_fresh_contexts():
    import libldpc_amd
    walked = libldpc_amd.HipDecoder(orc.H_TXT)
    llr = dumped(walked, lambda d: None, "AWGN", -5.0, 8)
    layered = dict(schedule="layered", correction=(0.8125, 0.25))
    quantized = dict(quantization=(6, 0.25), correction=(0.8125, 0.0))
    # (what the walked context is told, the decoding, what alone decides the result, the decoder that runs)
    walk = [
        (dict(), "BP_MS", dict(), "resident"),
        (layered, "BP_MS", layered, "layered-min-sum"),
        (dict(), "BP_MS", dict(), "resident"),
        (quantized, "BP_MS", quantized, "quantized-min-sum"),
        (dict(fast=3, **quantized), "BP", dict(fast=3), "layered16"),  # sum-product ignores the min-sum settings
        (dict(fast=3, **quantized), "BP_MS", quantized, "quantized-min-sum"),  # ... and min-sum the fast mode
        (dict(fast=2, **quantized), "BP", dict(fast=2), "layered32"),
        (dict(fast=1), "BP", dict(fast=1), "fast32"),
        (dict(fast=1, **layered), "BP_MS", layered, "layered-min-sum"),
        (dict(), "BP", dict(), "resident"),
        (dict(), "BP_MS", dict(), "resident"),
    ]
    seen = set()
    for i, (told, dec, alone, choice) in enumerate(walk):
        _apply(walked, **told)
        assert walked.decoder_choice(True, 50, dec) == choice, i
        r = walked.decode_batch(llr, early_term=True, iterations=50, decoding=dec, want=WANT)
        fresh = libldpc_amd.HipDecoder(orc.H_TXT)
        _apply(fresh, **alone)
        assert fresh.decoder_choice(True, 50, dec) == choice, i
        same(r, fresh.decode_batch(llr, early_term=True, iterations=50, decoding=dec, want=WANT), (i, told, dec))
        fresh.close()
        seen.add(choice)
    assert len(seen) == 6
