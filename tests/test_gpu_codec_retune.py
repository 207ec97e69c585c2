"""tts_hip_tune of a codec layout key AFTER the first decode: the packed weight images belong to the old value, so the call drops them and the next
pass plans and packs again (csrc/codec_plan.h, drop_codec_images).  The PCM after the change equals, bit for bit, that of a fresh context created with
the value; setting the key back reproduces the first PCM; setting a key to the value it has keeps the images (debug_read "codec_packs" counts pack
launches since create).  DAC-44k dims at 3 frames: the smallest shape that reaches every class of layer."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import hip, synth

pytestmark = pytest.mark.gpu

KEYS = ["dac_split", "dac_tap7", "dac_fuse", "dac_planes", "dac_convt_b3", "dac_conv1_direct"]


@pytest.fixture(scope="module")
def dac():
    model = synth.build(synth.parler_mini(layers=1, prompt_vocab=64, ctx=64))
    codes = np.random.default_rng(2).integers(0, model.cfg.cb_size, (3, model.cfg.n_out)).astype(np.uint32)
    return model, codes


def _engine(model, tune):
    eng = hip.HipEngine(model.cfg, flags=hip.FLAG_NO_PARLER, tune=tune)
    eng.load(model)
    return eng


def _packs(eng):
    out = np.zeros(1, dtype=np.float32)
    assert eng.L.tts_hip_debug_read(eng.ctx, b"codec_packs", out.ctypes.data_as(C.POINTER(C.c_float)), 1) == 1
    return int(out[0])


@pytest.mark.parametrize("key", KEYS)
def test_dac_layout_key_after_the_first_decode(dac, key):
    model, codes = dac
    # dac_conv1_direct shows only where the units are two launches
    base = {"dac_fuse": 0} if key == "dac_conv1_direct" else {}
    fresh = _engine(model, dict(base, **{key: 0}))
    want_other = fresh.dac_decode(codes)
    fresh.close()
    eng = _engine(model, base)
    first = eng.dac_decode(codes)
    n0 = _packs(eng)
    assert n0 > 0
    eng.tune(key, 1)                      # the value it has: the images stay
    assert np.array_equal(eng.dac_decode(codes), first) and _packs(eng) == n0
    eng.tune(key, 0)
    second = eng.dac_decode(codes)
    assert _packs(eng) > n0
    assert np.array_equal(second, want_other)
    eng.tune(key, 1)
    assert np.array_equal(eng.dac_decode(codes), first)
    eng.close()


def test_kokoro_b3_after_the_first_generate():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_kokoro.npz"))
    model = synth.build_kokoro(synth.kokoro_tiny())
    total = int(g["lens"].sum())
    noise = np.random.default_rng(int(g["noise_seed"])).random(9 * 50 * model.cfg.up_sampling_factor, dtype=np.float32)[:orc.KokoroOracle(model).noise_len(total)]

    def generate(eng):
        return eng.generate(g["tokens"], g["lens"], g["hidden"], "af_test", noise, hsrc_in=g["hsrc"])

    def tune(eng, v):
        eng._chk(eng.L.tts_hip_tune(eng.ctx, b"kokoro_b3", v))

    fresh = hip.KokoroEngine(model, tune={"kokoro_b3": 0})
    want_other = generate(fresh)
    fresh.close()
    eng = hip.KokoroEngine(model)
    first = generate(eng)
    n0 = _packs(eng)
    assert n0 > 0 and not np.array_equal(first, want_other)
    tune(eng, 1)                          # the value it has: the images stay
    assert np.array_equal(generate(eng), first) and _packs(eng) == n0
    tune(eng, 0)
    assert np.array_equal(generate(eng), want_other) and _packs(eng) > n0
    tune(eng, 1)
    assert np.array_equal(generate(eng), first)
    eng.close()
