#!/usr/bin/env python3
"""Host-path speed of the codec for profiles/codec_images.json: one process on one tree (tts_cpp_amd from the WORKING DIRECTORY), one JSON line of
ms per leg.  Run the parent's checkout and this one in alternating processes.  Legs, at the shapes of profiles/dac_bench.py, secondary_bench.py
and kokoro_bench.py: a 64 x 248-frame DAC pass (3 reps), one 248-frame utterance (20 reps; launch overhead shows most), the same on F16 codec
tensors, a SNAC 24 kHz window pass (8 windows of 32 frames, 20 reps), Kokoro-82M generate at 64 phoneme ids x 3 frames (3 reps)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import tts_cpp_amd  # noqa: E402,F401
from tts_cpp_amd import hip, synth  # noqa: E402


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return round((time.perf_counter() - t0) / reps * 1e3, 4)


out = {}
rng = np.random.default_rng(0)
for f16 in (False, True):
    cfg = synth.parler_mini(layers=1, prompt_vocab=64, ctx=64, dac_f16=f16)
    eng = hip.HipEngine(cfg, flags=hip.FLAG_NO_PARLER)
    eng.load(synth.build(cfg))
    codes = [rng.integers(0, cfg.cb_size, (248, cfg.n_out)).astype(np.uint32) for _ in range(64)]
    if not f16:
        out["dac_64x248_ms"] = timed(lambda: eng.dac_decode_batch(codes), 3)
    out["dac_f16_1x248_ms" if f16 else "dac_1x248_ms"] = timed(lambda: eng.dac_decode_batch(codes[:1]), 20)
    eng.close()

scfg = synth.snac_24khz(max_frames=4 * 32 * 8)
snac = hip.SnacEngine(scfg)
snac.load(synth.build_snac(scfg))
T = 4 * 32
windows = [(np.concatenate([rng.integers(0, scfg.cb_size, T // r) for r in scfg.repeats]).astype(np.uint32), 32, 8, 24, None) for _ in range(8)]
out["snac_8_windows_ms"] = timed(lambda: snac.decode_windows(windows), 20)
snac.close()

km = synth.build_kokoro(synth.kokoro_82m())
keng = hip.KokoroEngine(km)
kcfg = km.cfg
toks = np.concatenate([[0], rng.integers(1, kcfg.vocab, 64), [0]]).astype(np.uint32)
lens, hid = keng.durations(toks, kcfg.voices[0])
forced = np.full(toks.size, 3.0, dtype=np.float32)
noise = rng.random((kcfg.harmonic_num + 1) * int(forced.sum()) * kcfg.up_sampling_factor, dtype=np.float32)
out["kokoro_generate_64_ids_ms"] = timed(lambda: keng.generate(toks, forced, hid, kcfg.voices[0], noise), 3)
keng.close()
print(json.dumps(out))
