"""The raw bits behind profiles/codec_images.json: CRC32 of the PCM and of every dac:<stage> / snac:<stage> snapshot the codec leaves, for comparing
two builds of the tree (after profiles/attn_kv_bits.py).  One invocation is one process on one tree: it imports tts_cpp_amd and tests/ from the
WORKING DIRECTORY, so the same file runs against any built checkout:

    (cd PARENT_CHECKOUT && python THIS_FILE --out parent.json)
    (cd THIS_CHECKOUT   && python THIS_FILE --out new.json)
    python THIS_FILE --compare parent.json new.json

Entries: every ARITH_CASES row of tests/test_gpu_dac.py, F16 codec tensors with dac_f16_planes 1 and 0, and TTS_HIP_FLAG_VALU_GEMM, each on the DAC-44k
dims as a decode at 3 frames (with the stage snapshots), a ragged batch of 1, 5 and 3 frames and a decode at 70 frames; synth.snac_tiny with and
without noise; the Kokoro tiny model's generate under {}, kokoro_split 0, kokoro_b3 0, kokoro_mfma 0 and kokoro_lstm_split 0."""
import argparse
import json
import os
import sys
import zlib

import numpy as np


def crc(a):
    return f"{zlib.crc32(np.ascontiguousarray(a, dtype=np.float32).tobytes()) & 0xFFFFFFFF:08x}"


def record(out_path):
    root = os.getcwd()
    for p in (os.path.join(root, "oracle"), os.path.join(root, "tests"), root):
        sys.path.insert(0, p)
    import oracle as orc
    import test_gpu_dac as td
    from tts_cpp_amd import hip, synth

    out = {}

    def dac(tag, model, flags, tune, env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            eng = hip.HipEngine(model.cfg, flags=hip.FLAG_NO_PARLER | flags, tune=tune)
        finally:
            for k, v in old.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        eng.load(model)
        cfg = model.cfg
        codes = np.random.default_rng(2).integers(0, cfg.cb_size, (3, cfg.n_out)).astype(np.uint32)
        eng.set_debug(True)
        out[f"dac/{tag}/3 frames/pcm"] = crc(eng.dac_decode(codes))
        for st in range(2 + len(cfg.strides)):
            out[f"dac/{tag}/3 frames/dac:{st}"] = crc(eng.debug_read(f"dac:{st}", 1 << 22))   # the whole snapshot, whatever its size
        eng.set_debug(False)
        ragged = [np.random.default_rng(f).integers(0, cfg.cb_size, (f, cfg.n_out)).astype(np.uint32) for f in (1, 5)] + [codes]
        for i, pcm in enumerate(eng.dac_decode_batch(ragged)):
            out[f"dac/{tag}/ragged 1 5 3/pcm{i}"] = crc(pcm)
        out[f"dac/{tag}/70 frames/pcm"] = crc(eng.dac_decode(np.random.default_rng(70).integers(0, cfg.cb_size, (70, cfg.n_out)).astype(np.uint32)))
        eng.close()

    m32 = synth.build(synth.parler_mini(layers=1, prompt_vocab=64, ctx=64))
    for name, env, tune, _ in td.ARITH_CASES:
        dac(name, m32, 0, tune, env)
    dac("valu_gemm", m32, hip.FLAG_VALU_GEMM, {}, {})
    m16 = synth.build(synth.parler_mini(layers=1, prompt_vocab=64, ctx=64, dac_f16=True))
    for v in (1, 0):
        dac(f"f16_tensors_planes_{v}", m16, 0, {"dac_f16_planes": v}, {})

    T = 64
    sm = synth.build_snac(synth.snac_tiny(max_frames=T))
    scfg = sm.cfg
    rng = np.random.default_rng(11)
    codes = np.concatenate([rng.integers(0, scfg.cb_size, T // r) for r in scfg.repeats]).astype(np.uint32)
    noise = np.random.default_rng(12).standard_normal(orc.SnacOracle(sm).noise_len(T)).astype(np.float32)
    for with_noise in (True, False):
        eng = hip.SnacEngine(scfg)
        eng.load(sm)
        eng.set_debug(True)
        out[f"snac_tiny/noise={with_noise}/pcm"] = crc(eng.decode(codes, T, noise if with_noise else None))
        for st in range(2 + len(scfg.strides) + 1):
            out[f"snac_tiny/noise={with_noise}/snac:{st}"] = crc(eng.debug_read(f"snac:{st}", 1 << 22))
        eng.close()

    g = np.load(os.path.join(root, "tests", "golden", "tiny_kokoro.npz"))
    km = synth.build_kokoro(synth.kokoro_tiny())
    total = int(g["lens"].sum())
    knoise = np.random.default_rng(int(g["noise_seed"])).random(9 * 50 * km.cfg.up_sampling_factor, dtype=np.float32)[:orc.KokoroOracle(km).noise_len(total)]
    for tune in ({}, {"kokoro_split": 0}, {"kokoro_b3": 0}, {"kokoro_mfma": 0}, {"kokoro_lstm_split": 0}):
        eng = hip.KokoroEngine(km, tune=tune)
        lens, hid = eng.durations(g["tokens"], "af_test")
        tag = json.dumps(tune, sort_keys=True)
        out[f"kokoro_tiny/{tag}/durations"] = crc(np.concatenate([lens, hid.reshape(-1)]))
        pcm, hs = eng.generate(g["tokens"], g["lens"], g["hidden"], "af_test", knoise, want_hsrc=True)
        out[f"kokoro_tiny/{tag}/generate/pcm"] = crc(pcm)
        out[f"kokoro_tiny/{tag}/generate/hsrc"] = crc(hs)
        eng.close()
    json.dump(out, open(out_path, "w"), indent=1, sort_keys=True)
    print(json.dumps({"entries": len(out), "out": out_path}))


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    assert sorted(a) == sorted(b), "the two runs recorded different entries"
    differing = {k: [a[k], b[k]] for k in sorted(a) if a[k] != b[k]}
    print(json.dumps({"entries": len(a), "differing": differing, "verdict": "bit-identical" if not differing else "differs", "crc32": [a, b]}, indent=1, sort_keys=True))
    return 0 if not differing else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    record(args.out or "codec_bits.json")
