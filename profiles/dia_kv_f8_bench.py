"""The measurement behind profiles/dia_kv_f8.json / dia_kv_f8_parent_before.json: the Dia device loop's step over fp32, fp16 and e4m3 K/V caches
(tts_hip_tune "kv_f8"), Dia-1.6B shapes, synthetic fp16 matrices (secondary_bench.dia_tensors), on the model of dia_kv_f16_bench.py.

It imports tts_cpp_amd from the WORKING DIRECTORY, so the same file measures any built checkout; a kind the tree refuses is dropped (the parent: f32 and f16):

    (cd PARENT_CHECKOUT && python THIS_FILE --kinds f32,f16 --out dia_kv_f8_parent_before.json)
    (cd THIS_CHECKOUT   && python THIS_FILE --out dia_kv_f8.json)

One process per slot count runs its legs one after the other, fp32 -> fp16 -> e4m3 (-> the comparison kinds), each with tune("dia_cross_bounded") 0 and 1: the
weights are drawn once, every leg has its own context.  A leg: S slots (2 S rows) encoded with a 200-byte sentence, the greedy loop of tts_hip_dia_gen_begin with
max_gen 2100 run to position 84, 16 steps of warm-up, then STRETCHES stretches of STEPS timed steps from position 100; on to 1984, 16 steps, the same from 2000.
ms per step from a host clock around gen_launch + gen_wait.  A figure is [median, min, max] of its stretches (the positions grow from stretch to stretch).
Comparison kinds: "f8_generic" = e4m3 with tune("attn_wave") 0 (attn_gqa_kernel<128, *, kv_f8> for the cross launch); "f8_ext" = e4m3 with the bench-only
tune("dia_f8_ext") 1, attn_gqa_wave_kernel's EXT mapping instantiated over kv_f8 (key-split launches without dia_cross_bounded only; the key exists only in the
build that was measured: the mapping lost and was deleted)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

MAX_GEN = 2100
POSITIONS = (100, 2000)
WARM, STEPS, STRETCHES = 16, 16, 5
DELAY = [0, 8, 9, 10, 11, 12, 13, 14, 15]
TUNES = {"f32": {}, "f16": {}, "f8": {"kv_f8": 1}, "f8_generic": {"kv_f8": 1, "attn_wave": 0}, "f8_ext": {"kv_f8": 1, "dia_f8_ext": 1}}


def legs(kinds, slots):
    root = os.getcwd()
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "profiles"))
    import tts_cpp_amd  # noqa: F401
    from tts_cpp_amd import gguf, hip, synth
    import secondary_bench as sb
    assert os.path.dirname(os.path.abspath(hip.__file__)).startswith(root), hip.__file__
    cfg = synth.dia_1_6b(weight_type=gguf.F16, max_gen=MAX_GEN)
    rng = np.random.default_rng(3)
    model = sb._Model(cfg, sb.dia_tensors(cfg, rng)[0])
    toks = np.zeros(cfg.max_ctx, dtype=np.uint32)
    toks[:200] = rng.integers(32, 127, 200)
    for kind in kinds:
        for bounded in (0, 1):
            if kind == "f8_ext" and (bounded or 2 * slots * cfg.dec_heads > 256):
                continue
            eng = hip.DiaEngine(cfg, max_utterances=slots, **({"kv_type": gguf.F16} if kind == "f16" else {}))
            try:
                for k, v in {**TUNES[kind], "dia_cross_bounded": bounded}.items():
                    eng.tune(k, v)
            except hip.HipError as e:
                print(json.dumps({"kind": kind, "bounded": bounded, "dropped": str(e)}), flush=True)
                eng.close()
                continue
            eng.load(model)
            for u in range(slots):
                eng.encode_slot(u, toks, 200)
            eng.gen_begin(slots, MAX_GEN, DELAY, cfg.bos, cfg.eos, cfg.pad, 15)
            out, at = {}, 0
            for P in POSITIONS:
                eng.gen_launch(P - WARM - at)
                eng.gen_wait(take=False)
                eng.gen_launch(WARM)
                eng.gen_wait(take=False)
                ms = []
                for _ in range(STRETCHES):
                    t = time.perf_counter()
                    eng.gen_launch(STEPS)
                    _, steps, done, _ = eng.gen_wait(take=False)
                    ms.append((time.perf_counter() - t) / STEPS * 1e3)
                at = P + STEPS * STRETCHES
                assert not done.any() and min(steps) >= at - 1, (steps, done)      # every slot is still generating at the timed positions
                out[str(P)] = [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]
            print(json.dumps({"kind": kind, "bounded": bounded, "elem": int(eng.debug_read("di_kv_elem", 1)[0]), "ms": out}), flush=True)
            eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--kinds", default="f32,f16,f8,f8_generic,f8_ext")
    ap.add_argument("--slots", default="4,16,128")
    ap.add_argument("--legs", type=int, help="internal: run the legs of one slot count in this process, one JSON line each")
    args = ap.parse_args()
    kinds = args.kinds.split(",")
    if args.legs:
        return legs(kinds, args.legs)
    res = {"shapes": "dia-1.6b, fp16 matrices, max_gen %d, 200-byte sentences" % MAX_GEN, "figure": "ms per step [median, min, max] of %d stretches of %d steps" % (STRETCHES, STEPS),
           "ms_per_step": {}}
    for S in (int(s) for s in args.slots.split(",")):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--legs", str(S), "--kinds", args.kinds], capture_output=True, text=True, timeout=1100)
        rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
        res["ms_per_step"]["%d slots (%d rows)" % (S, 2 * S)] = rows
        print(S, json.dumps(rows), flush=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        if p.returncode != 0:
            print(p.stderr[-1500:], flush=True)
            raise SystemExit("the legs of %d slots ended with %d: nothing more is started on this device" % (S, p.returncode))


if __name__ == "__main__":
    main()
