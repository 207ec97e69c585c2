"""Parler-Mini shapes, fp16 weights and KV cache, no codec, 1023 slots (forwards of 1024 rows), greedy: what a voice per slot costs a step of
the continuous session.

  (a) one_description   every slot at voice 0: the one-description forward (the cross-attention inside the q projection's tiles)
  (b) eight_voices      slots cycling over 8 bank voices of 8 .. 32 positions: the "voices" forward (q stored, attn_short_voices_kernel, the out
                        projection reading the attended rows)
  (c) one_bank_voice    every slot at the same non-zero voice: the same forward, one K / V base
16-id prompts, a warm-up run of WARM steps (it captures the graph), then STEPS timed steps of one stream_run; REPS repetitions, median and
max - min.  On a build without the voice bank (the parent commit) only leg (a) runs and the result goes to parler_voices_parent_before.json:
leg (a) of this build must lie within that file's spread of its figure.  (b) and (c) are reported, not bounded.
Usage: python profiles/parler_voices_bench.py [--out FILE] [--reps N] [--slots N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tts_cpp_amd  # noqa: E402,F401
from tts_cpp_amd import gguf, hip, synth  # noqa: E402

MAX_STEPS, WARM, STEPS, PROMPT, KV = 256, 32, 64, 16, 128
VOICE_LENS = [8, 11, 15, 18, 22, 25, 29, 32]
HAVE_VOICES = hasattr(hip.HipEngine, "voice_bank")


def step_leg(eng, slots, prompts, reps, voices):
    ts, stopped = [], 0
    for _ in range(reps):
        eng.stream_begin(slots, MAX_STEPS, sampling=None)
        if voices is not None:
            eng.seq_voices(np.arange(slots), voices)   # before the admission: its prefill already attends
        eng.stream_admit(list(range(slots)), prompts[:slots])
        stopped += len(eng.stream_run(WARM))
        t = time.perf_counter()
        fin = eng.stream_run(STEPS)
        ts.append((time.perf_counter() - t) / STEPS * 1e3)
        stopped += len(fin)
        eng.stream_end()
    return {"ms_per_step": round(float(np.median(ts)), 4), "runs_ms": [round(x, 4) for x in ts], "spread_ms": round(max(ts) - min(ts), 4),
            "slots_stopped_inside": stopped}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "parler_voices.json" if HAVE_VOICES else "parler_voices_parent_before.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1023)
    args = ap.parse_args()
    slots = args.slots
    cfg = synth.parler_mini(weight_type=gguf.F16, max_gen=MAX_STEPS + PROMPT)
    model = synth.build(cfg)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(3, cfg.prompt_vocab, PROMPT).astype(np.uint32) for _ in range(slots)]
    out = {"setup": {"model": "synthetic Parler-Mini (24 x 1024, 16 heads, ffn 4096, 9 x 1088 logits), fp16 weights, fp16 KV cache, no codec",
                     "voice_bank": HAVE_VOICES, "slots": slots, "own_description_positions": cfg.enc_len, "voice_positions": VOICE_LENS,
                     "prompt_ids": PROMPT, "max_steps": MAX_STEPS, "warm_steps": WARM, "timed_steps": STEPS, "reps": args.reps,
                     "timing": "host wall clock around the blocking stream_run call, median of the runs listed",
                     "command": "python profiles/parler_voices_bench.py --reps %d --slots %d" % (args.reps, slots)}}
    eng = hip.HipEngine(cfg, max_seqs=slots + 1, kv_type=gguf.F16, kv_positions=KV, flags=hip.FLAG_NO_DAC)
    eng.load(model)
    st = {"one_description": step_leg(eng, slots, prompts, args.reps, None)}
    print("one_description", json.dumps(st["one_description"]), flush=True)
    if HAVE_VOICES:
        erng = np.random.default_rng(17)
        eng.voice_bank(len(VOICE_LENS))
        for v, n in enumerate(VOICE_LENS):
            eng.voice_set(v + 1, (erng.standard_normal((n, cfg.hidden)) * 0.5).astype(np.float32))
        # leg (a) once more with the bank in place and every slot at voice 0: the same launches
        legs = [("one_description_with_bank", np.zeros(slots, dtype=np.uint32)),
                ("eight_voices", 1 + np.arange(slots, dtype=np.uint32) % len(VOICE_LENS)),
                ("one_bank_voice", np.full(slots, 3, dtype=np.uint32))]
        for name, voices in legs:
            st[name] = step_leg(eng, slots, prompts, args.reps, voices)
            print(name, json.dumps(st[name]), flush=True)
        st["eight_voices_over_one_description"] = round(st["eight_voices"]["ms_per_step"] / st["one_description"]["ms_per_step"], 4)
        st["one_bank_voice_over_one_description"] = round(st["one_bank_voice"]["ms_per_step"] / st["one_description"]["ms_per_step"], 4)
    out["step_time"] = st
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
