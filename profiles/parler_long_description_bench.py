"""Parler-Mini shapes, fp16 weights and KV cache, no codec, 1023 slots (forwards of 1024 rows), greedy: what a description of more than 32
positions costs a step of the continuous session today.  A voice of the bank holds at most 32 positions (attn_short_body), so a longer
description can only be the context's own (tts_hip_parler_set_text_encoding); its cross-attention then leaves the fold inside the q
projection's tiles and runs the general attn_kernel as a launch of its own.  Set up as profiles/parler_voices_bench.py: 16-id prompts, a
warm-up run of WARM steps (it captures the graph), then STEPS timed steps of one stream_run; REPS repetitions, median with min .. max.

  own_8 / own_40 / own_100   every slot on the context's own description of 8, 40, 100 positions at the defaults

The figures are the baseline a bank of longer voices has to be held against.  Two processes of one build a minute apart on one
machine differed by 0.04 ms per step, all legs together: compare legs of one process, or repeat the processes in turn.
Usage: python profiles/parler_long_description_bench.py [--out FILE] [--reps N] [--slots N]"""
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
OWN_LENS = [8, 40, 100]


def step_leg(eng, slots, prompts, reps):
    ts, stopped = [], 0
    for _ in range(reps):
        eng.stream_begin(slots, MAX_STEPS, sampling=None)
        eng.stream_admit(list(range(slots)), prompts[:slots])
        stopped += len(eng.stream_run(WARM))
        t = time.perf_counter()
        fin = eng.stream_run(STEPS)
        ts.append((time.perf_counter() - t) / STEPS * 1e3)
        stopped += len(fin)
        eng.stream_end()
    return {"ms_per_step": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "runs_ms": [round(x, 4) for x in ts], "slots_stopped_inside": stopped}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "parler_long_description.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1023)
    args = ap.parse_args()
    slots = args.slots
    cfg = synth.parler_mini(weight_type=gguf.F16, max_gen=MAX_STEPS + PROMPT)
    model = synth.build(cfg)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(3, cfg.prompt_vocab, PROMPT).astype(np.uint32) for _ in range(slots)]
    erng = np.random.default_rng(17)
    out = {"setup": {"model": "synthetic Parler-Mini (24 x 1024, 16 heads, ffn 4096, 9 x 1088 logits), fp16 weights, fp16 KV cache, no codec",
                     "slots": slots, "own_description_positions": OWN_LENS, "prompt_ids": PROMPT, "max_steps": MAX_STEPS,
                     "warm_steps": WARM, "timed_steps": STEPS, "reps": args.reps,
                     "timing": "host wall clock around the blocking stream_run call, median of the runs listed, min and max beside it",
                     "command": "python profiles/parler_long_description_bench.py --reps %d --slots %d" % (args.reps, slots)}}
    eng = hip.HipEngine(cfg, max_seqs=slots + 1, kv_type=gguf.F16, kv_positions=KV, flags=hip.FLAG_NO_DAC)
    eng.load(model)
    st = {}
    for n in OWN_LENS:
        eng.set_text_encoding((erng.standard_normal((n, cfg.hidden)) * 0.5).astype(np.float32))
        st["own_%d" % n] = step_leg(eng, slots, prompts, args.reps)
        print("own_%d" % n, json.dumps(st["own_%d" % n]), flush=True)
    eng.close()
    base = st["own_8"]["ms_per_step"]
    for n in OWN_LENS[1:]:
        st["own_%d_over_own_8" % n] = round(st["own_%d" % n]["ms_per_step"] / base, 4)
    out["step_time"] = st
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
