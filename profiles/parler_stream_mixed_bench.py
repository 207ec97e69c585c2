"""Parler-Mini shapes, fp16 weights and KV cache, no codec: what carrying a sampler per slot costs the continuous session.

  (a) step time     every slot live (255 and 1023 slots: forwards of 256 and 1024 rows), 16-id prompts, a warm-up run of WARM steps (it captures
                    the graph), then STEPS timed steps of one stream_run:
                      uniform session, sampler::max (argmax_kernel)
                      uniform session, every slot sampled with top_k 50 (sample_kernel, settings in the launch)
                      mixed session, every slot greedy (the run replays the uniform greedy graph)
                      mixed session, every slot sampled with top_k 50 (sample_kernel, settings in the records)
                      mixed session, half the slots greedy, the others dealt top_k 50 / top_k 8 with a repetition penalty / top_k 20 + top_p 0.9 at
                      temperature 0.8
                    On a build without the mixed session (the parent commit) only the two uniform legs run; that file is the yardstick, and the
                    run-to-run spread of its legs the margin.
  (b) admission     one admission of 64 sampled utterances into an empty session of 255 slots: prefill side batch + the slots' state
  (c) runner        Runner.generate_stream(texts, configs=...) with 24 requests alternating two temperatures, in audio-s/s (--runner; a build
                    without stream_accepts runs them as consecutive sessions)
Usage: python profiles/parler_stream_mixed_bench.py [--out FILE] [--reps N] [--slots 255,1023] [--runner]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tts_cpp_amd  # noqa: E402,F401
from tts_cpp_amd import gguf, hip, synth  # noqa: E402

MAX_STEPS, WARM, STEPS, PROMPT, KV = 256, 32, 64, 16, 128
TOPK50 = dict(top_k=50)
PER_REQUEST = [None, dict(top_k=50), None, dict(top_k=8, repetition_penalty=1.3), None, dict(top_k=20, top_p=0.9, temperature=0.8, repetition_penalty=1.1), None, dict(top_k=50)]
HAVE_MIXED = hasattr(hip.HipEngine, "stream_begin_mixed")


def med(xs):
    return float(np.median(xs))


def _tuple(s):
    return (s.get("top_k", 50), s.get("top_p", 1.0), s.get("temperature", 1.0), s.get("repetition_penalty", 1.0))


def open_and_admit(eng, slots, which, prompts, uni, mixed, settings):
    """a session with slots[which] admitted in one call -> seconds the admission took"""
    sampled = any(s is not None for s in settings)
    if mixed:
        eng.stream_begin_mixed(slots, MAX_STEPS)
    else:
        assert len({None if s is None else _tuple(s) for s in settings}) == 1
        eng.stream_begin(slots, MAX_STEPS, sampling=_tuple(settings[0]) if sampled else None)
    t = time.perf_counter()
    if mixed:
        eng.stream_admit_mixed(which, prompts, settings, uni if sampled else None)
    else:
        eng.stream_admit(which, prompts, uni if sampled else None)
    return time.perf_counter() - t


def step_leg(eng, slots, prompts, uni, reps, mixed, settings):
    ts, stopped = [], 0
    for _ in range(reps):
        open_and_admit(eng, slots, list(range(slots)), prompts[:slots], uni[:slots], mixed, settings[:slots])
        stopped += len(eng.stream_run(WARM))
        t = time.perf_counter()
        fin = eng.stream_run(STEPS)
        ts.append((time.perf_counter() - t) / STEPS * 1e3)
        stopped += len(fin)
        eng.stream_end()
    return {"ms_per_step": round(med(ts), 4), "runs_ms": [round(x, 4) for x in ts], "spread_ms": round(max(ts) - min(ts), 4), "slots_stopped_inside": stopped}


def admit_leg(eng, slots, prompts, uni, reps, mixed):
    ts = []
    for _ in range(reps + 1):   # the first allocates the staging copies
        ts.append(open_and_admit(eng, slots, list(range(64)), prompts[:64], uni[:64], mixed, [TOPK50] * 64) * 1e3)
        eng.stream_end()
    ts = ts[1:]
    return {"ms": round(med(ts), 3), "runs_ms": [round(x, 3) for x in ts], "spread_ms": round(max(ts) - min(ts), 3), "utterances": 64, "slots": slots}


def runner_leg(cfg, model, reps):
    from tts_cpp_amd import runner
    path = model.write_gguf(os.path.join(tempfile.mkdtemp(prefix="parler_stream_mixed_"), "mini.gguf"))
    rng = np.random.default_rng(11)
    texts = [" ".join("w%d" % rng.integers(0, 50) for _ in range(int(rng.integers(4, 12)))) for _ in range(24)]
    configs = [dict(sample=1, seed=3 + i, top_k=50, temperature=(0.8, 1.1)[i % 2]) for i in range(24)]
    r = runner.Runner(path, max_seqs=25, sample=0)
    r.generate_stream(texts[:4], configs=configs[:4])   # warm-up: the session's buffers and graphs
    ts, samples = [], 0
    for _ in range(reps):
        t = time.perf_counter()
        out = r.generate_stream(texts, configs=configs)
        ts.append(time.perf_counter() - t)
        samples = sum(a.size for a in out)
    rate = r.sampling_rate
    r.close()
    os.remove(path)
    return {"requests": 24, "temperatures": [0.8, 1.1], "rows": 24, "seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts],
            "audio_seconds": round(samples / rate, 3), "audio_seconds_per_s": round(samples / rate / med(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "parler_stream_mixed.json" if HAVE_MIXED else "parler_stream_mixed_parent_before.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", default="255,1023")
    ap.add_argument("--runner", action="store_true")
    args = ap.parse_args()
    slot_counts = [int(s) for s in args.slots.split(",")]
    cfg = synth.parler_mini(weight_type=gguf.F16, max_gen=MAX_STEPS + PROMPT)
    model = synth.build(cfg)
    rng = np.random.default_rng(3)
    top = max(slot_counts)
    prompts = [rng.integers(3, cfg.prompt_vocab, PROMPT).astype(np.uint32) for _ in range(top)]
    uni = np.random.default_rng(7).random((top, MAX_STEPS, cfg.n_out), dtype=np.float32)
    out = {"setup": {"model": "synthetic Parler-Mini (24 x 1024, 16 heads, ffn 4096, 9 x 1088 logits), fp16 weights, fp16 KV cache, no codec",
                     "mixed_session": HAVE_MIXED, "prompt_ids": PROMPT, "max_steps": MAX_STEPS, "warm_steps": WARM, "timed_steps": STEPS, "reps": args.reps,
                     "timing": "host wall clock around the blocking stream_run / stream_admit call, median of the runs listed",
                     "command": "python profiles/parler_stream_mixed_bench.py --reps %d --slots %s%s" % (args.reps, args.slots, " --runner" if args.runner else "")}}
    for slots in slot_counts:
        eng = hip.HipEngine(cfg, max_seqs=slots + 1, kv_type=gguf.F16, kv_positions=KV, flags=hip.FLAG_NO_DAC)
        eng.load(model)
        legs = [("uniform_greedy", False, [None] * slots), ("uniform_sampled_top_k_50", False, [TOPK50] * slots)]
        if HAVE_MIXED:
            legs += [("mixed_all_greedy", True, [None] * slots), ("mixed_all_sampled_top_k_50", True, [TOPK50] * slots),
                     ("mixed_half_greedy_four_settings", True, [PER_REQUEST[u % len(PER_REQUEST)] for u in range(slots)])]
        st = {}
        for name, mixed, settings in legs:
            st[name] = step_leg(eng, slots, prompts, uni, args.reps, mixed, settings)
            print("step", slots, name, json.dumps(st[name]), flush=True)
        if HAVE_MIXED:
            st["mixed_greedy_minus_uniform_greedy_ms"] = round(st["mixed_all_greedy"]["ms_per_step"] - st["uniform_greedy"]["ms_per_step"], 4)
            st["mixed_sampled_minus_uniform_sampled_ms"] = round(st["mixed_all_sampled_top_k_50"]["ms_per_step"] - st["uniform_sampled_top_k_50"]["ms_per_step"], 4)
        out["step_time_%d_slots" % slots] = st
        if slots == min(slot_counts):
            adm = {"uniform_sampled": admit_leg(eng, slots, prompts, uni, args.reps, False)}
            if HAVE_MIXED:
                adm["mixed_sampled"] = admit_leg(eng, slots, prompts, uni, args.reps, True)
            out["admission_64"] = adm
            print("admission", json.dumps(adm), flush=True)
        eng.close()
    if args.runner:
        out["runner_two_temperatures"] = runner_leg(cfg, model, 3)
        print("runner", json.dumps(out["runner_two_temperatures"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
