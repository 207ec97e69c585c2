"""Dia-1.6B shapes, 4 slots (the model, texts and lengths of dia_stream_bench.py): what carrying a sampler per slot costs.

  (a) step time     all 4 slots live, positions WARM .. WARM + STEPS as in dia_stream_bench.py:
                      uniform session, sampler::max (argmax_kernel)           — the leg dia_stream_bench.py measures, repeated here
                      mixed session, every slot greedy (sample_kernel, the record says sampler::max)
                      uniform session, every slot sampled with top_k 50 (sample_kernel, settings in the launch)
                      mixed session, every slot sampled with top_k 50 (sample_kernel, settings in the records)
                    The yardstick is the parent commit's run of dia_stream_bench.py (dia_stream_mixed_parent_before.json): its session step and
                    the run-to-run spread of its legs.
  (b) ragged mix    the 12 utterances of dia_stream_bench.py (10:1 lengths) through one mixed session: with identical settings (all greedy, and
                    all top_k 50: a sampled row's selection costs more than an arg-max in either kind of session), and with per-request settings (greedy, top_k 50, top_k 8 with a repetition penalty, top_k 20 + top_p 0.9 at
                    temperature 0.8, in turn).  The head rows of the special ids are zero, but a sampled utterance may still draw one, so the
                    lengths are read back and the audio-seconds counted from them.
Usage: python profiles/dia_stream_mixed_bench.py [--out FILE] [--reps N] [--mix-reps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import tts_cpp_amd  # noqa: E402,F401
from tts_cpp_amd import gguf, hip, synth  # noqa: E402
from dia_stream_bench import FRAMES_PER_S, LENGTHS, LOOK_IN, N_RAGGED, SLOTS, STEPS, TEXT_LEN, WARM, build_model, med  # noqa: E402

TOPK50 = dict(top_k=50)
PER_REQUEST = [None, dict(top_k=50), dict(top_k=8, repetition_penalty=1.3), dict(top_k=20, top_p=0.9, temperature=0.8, repetition_penalty=1.1)]


def step_leg(eng, a, toks, uni, reps, mixed, setting):
    cfg = eng.cfg
    ts, stopped = [], 0
    for _ in range(reps + 1):               # the first repetition captures the graph and is dropped
        if mixed:
            eng.stream_begin_mixed(SLOTS, cfg.max_gen, **a)
            eng.stream_admit_mixed(list(range(SLOTS)), [toks] * SLOTS, [TEXT_LEN] * SLOTS, [setting] * SLOTS, uniforms=None if setting is None else uni)
        else:
            eng.stream_begin(SLOTS, cfg.max_gen, sampled=setting is not None, **(setting or {}), **a)
            eng.stream_admit(list(range(SLOTS)), [toks] * SLOTS, [TEXT_LEN] * SLOTS, uniforms=None if setting is None else uni)
        stopped += len(eng.stream_run(WARM))
        t = time.perf_counter()
        fin = eng.stream_run(STEPS)
        ts.append((time.perf_counter() - t) / STEPS * 1e3)
        stopped += len(fin)                 # a sampled slot may draw EOS and park inside the timed steps: counted, so that the reader knows
        assert setting is not None or fin == []
        eng.stream_end()
    ts = ts[1:]
    return {"ms_per_step": round(med(ts), 4), "runs_ms": [round(x, 4) for x in ts], "spread_ms": round(max(ts) - min(ts), 4), "slots_stopped_inside": stopped}


def ragged(eng, a, texts, uni, reps, settings):
    cfg = eng.cfg
    budgets = [n + 1 for n in LENGTHS]
    ts, runs, lens = [], 0, None
    for _ in range(reps):
        t = time.perf_counter()
        eng.stream_begin_mixed(SLOTS, cfg.max_gen, **a)
        free, slot_utt, lens, nxt, steps_run = list(range(SLOTS)), {}, [0] * N_RAGGED, 0, 0
        while nxt < N_RAGGED or slot_utt:
            take = []
            while nxt < N_RAGGED and free:
                take.append((free.pop(0), nxt))
                nxt += 1
            if take:
                st = [settings[u] for _, u in take]
                eng.stream_admit_mixed([s for s, _ in take], [texts[u] for _, u in take], [TEXT_LEN] * len(take), st, budgets=[budgets[u] for _, u in take],
                                       uniforms=None if all(x is None for x in st) else uni[:len(take)])
                slot_utt.update(take)
            fin = eng.stream_run(LOOK_IN)
            steps_run += LOOK_IN
            for s, n in fin:
                lens[slot_utt.pop(s)] = n
                free.append(s)
        eng.stream_end()
        ts.append(time.perf_counter() - t)
        runs = steps_run
    frames = sum(max(n - cfg.max_delay, 0) for n in lens)
    return {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "look_in_steps": LOOK_IN, "steps_run_upper_bound": runs, "lengths_steps": lens,
            "audio_seconds": round(frames / FRAMES_PER_S, 3), "audio_seconds_per_s": round(frames / FRAMES_PER_S / med(ts), 3),
            "live_share_of_slot_steps": round(sum(lens) / (SLOTS * runs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "dia_stream_mixed.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mix-reps", type=int, default=3)
    args = ap.parse_args()
    cfg = synth.dia_1_6b(weight_type=gguf.F16)
    rng = np.random.default_rng(3)
    eng = hip.DiaEngine(cfg, max_utterances=SLOTS)
    eng.load(build_model(cfg, rng))
    a = dict(delay_pattern=[0, 8, 9, 10, 11, 12, 13, 14, 15], bos=cfg.bos, eos=cfg.eos, pad=cfg.pad, max_delay=cfg.max_delay)
    texts = []
    for _ in range(N_RAGGED):
        t = np.zeros(cfg.max_ctx, dtype=np.uint32)
        t[:TEXT_LEN] = rng.integers(32, 127, TEXT_LEN)
        texts.append(t)
    uni = np.random.default_rng(7).random((SLOTS, cfg.max_gen, cfg.n_out), dtype=np.float32)
    out = {"setup": {"model": "synthetic Dia-1.6B (encoder 12 x 1024, decoder 18 x 2048, 16 / 4 heads x 128, ffn 8192, 9 x 1028 logits), fp16, 4 slots = 8 rows",
                     "text_bytes": TEXT_LEN, "warm_steps": WARM, "timed_steps": STEPS, "reps": args.reps, "mix_reps": args.mix_reps,
                     "timing": "host wall clock around the blocking calls, median of the runs listed; the first repetition of a step leg is dropped",
                     "command": "python profiles/dia_stream_mixed_bench.py --reps %d --mix-reps %d" % (args.reps, args.mix_reps)}}
    st = {}
    for name, mixed, setting in (("uniform_greedy", False, None), ("mixed_all_greedy", True, None), ("uniform_sampled_top_k_50", False, TOPK50),
                                 ("mixed_all_sampled_top_k_50", True, TOPK50)):
        st[name] = step_leg(eng, a, texts[0], uni, args.reps, mixed, setting)
        print("step", name, json.dumps(st[name]), flush=True)
    st["mixed_greedy_minus_uniform_greedy_ms"] = round(st["mixed_all_greedy"]["ms_per_step"] - st["uniform_greedy"]["ms_per_step"], 4)
    st["mixed_greedy_over_uniform_greedy"] = round(st["mixed_all_greedy"]["ms_per_step"] / st["uniform_greedy"]["ms_per_step"], 4)
    st["mixed_sampled_minus_uniform_sampled_ms"] = round(st["mixed_all_sampled_top_k_50"]["ms_per_step"] - st["uniform_sampled_top_k_50"]["ms_per_step"], 4)
    st["mixed_sampled_over_uniform_sampled"] = round(st["mixed_all_sampled_top_k_50"]["ms_per_step"] / st["uniform_sampled_top_k_50"]["ms_per_step"], 4)
    out["step_time"] = st
    mix = {"utterances": N_RAGGED, "slots": SLOTS, "budgets_steps": [n + 1 for n in LENGTHS]}
    mix["identical_settings"] = ragged(eng, a, texts, uni, args.mix_reps, [None] * N_RAGGED)
    print("ragged identical", json.dumps(mix["identical_settings"]), flush=True)
    mix["identical_settings_sampled_top_k_50"] = ragged(eng, a, texts, uni, args.mix_reps, [TOPK50] * N_RAGGED)
    print("ragged identical sampled", json.dumps(mix["identical_settings_sampled_top_k_50"]), flush=True)
    mix["per_request_settings"] = ragged(eng, a, texts, uni, args.mix_reps, [PER_REQUEST[u % len(PER_REQUEST)] for u in range(N_RAGGED)])
    mix["per_request_settings"]["settings"] = [PER_REQUEST[u % len(PER_REQUEST)] for u in range(N_RAGGED)]
    print("ragged per-request", json.dumps(mix["per_request_settings"]), flush=True)
    mix["per_request_over_identical_audio_s_per_s"] = round(mix["per_request_settings"]["audio_seconds_per_s"] / mix["identical_settings"]["audio_seconds_per_s"], 4)
    mix["per_request_over_identical_sampled_audio_s_per_s"] = round(mix["per_request_settings"]["audio_seconds_per_s"] /
                                                                    mix["identical_settings_sampled_top_k_50"]["audio_seconds_per_s"], 4)
    out["ragged_mix"] = mix
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
