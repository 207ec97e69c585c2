"""Orpheus-3B Q4_0 (the synthetic shapes of secondary_bench.py): the lock-step loop through its two ways in, the fixed batch and the continuous session.

  per-step time   tts_hip_orpheus_gen_launch (the fixed batch) against tts_hip_orpheus_stream_run (the session) at 8 and 32 rows, greedy and
                  sampled (top_k 50).  Both are one run of the same loop (forward, row-batched selection and row advance enqueued back to back),
                  so the two legs time the same thing; on commits before "one Orpheus lock-step loop" gen_launch was a host-driven loop of its
                  own (three copies, two synchronises and, when sampling, up to three launches per row in every step), which is what the
                  host_driven_* keys of the older recorded files hold
  ragged mix      24 utterances at 8 slots whose lengths spread over 10:1 (RAGGED_LENGTHS): once as consecutive generate_batch groups of 8,
                  once through one session with a look-in every 28 steps; tokens/s and the share of slot-steps that carried a live utterance.
                  A pilot run looks for a stopping id whose first occurrences spread the lengths that way; when the greedy ids of the random
                  weights offer none (they did not on the recorded runs), the lengths are set through the
                  other stopping condition the two loops share, the end of the cache: a context of RAGGED_CTX positions and prompts of
                  RAGGED_CTX + 1 - length ids.

  --mixed         the mixed session (tts_hip_orpheus_stream_begin_mixed) at 8 and 32 slots, step time of tts_hip_orpheus_stream_run:
                  (a) a uniform sampled session, (b) a mixed session whose slots all sample, each with its own setting (MIXED_SETTINGS in
                  turn; the same number of launches as (a)), (c) a mixed session with every other slot greedy (two more launches per step, the
                  arg-max pair).  The legs alternate within a repetition; five repetitions, median and spread (max - min).  A build without
                  the mixed session runs (a) only: that is how orpheus_stream_mixed_parent_before.json was made.

  --many-rows     the session's step time and tokens/s at --rows slots (64,128,256 for the recorded files; 64 alone on a build whose contexts stop at
                  64 slots: orpheus_many_rows_parent_before.json), greedy, every utterance behind a prompt of --prompt ids (480: positions around
                  512 inside the timed window), --kv f16 for the fp16 cache (256 fp32 slots of 1024 positions would be 60 GB).  Five repetitions,
                  median and spread (max - min).  At the largest row count one profiled step (tts_hip_profile: eager, every launch timed) gives the
                  split between the GEMM classes and self-attention.

A build without the session (hip.OrpheusEngine has no stream_begin) runs the generate_batch / gen_launch legs only: that is how
orpheus_stream_throughput_parent_before.json was made.  Usage: python profiles/orpheus_stream_bench.py [--out FILE] [--reps N]"""
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
import secondary_bench as sb  # noqa: E402

NO_STOP = 0xFFFFFFFF
SMP = dict(top_k=50, temperature=1.0, repetition_penalty=1.0, top_p=1.0)   # the default generation_configuration
STEPS, WARM = 56, 8
LOOK_IN = 28            # orpheus_runner's look-in interval
N_RAGGED, SLOTS, CAP = 24, 8, 512
RAGGED_CTX = 448
RAGGED_LENGTHS = [40, 400, 120, 60, 280, 80, 200, 48, 360, 100, 160, 44, 240, 72, 320, 56, 140, 400, 90, 180, 52, 300, 64, 220]


def med(v):
    return float(np.median(v))


def step_times(eng, B, prompts, uni, have_session, reps):
    out = {}
    for mode in ("greedy", "sampled"):
        kw = dict(uniforms=uni[:, :WARM + STEPS + 1], **SMP) if mode == "sampled" else {}
        batch, dev = [], []
        for _ in range(reps):
            eng.gen_begin(prompts, WARM + STEPS + 1, NO_STOP, **kw)
            eng.gen_launch(WARM)
            eng.gen_wait()
            t = time.perf_counter()
            eng.gen_launch(STEPS)
            eng.gen_wait()
            batch.append((time.perf_counter() - t) / STEPS * 1e3)
            eng.gen_launch(1)
            assert all(eng.gen_wait()[1])
        out[mode] = {"gen_launch_ms_per_step": round(med(batch), 4), "gen_launch_runs_ms": [round(x, 4) for x in batch]}
        if not have_session:
            continue
        for _ in range(reps):
            eng.stream_begin(B, WARM + STEPS + 2, NO_STOP, sampled=mode == "sampled", **SMP)
            eng.stream_admit(list(range(B)), prompts, uni if mode == "sampled" else None)
            assert eng.stream_run(WARM) == []
            t = time.perf_counter()
            fin = eng.stream_run(STEPS)
            dev.append((time.perf_counter() - t) / STEPS * 1e3)
            assert fin == []
            eng.stream_end()
        out[mode].update({"stream_run_ms_per_step": round(med(dev), 4), "stream_run_runs_ms": [round(x, 4) for x in dev],
                          "stream_run_over_gen_launch": round(med(dev) / med(batch), 4)})
    return out


MIXED_SETTINGS = [dict(top_k=50, temperature=1.0), dict(top_k=40, temperature=0.6), dict(top_k=64, temperature=0.9), dict(top_k=20, temperature=1.2)]


def mixed_step_times(eng, B, prompts, uni, have_mixed, reps):
    """step time of stream_run for the legs (a), (b), (c), alternating within a repetition"""
    legs = {"a_uniform_sampled": None}
    if have_mixed:
        legs["b_mixed_all_sampled"] = [dict(MIXED_SETTINGS[s % len(MIXED_SETTINGS)], repetition_penalty=1.0, top_p=1.0) for s in range(B)]
        legs["c_mixed_half_greedy"] = [None if s % 2 else legs["b_mixed_all_sampled"][s] for s in range(B)]
    runs = {k: [] for k in legs}
    for _ in range(reps):
        for name, settings in legs.items():
            if settings is None:
                eng.stream_begin(B, WARM + STEPS + 2, NO_STOP, sampled=True, **SMP)
                eng.stream_admit(list(range(B)), prompts, uni)
            else:
                eng.stream_begin_mixed(B, WARM + STEPS + 2, NO_STOP)
                eng.stream_admit_mixed(list(range(B)), prompts, settings, uni)
            assert eng.stream_run(WARM) == []
            t = time.perf_counter()
            fin = eng.stream_run(STEPS)
            runs[name].append((time.perf_counter() - t) / STEPS * 1e3)
            assert fin == []
            eng.stream_end()
    return {k: {"stream_run_ms_per_step": round(med(v), 4), "spread_ms": round(max(v) - min(v), 4), "runs_ms": [round(x, 4) for x in v]} for k, v in runs.items()}


def mixed_main(args):
    have_mixed = hasattr(hip.OrpheusEngine, "stream_begin_mixed")
    cfg = synth.orpheus_3b(ctx=1024, weight_type=gguf.Q4_0)
    tensors, _ = sb.orpheus_tensors(cfg, np.random.default_rng(7))
    model = sb._Model(cfg, tensors)
    out = {"setup": {"model": "synthetic Orpheus-3B (28 x 3072, 24 / 8 heads x 128, ffn 8192, 156 940 logits), Q4_0, n_ctx 1024", "prompt_ids": 32, "timed_steps": STEPS,
                     "warm_steps": WARM, "reps": args.reps, "uniform_sampling": SMP, "mixed_settings": MIXED_SETTINGS, "mixed_session": have_mixed,
                     "timing": "host wall clock around the blocking tts_hip_orpheus_stream_run, median of reps, spread = max - min"},
           "per_step": {}}
    prng = np.random.default_rng(11)
    for B in [int(x) for x in args.rows.split(",")]:
        eng = hip.OrpheusEngine(cfg, max_seqs=B)
        eng.load(model)
        prompts = [prng.integers(0, cfg.vocab, 32).astype(np.uint32) for _ in range(B)]
        uni = prng.random((B, WARM + STEPS + 2), dtype=np.float32)
        eng.generate_batch(prompts, 4, NO_STOP)
        out["per_step"][str(B)] = mixed_step_times(eng, B, prompts, uni, have_mixed, args.reps)
        print(B, json.dumps(out["per_step"][str(B)]), flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def many_rows_main(args):
    flags = hip.FLAG_KV_F16 if args.kv == "f16" else 0
    cfg = synth.orpheus_3b(ctx=1024, weight_type=gguf.Q4_0)
    tensors, _ = sb.orpheus_tensors(cfg, np.random.default_rng(7))
    model = sb._Model(cfg, tensors)
    rows = [int(x) for x in args.rows.split(",")]
    out = {"setup": {"model": "synthetic Orpheus-3B (28 x 3072, 24 / 8 heads x 128, ffn 8192, 156 940 logits), Q4_0, n_ctx 1024", "kv_cache": args.kv, "prompt_ids": args.prompt,
                     "timed_steps": STEPS, "warm_steps": WARM, "reps": args.reps, "selection": "greedy",
                     "timing": "host wall clock around the blocking tts_hip_orpheus_stream_run, median of reps, spread = max - min; one context of max_seqs = rows per leg"},
           "per_step": {}}
    prng = np.random.default_rng(11)
    for B in rows:
        eng = hip.OrpheusEngine(cfg, max_seqs=B, flags=flags)
        eng.load(model)
        prompts = [prng.integers(0, cfg.vocab, args.prompt).astype(np.uint32) for _ in range(B)]
        runs = []
        for _ in range(args.reps):
            eng.stream_begin(B, WARM + STEPS + 2, NO_STOP)
            eng.stream_admit(list(range(B)), prompts)
            assert eng.stream_run(WARM) == []
            t = time.perf_counter()
            fin = eng.stream_run(STEPS)
            runs.append((time.perf_counter() - t) / STEPS * 1e3)
            assert fin == []
            eng.stream_end()
        res = {"stream_run_ms_per_step": round(med(runs), 4), "spread_ms": round(max(runs) - min(runs), 4), "runs_ms": [round(x, 4) for x in runs],
               "tokens_per_s": round(B / med(runs) * 1e3, 1), "tokens_per_s_spread": round(B / min(runs) * 1e3 - B / max(runs) * 1e3, 1)}
        if B == max(rows):
            # one eager step with every launch timed: the classes' shares of the device time (the step itself is slower than the timed ones above)
            eng.stream_begin(B, 8, NO_STOP)
            eng.stream_admit(list(range(B)), prompts)
            eng.stream_run(2)
            eng.profile(True)
            eng.stream_run(1)
            prof = {k: v for k, v in eng.profile_get().items() if v["launches"]}
            eng.profile(False)
            eng.stream_end()
            total = sum(v["ms_total"] for v in prof.values())
            res["profiled_step"] = {"rows": B, "ms_total_of_timed_launches": round(total, 4),
                                    "classes": {k: {"ms": round(v["ms_total"], 4), "launches": v["launches"], "share": round(v["ms_total"] / total, 4)} for k, v in prof.items()},
                                    "note": "launches outside the profiled classes (rms norm, rope, silu, quantisation, selection) are not in the total"}
        out["per_step"][str(B)] = res
        print(B, json.dumps(res), flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def pick_stop(pilot):
    """the id whose first occurrences give lengths closest to a 10:1 spread (10th / 90th percentile) over all utterances"""
    best, best_score = None, None
    for tok in sorted({int(t) for ids in pilot for t in ids}):
        lens = np.array([(list(ids).index(tok) + 1) if tok in ids else len(ids) for ids in pilot], dtype=np.float64)
        if lens.min() < 8:
            continue
        ratio = np.percentile(lens, 90) / np.percentile(lens, 10)
        score = abs(np.log(ratio / 10.0))
        if best_score is None or score < best_score:
            best, best_score = tok, score
    return best


def ragged(eng, prompts, stop, how, have_session, reps):
    res = {"lengths_set_by": how, "stop_id": stop, "max_new": CAP, "utterances": N_RAGGED, "slots": SLOTS}
    ts, got = [], None
    for _ in range(reps):
        t = time.perf_counter()
        got = []
        for g0 in range(0, N_RAGGED, SLOTS):
            got += [ids.tolist() for ids in eng.generate_batch(prompts[g0:g0 + SLOTS], CAP, stop)]
        ts.append(time.perf_counter() - t)
    lens = [len(g) for g in got]
    total = sum(lens)
    # a group holds its 8 slots until its longest utterance ends; an utterance's first id comes with its prompt, the others take a step each
    slot_steps = sum(SLOTS * (max(lens[g0:g0 + SLOTS]) - 1) for g0 in range(0, N_RAGGED, SLOTS))
    res["lengths"] = lens
    res["generate_batch_groups"] = {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "tokens_per_s": round(total / med(ts), 1),
                                    "live_share_of_slot_steps": round((total - N_RAGGED) / slot_steps, 4)}
    if not have_session:
        return res
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        eng.stream_begin(SLOTS, CAP, stop)
        free, slot_utt, out, nxt, runs = list(range(SLOTS)), {}, [None] * N_RAGGED, 0, 0
        while nxt < N_RAGGED or slot_utt:
            while nxt < N_RAGGED and free:
                s = free.pop(0)
                eng.stream_admit([s], [prompts[nxt]])
                slot_utt[s] = nxt
                nxt += 1
            fin = eng.stream_run(LOOK_IN)
            runs += 1
            for s, cnt in fin:
                out[slot_utt.pop(s)] = eng.stream_collect(s, cnt).tolist()
                free.append(s)
        eng.stream_end()
        ts.append(time.perf_counter() - t)
    slens = [len(o) for o in out]
    res["session"] = {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "tokens_per_s": round(sum(slens) / med(ts), 1), "look_in_steps": LOOK_IN,
                      "runs": runs, "live_share_of_slot_steps": round((sum(slens) - N_RAGGED) / (SLOTS * LOOK_IN * runs), 4),
                      "utterances_with_generate_batch_ids": sum(a == b for a, b in zip(out, got)), "lengths": slens,
                      "speedup_over_groups": round(res["generate_batch_groups"]["seconds"] / med(ts), 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "orpheus_stream_throughput.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default="8,32")
    ap.add_argument("--mixed", action="store_true", help="the legs of the mixed session instead (--reps 5 for the recorded files)")
    ap.add_argument("--many-rows", action="store_true", help="session step time and tokens/s at --rows slots (--reps 5, --kv f16 for the recorded files)")
    ap.add_argument("--kv", default="f32", choices=["f32", "f16"], help="K/V cache element type of the --many-rows legs")
    ap.add_argument("--prompt", type=int, default=480, help="prompt ids per utterance of the --many-rows legs")
    args = ap.parse_args()
    if args.mixed:
        return mixed_main(args)
    if args.many_rows:
        return many_rows_main(args)
    have_session = hasattr(hip.OrpheusEngine, "stream_begin")
    cfg = synth.orpheus_3b(ctx=1024, weight_type=gguf.Q4_0)
    rng = np.random.default_rng(7)
    tensors, _ = sb.orpheus_tensors(cfg, rng)
    model = sb._Model(cfg, tensors)
    out = {"setup": {"model": "synthetic Orpheus-3B (28 x 3072, 24 / 8 heads x 128, ffn 8192, 156 940 logits), Q4_0, n_ctx 1024", "prompt_ids": 32, "timed_steps": STEPS,
                     "warm_steps": WARM, "reps": args.reps, "sampling": SMP, "session": have_session, "timing": "host wall clock around the blocking calls, median of reps"},
           "per_step": {}, "ragged_mix": {}}
    prng = np.random.default_rng(11)
    for B in [int(x) for x in args.rows.split(",")]:
        eng = hip.OrpheusEngine(cfg, max_seqs=B)
        eng.load(model)
        prompts = [prng.integers(0, cfg.vocab, 32).astype(np.uint32) for _ in range(B)]
        uni = prng.random((B, WARM + STEPS + 2), dtype=np.float32)
        eng.generate_batch(prompts, 4, NO_STOP)
        out["per_step"][str(B)] = step_times(eng, B, prompts, uni, have_session, args.reps)
        print(B, json.dumps(out["per_step"][str(B)]), flush=True)
        if B == SLOTS:
            rp = [prng.integers(0, cfg.vocab, 32).astype(np.uint32) for _ in range(N_RAGGED)]
            pilot = []
            for g0 in range(0, N_RAGGED, SLOTS):
                pilot += [ids.tolist() for ids in eng.generate_batch(rp[g0:g0 + SLOTS], CAP, NO_STOP)]
            stop = pick_stop(pilot)
            if stop is not None:
                out["ragged_mix"] = ragged(eng, rp, stop, "a stopping id chosen from the pilot run", have_session, args.reps)
            else:
                eng.close()
                cfg2 = synth.orpheus_3b(ctx=RAGGED_CTX, weight_type=gguf.Q4_0)
                eng = hip.OrpheusEngine(cfg2, max_seqs=B)
                eng.load(sb._Model(cfg2, tensors))
                rp = [prng.integers(0, cfg.vocab, RAGGED_CTX + 1 - n).astype(np.uint32) for n in RAGGED_LENGTHS]
                out["ragged_mix"] = ragged(eng, rp, NO_STOP, "the end of a cache of %d positions (the pilot run found no usable stopping id)" % RAGGED_CTX, have_session, args.reps)
                assert out["ragged_mix"]["lengths"] == RAGGED_LENGTHS
            print("ragged", json.dumps(out["ragged_mix"]), flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
