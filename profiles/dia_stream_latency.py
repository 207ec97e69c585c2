"""Chunked Dia audio latency (dia_runner::generate_chunked / generate_batch_chunked): synthetic Dia-1.6B (synth.dia_1_6b, every layer, fp16
matrices, F32 codec, head rows of the special ids zeroed so that a greedy utterance runs its whole max_generation_size), one utterance and a
lock-step batch of 4.

The one-call part needs nothing of the chunked code, so the same script measures a commit without it (--one-call-only): the encode pass and
the mean step of the device loop (tts_hip_dia_generate on the engine) and generate() / generate_batch() on the runner, `reps` runs each.
The chunked part: time to the first chunk and total time of the chunked calls at chunk_frames 16 / 32 / 64, against the one-call totals of
the same process and against the floor  encode + ceil((chunk_frames + h + max_delay) / 16) * 16 mean steps + one window pass  (step time
from --baseline, the one-call JSON of the commit to compare with, when given).  Writes one JSON (default profiles/dia_stream_latency.json).

    python profiles/dia_stream_latency.py [--out FILE] [--reps 7] [--one-call-only] [--baseline FILE ...] [--max-gen 3072]
"""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tts_cpp_amd  # noqa: E402,F401
from tts_cpp_amd import gguf, hip, runner, synth  # noqa: E402

SR = 44100.0
LOOK_IN = 16
TEXTS = ["[S1] The birch canoe slid on the smooth planks. [S2] Glue the sheet to the dark blue background. [S1] It is easy to tell the depth of a well.",
         "[S2] These days a chicken leg is a rare dish. [S1] Rice is often served in round bowls. [S2] The juice of lemons makes fine punch.",
         "[S1] The box was thrown beside the parked truck. [S2] The hogs were fed chopped corn and garbage. [S1] Four hours of steady work faced us.",
         "[S2] A large size in stockings is hard to sell. [S1] The boy was there when the sun rose. [S2] A rod is used to catch pink salmon."]


def say(*a):
    print(*a, flush=True)


def stats(ts):
    ts = [float(t) for t in ts]
    return {"median_s": round(float(np.median(ts)), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5), "runs_s": [round(t, 5) for t in ts]}


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.monotonic()
        fn()
        out.append(time.monotonic() - t0)
    return out


def engine_part(model, max_gen, reps):
    """encode and the device loop on the bare engine: ms per encode, mean ms per step over a whole generation, 1 and 4 utterances"""
    cfg = model.cfg
    eng = hip.DiaEngine(cfg, max_utterances=4)
    eng.load(model)
    toks = [runner.dia_tokenize(t, cfg.max_ctx) for t in TEXTS]
    for u, (t, n) in enumerate(toks):
        eng.encode_slot(u, t, n)
    enc = timed(lambda: eng.encode_slot(0, *toks[0]), max(3, reps))
    args = dict(delay_pattern=synth.DIA_DELAY_PATTERN, bos=cfg.bos, eos=cfg.eos, pad=cfg.pad, max_delay=cfg.max_delay)
    out = {"encode_ms": round(float(np.median(enc)) * 1e3, 3)}
    for n_utt in (1, 4):
        steps = len(eng.generate(n_utt, max_gen, **args)[0])   # warm-up: capture
        ts = timed(lambda: eng.generate(n_utt, max_gen, **args), 2)
        out[f"loop_ms_per_step_{n_utt}"] = round(min(ts) / steps * 1e3, 5)
        out["steps"] = steps
        say(f"engine: {n_utt} utterance(s), {steps} steps, {out[f'loop_ms_per_step_{n_utt}']} ms per step")
    eng.close()
    return out


def window_pass_ms(model, frames_list, reps):
    """one tts_hip_dac_decode_windows pass over the first windows of a chunked call (clipped at the utterance's start)"""
    dcfg = dataclasses.replace(model.dac.cfg, max_gen=4096)   # the codec context's frame capacity; the tensors do not depend on it
    eng = hip.HipEngine(dcfg, flags=hip.FLAG_NO_PARLER)
    eng.load(model.dac)
    h = eng.dac_halo_frames()
    rng = np.random.default_rng(5)
    out = {}
    for n_utt in (1, 4):
        for cf in frames_list:
            wins = [(rng.integers(0, dcfg.cb_size, (cf + h, dcfg.n_out)).astype(np.uint32), 0, cf) for _ in range(n_utt)]
            eng.dac_decode_windows(wins)
            out[f"{n_utt}x{cf}"] = round(float(np.median(timed(lambda: eng.dac_decode_windows(wins), max(3, reps)))) * 1e3, 3)
    eng.close()
    return h, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dia_stream_latency.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-gen", type=int, default=3072)
    ap.add_argument("--one-call-only", action="store_true", help="skip the chunked part (a commit without chunked Dia audio)")
    ap.add_argument("--baseline", nargs="*", default=[], help="one-call JSONs of the commit to compare with (its runs before and after this one)")
    args = ap.parse_args()

    cfg = synth.dia_1_6b(weight_type=gguf.F16, max_gen=args.max_gen)
    t0 = time.monotonic()
    model = synth.build_dia(cfg, suppress_special=True, pooled=True)
    path = os.path.join(tempfile.gettempdir(), f"tts_dia_stream_latency_{os.getpid()}.gguf")
    model.write_gguf(path)
    say(f"model written in {time.monotonic() - t0:.1f} s")
    out = {"setup": {"model": "synthetic Dia-1.6B (encoder 12 x 1024, decoder 18 x 2048, 9 heads x 1028 logits)", "matrices": "fp16", "codec": "F32",
                     "max_generation_size": args.max_gen, "max_delay": cfg.max_delay, "look_in_steps": LOOK_IN, "reps": args.reps, "greedy": True}}

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)

    try:
        out["engine"] = engine_part(model, args.max_gen, args.reps)
        save()
        r = runner.Runner(path, sample=0, max_seqs=4)
        say("runner loaded")
        ref = r.generate(TEXTS[0])   # warm-up: graph, codec buffers
        steps = r.last_tokens(1).size // cfg.n_out
        one = {"steps": steps, "frames": ref.size // cfg.hop, "audio_s": round(ref.size / SR, 3)}
        one["generate"] = stats(timed(lambda: r.generate(TEXTS[0]), args.reps))
        say("generate():", one["generate"])
        ref_b = r.generate_batch(TEXTS)
        one["generate_batch"] = stats(timed(lambda: r.generate_batch_sizes(TEXTS), args.reps))
        say("generate_batch():", one["generate_batch"])
        out["one_call"] = one
        save()

        if not args.one_call_only:
            base = [json.load(open(p)) for p in args.baseline]
            h, win = window_pass_ms(model, (16, 32, 64), args.reps)
            out["setup"]["halo_frames"] = h
            out["window_pass_ms"] = win
            step_ms = {n: (float(np.mean([b["engine"][f"loop_ms_per_step_{n}"] for b in base])) if base else out["engine"][f"loop_ms_per_step_{n}"]) for n in (1, 4)}
            out["floor_step_ms"] = {"source": "baseline one-call runs" if base else "this process", "1": round(step_ms[1], 5), "4": round(step_ms[4], 5)}
            if base:
                out["baseline_one_call"] = [{"engine": b["engine"], "generate": b["one_call"]["generate"], "generate_batch": b["one_call"]["generate_batch"]} for b in base]
                for key in ("generate", "generate_batch"):
                    lo = min(b["one_call"][key]["min_s"] for b in base)
                    hi = max(b["one_call"][key]["max_s"] for b in base)
                    med = one[key]["median_s"]
                    out[f"{key}_vs_baseline"] = {"baseline_range_s": [lo, hi], "median_s": med, "inside": bool(lo <= med <= hi),
                                                 "us_per_step_vs_baseline_median": round((med - float(np.median([b["one_call"][key]["median_s"] for b in base]))) / steps * 1e6, 3)}

            def floor_ms(n_utt, cf):
                return out["engine"]["encode_ms"] * n_utt + -(-(cf + h + cfg.max_delay) // LOOK_IN) * LOOK_IN * step_ms[n_utt] + win[f"{n_utt}x{cf}"]

            for name, n_utt, call, ref_total, ref_size in (
                    ("single_utterance", 1, lambda cf: [(a, t) for a, t in r.generate_chunked(TEXTS[0], chunk_frames=cf)], one["generate"]["median_s"], ref.size),
                    ("batch_of_4", 4, lambda cf: [(a, t) for _, a, t in r.generate_batch_chunked(TEXTS, chunk_frames=cf)], one["generate_batch"]["median_s"],
                     sum(a.size for a in ref_b))):
                res = {}
                for cf in (16, 32, 64):
                    call(cf)   # warm-up
                    runs = []
                    for _ in range(args.reps):
                        t0 = time.monotonic()
                        ch = call(cf)
                        t1 = time.monotonic()
                        assert sum(a.size for a, _ in ch) == ref_size
                        runs.append((ch[0][1] - t0, t1 - t0, len(ch)))
                    first, total = float(np.median([x[0] for x in runs])), float(np.median([x[1] for x in runs]))
                    res[f"chunk_frames_{cf}"] = {"first_chunk_ms": round(first * 1e3, 2), "first_chunk_ms_runs": [round(x[0] * 1e3, 2) for x in runs],
                                                 "floor_ms": round(floor_ms(n_utt, cf), 2), "first_vs_floor": round(first * 1e3 / floor_ms(n_utt, cf), 3),
                                                 "total_s": round(total, 5), "total_s_runs": [round(x[1], 5) for x in runs],
                                                 "total_vs_one_call": round(total / ref_total, 4), "chunks": runs[0][2]}
                    say(name, cf, res[f"chunk_frames_{cf}"])
                    out[name] = res
                    save()
        r.close()
    finally:
        if os.path.exists(path):
            os.remove(path)
    save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
