"""Chunked audio latency (parler_runner::generate_chunked): synthetic Parler-Mini, fp16 matrices, F32 codec, the bench's 16-id prompts and
256 audio steps.  One utterance: time to the first chunk, every chunk's arrival and the total wall time at chunk_frames 16 / 32 / 64, against
generate() on the same runner (after a warm-up).  A lock-step batch of 64: audio-s/s of generate_batch_chunked against generate_batch.
Writes one JSON (default profiles/stream_latency.json).

    python profiles/stream_latency.py [--out profiles/stream_latency.json] [--reps 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tts_cpp_amd  # noqa: E402,F401
from tts_cpp_amd import gguf, runner, synth  # noqa: E402

from bench import make_sentences  # noqa: E402  (the bench's exact-length pseudo-sentences)

SR = 44100.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_latency.json"))
    ap.add_argument("--prompt-len", type=int, default=16)
    ap.add_argument("--audio-steps", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    cfg = synth.parler_mini(weight_type=gguf.F16, dac_f16=False, max_gen=args.prompt_len + args.audio_steps)
    path = os.path.join(tempfile.gettempdir(), f"tts_stream_latency_{args.prompt_len + args.audio_steps}.gguf")
    synth.build(cfg).write_gguf(path)
    r = runner.Runner(path, sample=0, max_seqs=args.batch)
    text = make_sentences(r, 1, args.prompt_len, 77)[0]
    texts = make_sentences(r, args.batch, args.prompt_len, 78)
    out = {"setup": {"model": "synthetic Parler-Mini (24 layers, hidden 1024, 9 heads)", "matrices": "fp16", "codec": "F32", "prompt_ids": args.prompt_len,
                     "audio_steps": args.audio_steps, "look_in_steps": 32, "reps": args.reps, "halo_frames": 10}}

    # one utterance
    r.generate(text)                       # warm-up: graphs, codec buffers
    for cf in (16, 32, 64):
        r.generate_chunked(text, chunk_frames=cf)
    ref = r.generate(text)
    t_gen = []
    for _ in range(args.reps):
        t0 = time.monotonic()
        r.generate(text)
        t_gen.append(time.monotonic() - t0)
    single = {"generate_s": round(float(np.median(t_gen)), 4), "audio_s": round(ref.size / SR, 3)}
    for cf in (16, 32, 64):
        runs = []
        for _ in range(args.reps):
            t0 = time.monotonic()
            ch = r.generate_chunked(text, chunk_frames=cf)
            t1 = time.monotonic()
            pcm = np.concatenate([a for a, _ in ch])
            runs.append({"total_s": t1 - t0, "first_s": ch[0][1] - t0, "arrivals_ms": [round((t - t0) * 1e3, 2) for _, t in ch],
                         "max_abs_diff": float(np.abs(pcm - ref).max()) if pcm.size == ref.size else None})
        best = sorted(runs, key=lambda x: x["total_s"])[len(runs) // 2]
        single[f"chunk_frames_{cf}"] = {
            "first_chunk_ms": round(float(np.median([x["first_s"] for x in runs])) * 1e3, 2),
            "total_s": round(float(np.median([x["total_s"] for x in runs])), 4),
            "total_vs_generate": round(float(np.median([x["total_s"] for x in runs])) / single["generate_s"], 4),
            "chunks": len(best["arrivals_ms"]), "arrivals_ms_median_run": best["arrivals_ms"],
            "max_abs_diff_vs_generate": max(x["max_abs_diff"] for x in runs)}
    out["single_utterance"] = single

    # lock-step batch
    r.generate_batch(texts)
    r.generate_batch_chunked(texts, chunk_frames=32)
    ref_b = r.generate_batch(texts)
    n_samples = sum(a.size for a in ref_b)
    t_b = []
    for _ in range(args.reps):
        t0 = time.monotonic()
        r.generate_batch_sizes(texts)
        t_b.append(time.monotonic() - t0)
    batch = {"utterances": args.batch, "generate_batch_audio_s_per_s": round(n_samples / SR / float(np.median(t_b)), 2)}
    for cf in (32, 64):
        ts, first = [], []
        for _ in range(args.reps):
            t0 = time.monotonic()
            ch = r.generate_batch_chunked(texts, chunk_frames=cf)
            ts.append(time.monotonic() - t0)
            first.append(ch[0][2] - t0)
        assert sum(a.size for _, a, _ in ch) == n_samples
        v = n_samples / SR / float(np.median(ts))
        batch[f"chunk_frames_{cf}"] = {"audio_s_per_s": round(v, 2), "fraction_of_generate_batch": round(v / batch["generate_batch_audio_s_per_s"], 4),
                                        "first_chunk_ms": round(float(np.median(first)) * 1e3, 2)}
    out["batch"] = batch
    r.close()
    os.remove(path)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
