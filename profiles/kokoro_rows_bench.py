#!/usr/bin/env python3
"""Kokoro duration pass for several clauses in one context (tts_hip_kokoro_durations_batch, TTS_KOKORO_ROWS) at the Kokoro-82M widths, synthetic
weights with forced_frames = 3 (shape determinism).  One process; every figure is the median of 5 timed repeats after one warm-up, all repeats kept.

  durations        8 clauses of 66 / 402 rows: 8 tts_hip_kokoro_durations calls in a row against one tts_hip_kokoro_durations_batch of B = 2, 4, 8
                   (the sequential figure for B clauses is the time of the first B calls)
  generate_batch   the runner on 16 utterances of 400 ids at 1 / 2 / 4 / 8 lanes with TTS_KOKORO_ROWS = 0 and 8

On a tree without the batch call (the parent commit) only the rows-off legs run, which is how profiles/kokoro_rows_parent_before.json was made:
  python profiles/kokoro_rows_bench.py --out profiles/kokoro_rows.json"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tts_cpp_amd  # noqa: E402,F401
from tts_cpp_amd import hip, runner, synth  # noqa: E402

REPEATS = 5


def timed(fn):
    fn()                                                   # warm-up
    ms = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats_ms": [round(v, 3) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lanes", default="1,2,4,8")
    args = ap.parse_args()
    model = synth.build_kokoro(synth.kokoro_82m(forced_frames=3))
    cfg = model.cfg
    voice = cfg.voices[0]
    rng = np.random.default_rng(1)
    eng = hip.KokoroEngine(model)
    has_batch = hasattr(eng, "durations_batch")
    out = {"widths": "kokoro_82m(forced_frames=3)", "repeats": REPEATS, "has_durations_batch": has_batch, "durations": {}, "generate_batch": {}}
    for rows in (66, 402):
        toks = [np.concatenate([[0], rng.integers(1, cfg.vocab, rows - 2), [0]]).astype(np.uint32) for _ in range(8)]
        leg = {}
        for B in (1, 2, 4, 8):
            leg[f"sequential_{B}"] = timed(lambda: [eng.durations(t, voice) for t in toks[:B]])
            if has_batch:
                leg[f"batch_{B}"] = timed(lambda: eng.durations_batch(toks[:B], [voice] * B))
        out["durations"][str(rows)] = leg
        print(rows, "rows:", {k: v["median_ms"] for k, v in leg.items()}, flush=True)
    eng.close()
    os.environ["TTS_KOKORO_INPUT_IS_PHONEMES"] = "1"
    texts = ["".join(chr(0x61 + int(v)) for v in rng.integers(0, 26, 398)) for _ in range(16)]
    with tempfile.TemporaryDirectory() as td:
        gpath = model.write_gguf(os.path.join(td, "kokoro82m.gguf"))
        first = None
        for lanes in (int(x) for x in args.lanes.split(",") if x):
            for rows_on in ((0, 8) if has_batch else (0,)):
                os.environ["TTS_KOKORO_ROWS"] = str(rows_on)    # read when the runner is constructed
                r = runner.Runner(gpath, voice=voice.encode(), max_seqs=lanes, share_with=first)
                first = first or r
                sizes = []
                leg = timed(lambda: sizes.append(r.generate_batch_sizes(texts, voice=voice.encode())))
                audio_s = sum(sizes[-1]) / 24000.0
                leg["audio_seconds_per_sec"] = round(audio_s / (leg["median_ms"] * 1e-3), 1)
                leg["audio_seconds_per_sec_repeats"] = [round(audio_s / (v * 1e-3), 1) for v in leg["repeats_ms"]]
                out["generate_batch"][f"lanes_{lanes}_rows_{rows_on}"] = leg
                print(f"generate_batch lanes {lanes} rows {rows_on}: {leg['audio_seconds_per_sec']} audio-s/s ({leg['audio_seconds_per_sec_repeats']})", flush=True)
                if r is not first:
                    r.close()
        first.close()
    txt = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
