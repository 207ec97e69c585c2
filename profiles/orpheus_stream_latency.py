"""Chunked Orpheus audio latency at the real shapes: Orpheus-3B Q4_0 (synthetic blocks, as bench.py --workload orpheus) and SNAC 24 kHz.
The 3B model is not written to a GGUF here, so the script drives the two engines with the runner's look-in loop (orpheus_runner::chunk_run:
launch the next piece of steps, decode the windows the previous look-in made ready, look at the ids); random codes of the right layout stand
in for the ids' payload, timing does not depend on their values.  One sequence and a lock-step batch of 8, chunk_frames 1 / 4 / 16: time to
the first chunk, total time, and the one-call loop + whole-utterance decode ("generate") on the same engines.  Writes one JSON.

--whole-only measures the one-call part alone and uses nothing a commit without chunked Orpheus audio lacks: run it (and
`bench.py --workload orpheus`) in a checkout of the parent commit, then hand both files to the full run with --parent / --parent-bench; the
full run reports its own generate median against the parent's min - max spread and the chunked totals against the parent's generate.

    python profiles/orpheus_stream_latency.py [--out profiles/orpheus_stream_latency.json] [--frames 44] [--reps 5]
                                              [--whole-only] [--parent parent.json] [--parent-bench parent_bench.json] [--bench this_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import tts_cpp_amd  # noqa: E402,F401
from tts_cpp_amd import gguf, hip, synth  # noqa: E402

from secondary_bench import _Model, orpheus_tensors  # noqa: E402

NO_STOP = 0xFFFFFFFF


def codes_of(levels, f0, f1):
    return np.concatenate([l[f0 * (4 // r):f1 * (4 // r)] for l, r in zip(levels, (4, 2, 1))])


def chunked(eng, snac, prompts, levels, n_ids, cf, h, lockstep):
    """the runner's loop; -> (first chunk s, total s, chunks)"""
    n = len(prompts)
    piece = 7 * min(cf, 8)
    t0 = time.monotonic()
    eng.gen_begin(prompts, n_ids, NO_STOP)
    ids, done = eng.gen_wait()
    nxt = [0] * n
    first, chunks = None, 0
    while True:
        ws = []
        for u in range(n):
            F = ids[u].size // 7
            f1 = F if done[u] else nxt[u] + max(0, F - h - nxt[u]) // cf * cf
            if f1 > nxt[u]:
                w0, w1 = max(0, nxt[u] - h), min(F, f1 + h)
                ws.append((codes_of(levels[u], w0, w1), w1 - w0, nxt[u] - w0, f1 - w0, None))
                chunks += -(-(f1 - nxt[u]) // cf)
                nxt[u] = f1
        if done.all() and not ws:
            break
        if not lockstep and not done.all():
            eng.gen_launch(piece)
        if ws:
            snac.decode_windows(ws, split=True)
            if first is None:
                first = time.monotonic() - t0
        if lockstep and not done.all():
            eng.gen_launch(piece)
        if not done.all():
            ids, done = eng.gen_wait()
    return first, time.monotonic() - t0, chunks


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orpheus_stream_latency.json"))
    ap.add_argument("--frames", type=int, default=44)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--parent-bench", default=None)
    ap.add_argument("--bench", default=None)
    args = ap.parse_args()
    parent = json.load(open(args.parent)) if args.parent else None
    n_ids, K = 7 * args.frames, args.frames
    cfg = synth.orpheus_3b(ctx=1024, weight_type=gguf.Q4_0)
    rng = np.random.default_rng(7)
    tensors, _ = orpheus_tensors(cfg, rng)
    model = _Model(cfg, tensors)
    scfg = synth.snac_24khz(max_frames=4 * K)
    snac = hip.SnacEngine(scfg)
    snac.load(synth.build_snac(scfg))
    h = None if args.whole_only else snac.halo_frames()
    out = {"setup": {"decoder": "Orpheus-3B shapes, Q4_0 (synthetic blocks)", "codec": "SNAC 24 kHz shapes, F32", "prompt_ids": 32, "ids": n_ids, "frames": K,
                     "halo_frames": h, "look_in_steps": "7 * min(chunk_frames, 8)", "reps": args.reps,
                     "note": "engine-level restatement of orpheus_runner::chunk_run (gen_begin / gen_launch / gen_wait + decode_windows_begin / _end): one sequence "
                             "launches, decodes the ready windows under the running steps, then waits; a lock-step batch decodes and hands out the ready windows "
                             "before its blocking launch",
                     "first_chunk_floor": "prefill + (7 * (chunk_frames + halo) - 1) steps at the mean ms/step of the whole generation + one window pass; the early steps "
                                          "attend to fewer positions than the mean one, so a first chunk can come in slightly under it"}}
    for name, B in (("single_sequence", 1), (f"lockstep_batch_{args.batch}", args.batch)):
        eng = hip.OrpheusEngine(cfg, max_seqs=B)
        eng.load(model)
        prompts = [rng.integers(0, cfg.vocab, 32).astype(np.uint32) for _ in range(B)]
        levels = [[rng.integers(0, scfg.cb_size, 4 * K // r).astype(np.uint32) for r in scfg.repeats] for _ in range(B)]

        def whole():
            t0 = time.monotonic()
            if B == 1:
                eng.generate_greedy(prompts[0], n_ids, NO_STOP)
            else:
                eng.generate_batch(prompts, n_ids, NO_STOP)
            t1 = time.monotonic()
            for u in range(B):
                snac.decode(codes_of(levels[u], 0, K), 4 * K, None)
            return t1 - t0, time.monotonic() - t1

        whole()
        runs = [whole() for _ in range(args.reps)]
        tot = [a + b for a, b in runs]
        res = {"generate_s": {"median": round(med(tot), 5), "min": round(min(tot), 5), "max": round(max(tot), 5), "runs": [round(t, 5) for t in tot],
                              "decoder_s": round(med([a for a, _ in runs]), 5), "snac_whole_s": round(med([b for _, b in runs]), 5)}}
        out[name] = res
        if args.whole_only:
            eng.close()
            continue
        ref = med(tot)   # what the chunked totals are compared with: the parent's generate when its file is given
        if parent:
            pg = parent[name]["generate_s"]
            ref = pg["median"]
            res["generate_parent_s"] = pg
            res["generate_median_inside_parent_spread"] = bool(pg["min"] <= med(tot) <= pg["max"])
            res["generate_median_vs_parent_spread"] = "below its minimum (faster)" if med(tot) < pg["min"] else "above its maximum (slower)" if med(tot) > pg["max"] else "inside"
            res["generate_vs_parent"] = round(med(tot) / pg["median"], 4)

        def timed(fn):
            ts = []
            for _ in range(args.reps + 1):
                t0 = time.monotonic()
                fn()
                ts.append(time.monotonic() - t0)
            return med(ts[1:])

        def begin():
            eng.gen_begin(prompts, n_ids, NO_STOP)
            eng.gen_wait()

        prefill = timed(begin)
        win = timed(lambda: snac.decode_windows([(codes_of(levels[0], 0, 1 + 2 * h), 1 + 2 * h, h, h + 1, None)] * B, split=True))
        step = (med([a for a, _ in runs]) - prefill) / (n_ids - 1)
        res.update({"prefill_and_first_selection_ms": round(prefill * 1e3, 2), "ms_per_step": round(step * 1e3, 4), "one_window_pass_ms": round(win * 1e3, 3)})
        for cf in (1, 4, 16):
            chunked(eng, snac, prompts, levels, n_ids, cf, h, B > 1)
            rs = [chunked(eng, snac, prompts, levels, n_ids, cf, h, B > 1) for _ in range(args.reps)]
            floor = prefill + (7 * (cf + h) - 1) * step + win   # the ids of frames [0, cf + h) after the first, then one window pass
            tt = med([r[1] for r in rs])
            res[f"chunk_frames_{cf}"] = {"first_chunk_ms": round(med([r[0] for r in rs]) * 1e3, 2), "first_chunk_floor_ms": round(floor * 1e3, 2),
                                         "total_s": round(tt, 4), "total_vs_generate": round(tt / ref, 4),
                                         "total_minus_generate_in_window_passes": round((tt - ref) / win, 2), "chunks": rs[0][2]}
        res["total_vs_generate_is_against"] = "the parent commit's generate median" if parent else "this commit's generate median"
        eng.close()
    snac.close()
    keys = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "ms_per_decode_step", "snac_ms_per_64_frames")
    for label, path in (("bench_orpheus_this_commit", args.bench), ("bench_orpheus_parent_commit", args.parent_bench)):
        if path:
            b = json.loads(open(path).read().strip().split("\n")[-1])
            out[label] = {k: b[k] for k in keys if k in b}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
