"""Dia-1.6B shapes (the model of dia_stream_bench.py: fp16 matrices, 4 utterance slots) and the F32 codec of synth.dia_1_6b on a context of its
own: the continuous session with chunked audio, restating dia_runner::stream_step's loop on the two engines — admit, tts_hip_dia_stream_launch
(16), the window pass of the rows the previous wait brought (tts_hip_dac_decode_windows on the codec context) while the steps run,
tts_hip_dia_stream_wait taking rows.  The codes of the windows are random (the pass costs what it costs whatever they are); window sizes follow
the runner's plan: per slot the whole chunks whose right halo is final, with a left halo.

  (a) step cost with nobody chunking   tts_hip_dia_stream_run, 4 slots live, positions 16 .. 144, `reps` runs: the same leg as (a) of
                                       dia_stream_bench.py, so a build of the parent commit measures it with this script too
  (b) first chunk                      three slots live, a fourth utterance admitted: wall time from before its admission to the end of the
                                       window pass that holds its first chunk, chunk_frames 16 / 32 / 64, against the floor
                                       admission + 16 * ceil((chunk_frames + halo + max_delay) / 16) session steps + one window pass
                                       built from the parent's figures when --parent FILE gives them (else this process')
  (c) ragged mix                       the 12 utterances of dia_stream_bench.py through the chunked session per chunk_frames, against the
                                       unchunked session (stream_run / stream_collect, codec excluded as there) in the same process

A build without tts_hip_dia_stream_launch runs the unchunked legs only and writes dia_stream_chunked_parent_before.json.
Usage: python profiles/dia_stream_chunked_bench.py [--out FILE] [--reps N] [--mix-reps N] [--parent FILE]"""
import argparse
import dataclasses
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

CHUNKS = (16, 32, 64)


def step_time(eng, a, toks, reps):
    sess = []
    for _ in range(reps + 1):               # the first repetition captures the graph and is dropped
        eng.stream_begin(SLOTS, eng.cfg.max_gen, **a)
        eng.stream_admit(list(range(SLOTS)), [toks] * SLOTS, [TEXT_LEN] * SLOTS)
        assert eng.stream_run(WARM) == []
        t = time.perf_counter()
        fin = eng.stream_run(STEPS)
        sess.append((time.perf_counter() - t) / STEPS * 1e3)
        assert fin == []
        eng.stream_end()
    sess = sess[1:]
    return {"session_stream_run_ms_per_step": round(med(sess), 4), "session_runs_ms": [round(x, 4) for x in sess], "min_ms": round(min(sess), 4),
            "max_ms": round(max(sess), 4)}


def admission(eng, a, toks, reps):
    ts = []
    for _ in range(reps + 1):
        eng.stream_begin(SLOTS, eng.cfg.max_gen, **a)
        eng.stream_admit([0, 1, 2], [toks] * 3, [TEXT_LEN] * 3)
        assert eng.stream_run(LOOK_IN) == []
        t = time.perf_counter()
        eng.stream_admit([3], [toks], [TEXT_LEN])
        ts.append((time.perf_counter() - t) * 1e3)
        eng.stream_end()
    return {"admit_one_ms": round(med(ts[1:]), 3), "runs_ms": [round(x, 3) for x in ts[1:]]}


class Chunker:
    """dia_runner::chunker on step counts: every frame is kept (the model draws no special id), so after `steps` steps steps - max_delay frames
    are final"""

    def __init__(self, cf, halo, max_delay, dcfg, rng):
        self.cf, self.h, self.d, self.dcfg, self.rng = cf, halo, max_delay, dcfg, rng
        self.emitted = {}

    def reset(self, slot):
        self.emitted[slot] = 0

    def plan(self, slot, steps, finished):
        have, e = max(0, steps - self.d), self.emitted[slot]
        end = have if finished else (e + (have - self.h - e) // self.cf * self.cf if have >= e + self.h + self.cf else e)
        if end == e:
            return None
        w0, w1 = max(0, e - self.h), min(end + self.h, have)
        self.emitted[slot] = end
        return (self.rng.integers(0, self.dcfg.cb_size, (w1 - w0, self.dcfg.n_out)).astype(np.uint32), e - w0, end - w0)


def chunked_session(eng, dac, a, texts, budgets, cf, halo, dcfg, rng, first_of=None):
    """-> (per-utterance step counts, wall time of the first window pass that holds a chunk of utterance `first_of`, frames decoded)"""
    cfg = eng.cfg
    eng.stream_begin(SLOTS, cfg.max_gen, **a)
    ch = Chunker(cf, halo, cfg.max_delay, dcfg, rng)
    free, slot_utt, lens, nxt, wins, win_utt, first, frames = list(range(SLOTS)), {}, [0] * len(texts), 0, [], [], None, 0
    while nxt < len(texts) or slot_utt or wins:
        take = []
        while nxt < len(texts) and free:
            take.append((free.pop(0), nxt))
            nxt += 1
        if take:
            eng.stream_admit([s for s, _ in take], [texts[u] for _, u in take], [TEXT_LEN] * len(take), budgets=[budgets[u] for _, u in take])
            slot_utt.update(take)
            for s, _ in take:
                ch.reset(s)
        eng.stream_launch(LOOK_IN)
        if wins:                                  # under the steps
            dac.dac_decode_windows(wins)
            frames += sum(k1 - k0 for _, k0, k1 in wins)
            if first is None and first_of in win_utt:
                first = time.perf_counter()
            wins, win_utt = [], []
        _, steps, done, fin = eng.stream_wait()
        ended = dict(fin)
        for s in sorted(slot_utt):
            w = ch.plan(s, int(steps[s]), s in ended)
            if w is not None:
                wins.append(w)
                win_utt.append(slot_utt[s])
        for s, n in fin:
            lens[slot_utt.pop(s)] = n
            free.append(s)
        if not slot_utt and nxt == len(texts) and wins:   # nothing to run the codec under
            dac.dac_decode_windows(wins)
            frames += sum(k1 - k0 for _, k0, k1 in wins)
            wins, win_utt = [], []
    eng.stream_end()
    return lens, first, frames


def plain_session(eng, a, texts, budgets):
    eng.stream_begin(SLOTS, eng.cfg.max_gen, **a)
    free, slot_utt, lens, nxt = list(range(SLOTS)), {}, [0] * len(texts), 0
    while nxt < len(texts) or slot_utt:
        take = []
        while nxt < len(texts) and free:
            take.append((free.pop(0), nxt))
            nxt += 1
        if take:
            eng.stream_admit([s for s, _ in take], [texts[u] for _, u in take], [TEXT_LEN] * len(take), budgets=[budgets[u] for _, u in take])
            slot_utt.update(take)
        for s, n in eng.stream_run(LOOK_IN):
            lens[slot_utt.pop(s)] = len(eng.stream_collect(s, n))
            free.append(s)
    eng.stream_end()
    return lens


def main():
    have = hasattr(hip.DiaEngine, "stream_launch")
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "dia_stream_chunked.json" if have else "dia_stream_chunked_parent_before.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mix-reps", type=int, default=3)
    ap.add_argument("--parent", default=None, help="dia_stream_chunked_parent_before.json of a build of the parent commit")
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
    budgets = [n + 1 for n in LENGTHS]
    frames = sum(n - cfg.max_delay for n in LENGTHS)
    out = {"setup": {"model": "synthetic Dia-1.6B shapes of dia_stream_bench.py, fp16, 4 slots = 8 rows; F32 codec of synth.dia_1_6b on its own context",
                     "text_bytes": TEXT_LEN, "warm_steps": WARM, "timed_steps": STEPS, "reps": args.reps, "mix_reps": args.mix_reps, "chunked": have,
                     "timing": "host wall clock around the blocking calls, median of the runs listed"}}

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    out["step_time"] = step_time(eng, a, texts[0], args.reps)
    print("step", json.dumps(out["step_time"]), flush=True)
    out["admission"] = admission(eng, a, texts[1], args.reps)
    ts = []
    for _ in range(args.mix_reps):
        t = time.perf_counter()
        assert plain_session(eng, a, texts, budgets) == LENGTHS
        ts.append(time.perf_counter() - t)
    out["ragged_unchunked_session"] = {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "audio_seconds_per_s": round(frames / FRAMES_PER_S / med(ts), 3)}
    print("ragged", json.dumps(out["ragged_unchunked_session"]), flush=True)
    save()
    if not have:
        eng.close()
        return
    parent = json.load(open(args.parent)) if args.parent else None
    if parent:
        p = parent["step_time"]
        v = out["step_time"]["session_stream_run_ms_per_step"]
        out["step_time_vs_parent"] = {"parent_ms": p["session_stream_run_ms_per_step"], "parent_range_ms": [p["min_ms"], p["max_ms"]], "this_ms": v,
                                      "ratio": round(v / p["session_stream_run_ms_per_step"], 4), "inside_parent_range": bool(p["min_ms"] <= v <= p["max_ms"])}
    base = parent or out
    step_ms, admit_ms = base["step_time"]["session_stream_run_ms_per_step"], base["admission"]["admit_one_ms"]
    dmodel = synth.build_dia(synth.dia_1_6b(weight_type=gguf.F16, enc_layers=1, dec_layers=1), suppress_special=True, pooled=True).dac   # the codec is what is needed
    dcfg = dataclasses.replace(dmodel.cfg, max_gen=4096)   # the codec context's frame capacity; the tensors do not depend on it
    dac = hip.HipEngine(dcfg, flags=hip.FLAG_NO_PARLER)
    dac.load(dmodel)
    halo = dac.dac_halo_frames()
    out["setup"]["halo_frames"] = halo
    # (b) three slots far into long utterances, a fourth admitted beside them
    out["first_chunk"] = {}
    for cf in CHUNKS:
        win = [(rng.integers(0, dcfg.cb_size, (cf + halo, dcfg.n_out)).astype(np.uint32), 0, cf)]
        dac.dac_decode_windows(win)
        wts = []
        for _ in range(max(3, args.reps)):
            t = time.perf_counter()
            dac.dac_decode_windows(win)
            wts.append((time.perf_counter() - t) * 1e3)
        need = -(-(cf + halo + cfg.max_delay) // LOOK_IN) * LOOK_IN
        floor = admit_ms + need * step_ms + med(wts)
        runs = []
        for _ in range(args.reps + 1):
            # utterances 0..2 fill three slots and outlast the fourth's first chunk; only the fourth is timed: its admission is the session's second
            eng.stream_begin(SLOTS, cfg.max_gen, **a)
            ch = Chunker(cf, halo, cfg.max_delay, dcfg, rng)
            eng.stream_admit([0, 1, 2], texts[:3], [TEXT_LEN] * 3, budgets=[1000] * 3)
            eng.stream_launch(LOOK_IN)
            eng.stream_wait()
            t0 = time.perf_counter()
            eng.stream_admit([3], [texts[3]], [TEXT_LEN], budgets=[need + 64])
            ch.reset(3)
            w, t1 = None, None
            while t1 is None:
                eng.stream_launch(LOOK_IN)
                if w is not None:
                    dac.dac_decode_windows([w])
                    t1 = time.perf_counter()
                _, steps, _, _ = eng.stream_wait()
                w = ch.plan(3, int(steps[3]), False)
            eng.stream_end()
            runs.append((t1 - t0) * 1e3)
        runs = runs[1:]
        out["first_chunk"][f"chunk_frames_{cf}"] = {"first_chunk_ms": round(med(runs), 2), "runs_ms": [round(x, 2) for x in runs], "steps_needed": need,
                                                    "window_pass_ms": round(med(wts), 3), "floor_ms": round(floor, 2), "floor_from": "parent" if parent else "this process",
                                                    "first_vs_floor": round(med(runs) / floor, 3),
                                                    "unchunked_session_ms_for_a_3072_step_utterance": round(admit_ms + 3072 * step_ms, 1)}
        print("first", cf, json.dumps(out["first_chunk"][f"chunk_frames_{cf}"]), flush=True)
        save()
    # (c) the ragged mix, chunked
    ref = (parent or out)["ragged_unchunked_session"]
    out["ragged_chunked_session"] = {"against": "parent" if parent else "this process", "unchunked_seconds": ref["seconds"]}
    for cf in CHUNKS:
        ts, fr = [], 0
        for _ in range(args.mix_reps):
            t = time.perf_counter()
            lens, _, fr = chunked_session(eng, dac, a, texts, budgets, cf, halo, dcfg, rng)
            ts.append(time.perf_counter() - t)
            assert lens == LENGTHS and fr == frames, (lens, fr)
        out["ragged_chunked_session"][f"chunk_frames_{cf}"] = {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts],
                                                               "audio_seconds_per_s": round(frames / FRAMES_PER_S / med(ts), 3),
                                                               "audio_s_per_s_over_unchunked": round(ref["seconds"] / med(ts), 4)}
        print("ragged", cf, json.dumps(out["ragged_chunked_session"][f"chunk_frames_{cf}"]), flush=True)
        save()
    dac.close()
    eng.close()


if __name__ == "__main__":
    main()
