"""Parler-Mini shapes, fp16 weights and KV cache, the DAC 44 kHz codec on the same context: the continuous session with chunked audio,
restating parler_runner::stream_step's loop on the engine — admit, tts_hip_parler_stream_launch (32), the window pass of the rows the previous
wait brought (tts_hip_dac_decode_windows, the windows of all slots in one pass) while the steps run, tts_hip_parler_stream_wait taking rows.
The codes of the windows are random (the pass costs what it costs whatever they are); window sizes follow parler_runner::chunker::plan: per
slot the whole chunks whose right halo is final, with both halos.

  (a) session step     tts_hip_parler_stream_run without a hook, 1023 slots live (a forward of 1024 rows), greedy, WARM steps then STEPS timed.  A
                       build of the parent commit measures it with this script too; --only-a appends one JSON line per process to --out, for
                       alternating processes of the two builds (the bar: the parent's own spread over its processes)
  (b) first chunk      62 slots live and chunking, a 63rd utterance admitted: wall time from before its admission to the end of the window pass
                       that holds its first chunk, chunk_frames 8 and 32; beside it, on either build, the time at which the unchunked session
                       delivers that utterance's audio: admission, its MAX_STEPS steps, collect, its whole-utterance decode
  (c) ragged mix       126 utterances of 64 ... 304 steps through 63 slots in audio-s/s: the chunked session per chunk_frames, every codec pass
                       included, against the unchunked session with the codec passes of parler_runner (finished utterances in groups, at most one
                       look-in late)

A build without tts_hip_parler_stream_launch runs the unchunked legs only and writes parler_stream_chunked_parent_before.json.
Usage: python profiles/parler_stream_chunked_bench.py [--out FILE] [--reps N] [--mix-reps N] [--only-a]"""
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

LOOK_IN, WARM, STEPS, PROMPT = 32, 32, 64, 16
BIG = 1023               # slots of (a)
SLOTS = 63               # slots of (b) and (c): every forward is one of 64 rows
MAX_STEPS = 256          # steps of the utterances of (b)
KV = 320                 # cached positions of (b) and (c): an utterance ends at position KV
N_RAGGED = 126
CHUNKS = (8, 32)
CHUNKED = hasattr(hip.HipEngine, "stream_launch")


def med(xs):
    return float(np.median(xs))


def step_time(model, cfg, reps):
    eng = hip.HipEngine(cfg, max_seqs=BIG + 1, kv_type=gguf.F16, kv_positions=128, flags=hip.FLAG_NO_DAC)
    eng.load(model)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(3, cfg.prompt_vocab, PROMPT).astype(np.uint32) for _ in range(BIG)]
    runs = []
    for _ in range(reps):
        eng.stream_begin(BIG, WARM + STEPS + 2, sampling=None)
        eng.stream_admit(list(range(BIG)), prompts)
        assert eng.stream_run(WARM) == []
        t = time.perf_counter()
        fin = eng.stream_run(STEPS)
        runs.append((time.perf_counter() - t) / STEPS * 1e3)
        assert fin == []
        eng.stream_end()
    eng.close()
    return {"slots": BIG, "session_stream_run_ms_per_step": round(med(runs), 4), "session_runs_ms": [round(x, 4) for x in runs],
            "min_ms": round(min(runs), 4), "max_ms": round(max(runs), 4)}


class Windows:
    """chunker::plan on frame counts: per slot the first frame not handed out"""

    def __init__(self, cfg, halo, cf, rng):
        self.nh, self.h, self.cf = cfg.n_out, halo, cf
        self.codes = rng.integers(0, cfg.cb_size, (4096, cfg.n_out)).astype(np.uint32)
        self.next = {}

    def admit(self, slot):
        self.next[slot] = 0

    def cut(self, steps, ended):
        """steps / ended per slot -> the windows [(slot, codes, keep0, keep1)] of this look-in"""
        out = []
        for s in sorted(self.next):
            have = max(int(steps[s]) - self.nh + 1, 0)   # frame i takes head k's token from step i + k
            nx = self.next[s]
            if ended[s]:
                f1 = have
            else:
                f1 = nx + (have - self.h - nx) // self.cf * self.cf if have >= nx + self.h + self.cf else nx
            if f1 <= nx:
                continue
            w0, w1 = max(nx - self.h, 0), min(have, f1 + self.h)
            out.append((s, self.codes[:w1 - w0], nx - w0, f1 - w0))
            self.next[s] = f1
        for s in [s for s in self.next if ended[s]]:
            del self.next[s]
        return out


def window_pass(eng, wins):
    if wins:
        eng.dac_decode_windows([w[1:] for w in wins])
    return sum(w[3] - w[2] for w in wins)


def first_chunk(eng, cfg, halo, prompts, cf, reps, rng):
    """(b): slots 0..61 live and chunking, slot 62 admitted; until the window pass that holds slot 62's first chunk has ended"""
    ts, launches = [], 0
    for _ in range(reps + 1):                # the first repetition warms the window shapes and is dropped
        eng.stream_begin(SLOTS, KV, sampling=None)
        eng.stream_admit(list(range(SLOTS - 1)), prompts[:SLOTS - 1])
        W = Windows(cfg, halo, cf, rng)
        for s in range(SLOTS - 1):
            W.admit(s)
        eng.stream_launch(LOOK_IN)
        _, cnt, done, _ = eng.stream_wait()
        pending = W.cut(cnt, done)
        t = time.perf_counter()
        eng.stream_admit([SLOTS - 1], prompts[SLOTS - 1:SLOTS])
        W.admit(SLOTS - 1)
        launches = 0
        while True:
            eng.stream_launch(LOOK_IN)
            launches += 1
            window_pass(eng, pending)
            if any(w[0] == SLOTS - 1 for w in pending):
                ts.append((time.perf_counter() - t) * 1e3)
                eng.stream_wait()
                break
            _, cnt, done, _ = eng.stream_wait()
            pending = W.cut(cnt, done)
        eng.stream_end()
    ts = ts[1:]
    return {"first_chunk_ms": round(med(ts), 3), "runs_ms": [round(x, 3) for x in ts], "launches_before_its_pass": launches}


def unchunked_delivery(eng, cfg, prompts, reps, rng):
    """(b), the unchunked session: the same utterance beside the same 62, until its whole-utterance decode has ended"""
    codes = rng.integers(0, cfg.cb_size, (KV, cfg.n_out)).astype(np.uint32)
    ts, steps = [], 0
    for _ in range(reps + 1):
        eng.stream_begin(SLOTS, KV, sampling=None)
        eng.stream_admit(list(range(SLOTS - 1)), prompts[:SLOTS - 1])
        eng.stream_run(LOOK_IN)
        t = time.perf_counter()
        eng.stream_admit([SLOTS - 1], prompts[SLOTS - 1:SLOTS])
        while True:
            fin = dict(eng.stream_run(LOOK_IN))
            if SLOTS - 1 in fin:
                steps = fin[SLOTS - 1]
                eng.stream_collect(SLOTS - 1, steps)
                eng.dac_decode(codes[:steps - cfg.n_out + 1])
                ts.append((time.perf_counter() - t) * 1e3)
                break
        eng.stream_end()
    ts = ts[1:]
    return {"utterance_steps": steps, "audio_after_ms": round(med(ts), 1), "runs_ms": [round(x, 1) for x in ts]}


def ragged(cfg, rng):
    lens = [int(x) for x in np.linspace(KV - 304, KV - 64, N_RAGGED).round()]
    order = np.random.default_rng(5).permutation(N_RAGGED)
    return [rng.integers(3, cfg.prompt_vocab, lens[i]).astype(np.uint32) for i in order]


def mix_unchunked(eng, cfg, prompts, reps, rng):
    codes = rng.integers(0, cfg.cb_size, (KV, cfg.n_out)).astype(np.uint32)
    ts, frames = [], 0
    for _ in range(reps):
        t = time.perf_counter()
        eng.stream_begin(SLOTS, KV, sampling=None)
        free, live, nxt, frames = list(range(SLOTS)), 0, 0, 0
        while nxt < len(prompts) or live:
            take = min(len(free), len(prompts) - nxt)
            if take:
                sl = [free.pop(0) for _ in range(take)]
                eng.stream_admit(sl, prompts[nxt:nxt + take])
                nxt += take
                live += take
            group = []
            for s, c in eng.stream_run(LOOK_IN):
                eng.stream_collect(s, c)
                group.append(codes[:c - cfg.n_out + 1])
                free.append(s)
                live -= 1
            if group:                        # the finished utterances of this look-in: one codec pass
                eng.dac_decode_batch(group)
                frames += sum(len(g) for g in group)
        eng.stream_end()
        ts.append(time.perf_counter() - t)
    audio = frames * cfg.hop / 44100.0
    return {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "audio_seconds": round(audio, 2), "audio_s_per_s": round(audio / med(ts), 1),
            "codec": "one pass per look-in over the utterances that finished in it"}


def mix_chunked(eng, cfg, halo, prompts, cf, reps, rng):
    ts, passes, frames = [], 0, 0
    for _ in range(reps):
        t = time.perf_counter()
        eng.stream_begin(SLOTS, KV, sampling=None)
        W = Windows(cfg, halo, cf, rng)
        free, live, nxt, pending, passes, frames = list(range(SLOTS)), 0, 0, [], 0, 0
        closing = []
        while nxt < len(prompts) or live or pending:
            take = min(len(free), len(prompts) - nxt)
            if take:
                sl = [free.pop(0) for _ in range(take)]
                eng.stream_admit(sl, prompts[nxt:nxt + take])
                for s in sl:
                    W.admit(s)
                nxt += take
                live += take
            if live:
                eng.stream_launch(LOOK_IN)
            frames += window_pass(eng, pending)
            passes += bool(pending)
            free += closing                  # a slot is free once its occupant's last piece is out
            closing, pending = [], []
            if live:
                _, cnt, done, fin = eng.stream_wait()
                pending = W.cut(cnt, done)
                for s, c in fin:
                    closing.append(s)
                    live -= 1
        eng.stream_end()
        ts.append(time.perf_counter() - t)
    audio = frames * cfg.hop / 44100.0
    return {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "audio_seconds": round(audio, 2), "audio_s_per_s": round(audio / med(ts), 1),
            "codec_passes": passes, "codec": "every pass included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mix-reps", type=int, default=2)
    ap.add_argument("--only-a", action="store_true", help="leg (a) alone, for alternating processes of two builds: printed, and appended as one JSON line to --out when given")
    args = ap.parse_args()
    out_path = args.out or os.path.join(HERE, "parler_stream_chunked.json" if CHUNKED else "parler_stream_chunked_parent_before.json")
    cfg = synth.parler_mini(weight_type=gguf.F16, max_gen=KV)
    model = synth.build(cfg)
    out = {"setup": {"model": "synthetic Parler-Mini (24 x 1024, 16 heads, ffn 4096, 9 x 1088 logits), fp16 weights, fp16 KV cache; DAC 44 kHz codec on the same context",
                     "look_in_steps": LOOK_IN, "prompt_ids": PROMPT, "reps": args.reps, "mix_reps": args.mix_reps, "sampler": "sampler::max",
                     "timing": "host wall clock, medians", "chunked_session": CHUNKED}}
    out["a_session_step"] = step_time(model, cfg, args.reps)
    print("a", json.dumps(out["a_session_step"]), flush=True)
    if args.only_a:
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps({"build_with_chunked_session": CHUNKED, "a_session_step": out["a_session_step"]}) + "\n")
        return
    rng = np.random.default_rng(11)
    eng = hip.HipEngine(cfg, max_seqs=SLOTS + 1, kv_type=gguf.F16, kv_positions=KV)
    eng.load(model)
    halo = eng.dac_halo_frames()
    out["setup"]["halo_frames"] = halo
    prompts = [rng.integers(3, cfg.prompt_vocab, KV - MAX_STEPS).astype(np.uint32) for _ in range(SLOTS)]
    out["b_first_chunk"] = {"slots": SLOTS, "unchunked_session": unchunked_delivery(eng, cfg, prompts, args.reps, rng)}
    print("b unchunked", json.dumps(out["b_first_chunk"]["unchunked_session"]), flush=True)
    if CHUNKED:
        for cf in CHUNKS:
            leg = first_chunk(eng, cfg, halo, prompts, cf, args.reps, rng)
            out["b_first_chunk"][str(cf)] = leg
            print("b", cf, json.dumps(leg), flush=True)
    rp = ragged(cfg, rng)
    out["c_ragged_mix"] = {"slots": SLOTS, "utterances": N_RAGGED, "unchunked_session": mix_unchunked(eng, cfg, rp, args.mix_reps, rng)}
    print("c", json.dumps(out["c_ragged_mix"]["unchunked_session"]), flush=True)
    if CHUNKED:
        base = out["c_ragged_mix"]["unchunked_session"]["audio_s_per_s"]
        for cf in CHUNKS:
            leg = mix_chunked(eng, cfg, halo, rp, cf, args.mix_reps, rng)
            leg["of_unchunked_audio_s_per_s"] = round(leg["audio_s_per_s"] / base, 4)
            out["c_ragged_mix"]["chunked_%d" % cf] = leg
            print("c", cf, json.dumps(leg), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
