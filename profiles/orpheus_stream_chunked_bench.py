"""Orpheus-3B Q4_0 shapes (the model of orpheus_stream_bench.py, 8 slots) and the SNAC 24 kHz codec of synth.snac_24khz on a context of its own:
the continuous session with chunked audio, restating orpheus_runner::stream_step's loop on the two engines — admit, tts_hip_orpheus_stream_launch
(28), the window pass of the ids the previous wait brought (tts_hip_snac_decode_windows_begin / _end on the codec context, the windows of all slots
in one pass) while the steps run, tts_hip_orpheus_stream_wait taking ids.  The codes of the windows are random (the pass costs what it costs
whatever they are) and so is their noise; window sizes follow chunk_collect: per slot the whole chunks whose halo is complete, with both halos.

  (a) session step           tts_hip_orpheus_stream_run, 8 slots live, 56 steps after 8, `reps` sessions: median, every run, min and max; a build
                             of the parent commit measures it with this script too
  (b) first chunk            seven slots live, an eighth utterance admitted: wall time from before its admission to the end of the window pass
                             that holds its first chunk, chunk_frames 1 / 4 / 16, against the floor
                             admission + 28 * ceil(7 * (chunk_frames + halo) / 28) session steps + one window pass
                             built from the parent's figures when --parent FILE gives them (else this process'); and the time at which an
                             unchunked session delivers that utterance: admission + (max_new - 1) steps + its whole-utterance SNAC decode
  (c) ragged mix             the 24 utterances of orpheus_stream_bench.py (10:1 lengths through the end of a 448-position cache) through the
                             chunked session per chunk_frames, every codec pass included, against the unchunked session (stream_run /
                             stream_collect, codec excluded as there) in the same process
  (d) codec overlap          how much of a 28-step run at 8 rows is still to run when stream_launch returns: the lock-step loop is enqueued by
                             the host launch by launch, so the host is free for the codec pass only for what is left

A build without tts_hip_orpheus_stream_launch runs the unchunked legs only and writes orpheus_stream_chunked_parent_before.json.
Usage: python profiles/orpheus_stream_chunked_bench.py [--out FILE] [--reps N] [--mix-reps N] [--parent FILE] [--only-a]"""
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
from orpheus_stream_bench import LOOK_IN, N_RAGGED, NO_STOP, RAGGED_CTX, RAGGED_LENGTHS, SLOTS, STEPS, WARM, med  # noqa: E402

CHUNKS = (1, 4, 16)
MAX_NEW = 2100          # orpheus_hparams::max_generation_size
PROMPT = 32


def step_time(eng, prompts, reps):
    runs = []
    for _ in range(reps):
        eng.stream_begin(SLOTS, WARM + STEPS + 2, NO_STOP)
        eng.stream_admit(list(range(SLOTS)), prompts)
        assert eng.stream_run(WARM) == []
        t = time.perf_counter()
        fin = eng.stream_run(STEPS)
        runs.append((time.perf_counter() - t) / STEPS * 1e3)
        assert fin == []
        eng.stream_end()
    return {"session_stream_run_ms_per_step": round(med(runs), 4), "session_runs_ms": [round(x, 4) for x in runs], "min_ms": round(min(runs), 4),
            "max_ms": round(max(runs), 4)}


def admission(eng, prompts, reps):
    ts = []
    for _ in range(reps):
        eng.stream_begin(SLOTS, MAX_NEW, NO_STOP)
        eng.stream_admit(list(range(SLOTS - 1)), prompts[:SLOTS - 1])
        assert eng.stream_run(LOOK_IN) == []
        t = time.perf_counter()
        eng.stream_admit([SLOTS - 1], prompts[SLOTS - 1:SLOTS])
        ts.append((time.perf_counter() - t) * 1e3)
        eng.stream_end()
    return {"admission_beside_7_ms": round(med(ts), 4), "runs_ms": [round(x, 4) for x in ts]}


class Windows:
    """chunk_collect on frame counts: per slot the frames it has, the first frame not handed out, and whether it ended"""

    def __init__(self, scfg, halo, cf, rng):
        self.scfg, self.h, self.cf = scfg, halo, cf
        self.ups = np.cumprod(scfg.strides)
        self.codes = rng.integers(0, scfg.cb_size, 7 * 4096).astype(np.uint32)
        self.noise = rng.standard_normal(int(4 * self.ups.sum()) * 64).astype(np.float32)
        self.next = {}

    def admit(self, slot):
        self.next[slot] = 0

    def cut(self, frames, ended):
        """frames / ended: per slot -> the windows [(slot, codes, frames, keep0, keep1, noise)] of this look-in"""
        out = []
        for s in sorted(self.next):
            F, nx = int(frames[s]), self.next[s]
            if ended[s]:
                f1 = F
            else:
                avail = max(F - self.h, 0)
                f1 = nx + (avail - nx) // self.cf * self.cf if avail > nx else nx
            if f1 <= nx:
                continue
            w0, w1 = max(nx - self.h, 0), min(F, f1 + self.h)
            n = w1 - w0
            out.append((s, self.codes[:7 * n], n, nx - w0, f1 - w0, self.noise[:int(4 * self.ups.sum()) * n]))
            self.next[s] = f1
        for s in [s for s in self.next if ended[s]]:
            del self.next[s]
        return out


def window_pass(snac, wins):
    if wins:
        snac.decode_windows([w[1:] for w in wins], split=True)


def first_chunk(eng, snac, scfg, halo, prompts, cf, reps, rng):
    """(b): slots 0..6 live and chunking, slot 7 admitted; until the window pass that holds slot 7's first chunk has ended"""
    ts, launches = [], 0
    for _ in range(reps + 1):                # the first repetition warms the window shapes and is dropped
        eng.stream_begin(SLOTS, MAX_NEW, NO_STOP)
        eng.stream_admit(list(range(SLOTS - 1)), prompts[:SLOTS - 1])
        W = Windows(scfg, halo, cf, rng)
        for s in range(SLOTS - 1):
            W.admit(s)
        eng.stream_launch(LOOK_IN)
        _, cnt, done, _ = eng.stream_wait()
        pending = W.cut(cnt // 7, done)
        t = time.perf_counter()
        eng.stream_admit([SLOTS - 1], prompts[SLOTS - 1:SLOTS])
        W.admit(SLOTS - 1)
        launches = 0
        while True:
            eng.stream_launch(LOOK_IN)
            launches += 1
            window_pass(snac, pending)
            if any(w[0] == SLOTS - 1 for w in pending):
                ts.append((time.perf_counter() - t) * 1e3)
                eng.stream_wait()
                break
            _, cnt, done, _ = eng.stream_wait()
            pending = W.cut(cnt // 7, done)
        eng.stream_end()
    ts = ts[1:]
    return {"first_chunk_ms": round(med(ts), 3), "runs_ms": [round(x, 3) for x in ts], "launches_before_its_pass": launches}


def one_pass(snac, scfg, halo, cf, reps, rng):
    """the window pass that holds a first chunk beside seven slots that hand out what 28 steps made: 4 frames each"""
    W = Windows(scfg, halo, cf, rng)
    wins = [(SLOTS - 1, W.codes[:7 * (cf + halo)], cf + halo, 0, cf, W.noise[:int(4 * W.ups.sum()) * (cf + halo)])]
    k = 4 // cf * cf
    if k:
        wins += [(s, W.codes[:7 * (k + 2 * halo)], k + 2 * halo, halo, halo + k, W.noise[:int(4 * W.ups.sum()) * (k + 2 * halo)]) for s in range(SLOTS - 1)]
    ts = []
    for _ in range(reps + 1):
        t = time.perf_counter()
        window_pass(snac, wins)
        ts.append((time.perf_counter() - t) * 1e3)
    return round(med(ts[1:]), 4)


def overlap(eng, prompts, reps):
    """(d): wall time of stream_launch(28) and of the wait that follows, 8 rows"""
    la, wa = [], []
    for _ in range(reps):
        eng.stream_begin(SLOTS, MAX_NEW, NO_STOP)
        eng.stream_admit(list(range(SLOTS)), prompts)
        assert eng.stream_run(WARM) == []
        t0 = time.perf_counter()
        eng.stream_launch(LOOK_IN)
        t1 = time.perf_counter()
        eng.stream_wait()
        t2 = time.perf_counter()
        la.append((t1 - t0) * 1e3)
        wa.append((t2 - t1) * 1e3)
        eng.stream_end()
    return {"launch_returns_after_ms": round(med(la), 3), "wait_after_it_ms": round(med(wa), 3), "share_still_running_when_launch_returns": round(med(wa) / (med(la) + med(wa)), 4),
            "launch_runs_ms": [round(x, 3) for x in la], "wait_runs_ms": [round(x, 3) for x in wa]}


def mix_unchunked(eng, prompts, reps):
    ts, lens = [], None
    for _ in range(reps):
        t = time.perf_counter()
        eng.stream_begin(SLOTS, 512, NO_STOP)
        free, slot_utt, out, nxt = list(range(SLOTS)), {}, [None] * N_RAGGED, 0
        while nxt < N_RAGGED or slot_utt:
            while nxt < N_RAGGED and free:
                s = free.pop(0)
                eng.stream_admit([s], [prompts[nxt]])
                slot_utt[s] = nxt
                nxt += 1
            for s, c in eng.stream_run(LOOK_IN):
                out[slot_utt.pop(s)] = eng.stream_collect(s, c)
                free.append(s)
        eng.stream_end()
        ts.append(time.perf_counter() - t)
        lens = [len(o) for o in out]
    assert lens == RAGGED_LENGTHS
    return {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "tokens_per_s": round(sum(lens) / med(ts), 1), "codec": "excluded"}


def mix_chunked(eng, snac, scfg, halo, prompts, cf, reps, rng):
    ts, passes, lens = [], 0, None
    for _ in range(reps):
        t = time.perf_counter()
        eng.stream_begin(SLOTS, 512, NO_STOP)
        W = Windows(scfg, halo, cf, rng)
        free, slot_utt, lens, nxt, pending, passes = list(range(SLOTS)), {}, [0] * N_RAGGED, 0, [], 0
        while nxt < N_RAGGED or slot_utt or pending:
            while nxt < N_RAGGED and free:
                s = free.pop(0)
                eng.stream_admit([s], [prompts[nxt]])
                W.admit(s)
                slot_utt[s] = nxt
                nxt += 1
            eng.stream_launch(LOOK_IN)
            window_pass(snac, pending)
            passes += bool(pending)
            _, cnt, done, fin = eng.stream_wait()
            pending = W.cut(cnt // 7, done)
            for s, c in fin:
                lens[slot_utt.pop(s)] = c
                free.append(s)
        eng.stream_end()
        ts.append(time.perf_counter() - t)
    assert lens == RAGGED_LENGTHS
    return {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "tokens_per_s": round(sum(lens) / med(ts), 1), "codec_passes": passes, "codec": "every pass included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mix-reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="orpheus_stream_chunked_parent_before.json: the floor of (b) and the parent's legs come from it")
    ap.add_argument("--only-a", action="store_true", help="leg (a) alone, for alternating processes of two builds: printed, and appended as one JSON line to --out when given")
    args = ap.parse_args()
    chunked = hasattr(hip.OrpheusEngine, "stream_launch")
    out_path = args.out or os.path.join(HERE, "orpheus_stream_chunked.json" if chunked else "orpheus_stream_chunked_parent_before.json")
    cfg = synth.orpheus_3b(ctx=PROMPT + MAX_NEW + 4, weight_type=gguf.Q4_0)
    tensors, _ = sb.orpheus_tensors(cfg, np.random.default_rng(7))
    rng = np.random.default_rng(11)
    prompts = [rng.integers(0, cfg.vocab, PROMPT).astype(np.uint32) for _ in range(SLOTS)]
    scfg = synth.snac_24khz()
    snac = hip.SnacEngine(scfg)
    snac.load(synth.build_snac(scfg))
    halo = snac.halo_frames()
    out = {"setup": {"model": "synthetic Orpheus-3B (28 x 3072, 24 / 8 heads x 128, ffn 8192, 156 940 logits), Q4_0", "codec": "synthetic SNAC 24 kHz, halo %d frames" % halo,
                     "slots": SLOTS, "look_in_steps": LOOK_IN, "max_new": MAX_NEW, "prompt_ids": PROMPT, "reps": args.reps, "mix_reps": args.mix_reps, "sampler": "sampler::max",
                     "timing": "host wall clock, medians", "chunked_session": chunked}}
    eng = hip.OrpheusEngine(cfg, max_seqs=SLOTS)
    eng.load(sb._Model(cfg, tensors))
    eng.generate_batch(prompts, 4, NO_STOP)
    out["a_session_step"] = step_time(eng, prompts, args.reps)
    print("a", json.dumps(out["a_session_step"]), flush=True)
    if args.only_a:
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps({"build_with_chunked_session": chunked, "a_session_step": out["a_session_step"]}) + "\n")
        return
    out["admission"] = admission(eng, prompts, args.reps)
    print("admission", json.dumps(out["admission"]), flush=True)
    out["window_pass_ms"] = {str(cf): one_pass(snac, scfg, halo, cf, args.reps, rng) for cf in CHUNKS}
    # what an unchunked session does for the utterance of (b): its whole-utterance decode, MAX_NEW / 7 frames
    T = 4 * (MAX_NEW // 7)
    full_codes = np.concatenate([rng.integers(0, scfg.cb_size, T // r).astype(np.uint32) for r in scfg.repeats])
    full_noise = rng.standard_normal(int(np.cumprod(scfg.strides).sum()) * T).astype(np.float32)
    ts = []
    for _ in range(args.reps + 1):            # the first one is dropped
        t = time.perf_counter()
        snac.decode(full_codes, T, full_noise)
        ts.append((time.perf_counter() - t) * 1e3)
    out["whole_utterance_decode_ms"] = round(med(ts[1:]), 3)
    print("passes", json.dumps(out["window_pass_ms"]), out["whole_utterance_decode_ms"], flush=True)
    parent = json.load(open(args.parent)) if args.parent else out
    p_step, p_adm = parent["a_session_step"]["session_stream_run_ms_per_step"], parent["admission"]["admission_beside_7_ms"]
    out["b_first_chunk"] = {}
    for cf in CHUNKS:
        steps = LOOK_IN * -(-7 * (cf + halo) // LOOK_IN)
        leg = {"floor_steps": steps, "floor_ms": round(p_adm + steps * p_step + parent["window_pass_ms"][str(cf)], 3),
               "unchunked_session_delivers_after_ms": round(p_adm + (MAX_NEW - 1) * p_step + parent["whole_utterance_decode_ms"], 1),
               "figures_from": "the parent build's file" if args.parent else "this process"}
        if chunked:
            leg.update(first_chunk(eng, snac, scfg, halo, prompts, cf, args.reps, rng))
            leg["over_floor"] = round(leg["first_chunk_ms"] / leg["floor_ms"], 4)
        out["b_first_chunk"][str(cf)] = leg
        print("b", cf, json.dumps(leg), flush=True)
    if chunked:
        out["d_codec_overlap"] = overlap(eng, prompts, args.reps)
        print("d", json.dumps(out["d_codec_overlap"]), flush=True)
    eng.close()
    cfg2 = synth.orpheus_3b(ctx=RAGGED_CTX, weight_type=gguf.Q4_0)
    eng = hip.OrpheusEngine(cfg2, max_seqs=SLOTS)
    eng.load(sb._Model(cfg2, tensors))
    rp = [rng.integers(0, cfg.vocab, RAGGED_CTX + 1 - n).astype(np.uint32) for n in RAGGED_LENGTHS]
    eng.generate_batch(rp[:SLOTS], 4, NO_STOP)
    out["c_ragged_mix"] = {"unchunked_session": mix_unchunked(eng, rp, args.mix_reps)}
    print("c", json.dumps(out["c_ragged_mix"]), flush=True)
    if chunked:
        p_tps = parent["c_ragged_mix"]["unchunked_session"]["tokens_per_s"]
        for cf in CHUNKS:
            leg = mix_chunked(eng, snac, scfg, halo, rp, cf, args.mix_reps, rng)
            leg["of_parent_unchunked_tokens_per_s"] = round(leg["tokens_per_s"] / p_tps, 4)
            out["c_ragged_mix"]["chunked_%d" % cf] = leg
            print("c", cf, json.dumps(leg), flush=True)
    eng.close()
    snac.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
