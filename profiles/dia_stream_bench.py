"""Dia-1.6B shapes (synth.dia_1_6b, fp16 matrices, every matrix a slice of one small-normal buffer as in dia_bench.py), 4 utterance slots: the
lock-step loop of tts_hip_dia_generate against the continuous session (tts_hip_dia_stream_*).

  (a) step time     the session step with all 4 slots live (tts_hip_dia_stream_run) against the tts_hip_dia_gen_launch step at n_utt = 4, the
                    same positions (WARM .. WARM + STEPS) on both sides.  The forward is the same; the pre-step differs and parked slots sit
                    out of the sampler.  Gate: within the lock-step leg's own run-to-run spread (max - min of its runs) on the parent commit.
  (b) ragged mix    N_RAGGED utterances whose step counts (LENGTHS) spread over 10:1, once through one session of 4 slots that refills freed
                    slots at a look-in every 16 steps (per-slot budgets), once as consecutive groups of 4 the way generate_batch runs them: four
                    encoder passes, then tts_hip_dia_generate until the group's longest utterance is done (its max_gen is the group's largest
                    budget: the lock-step loop has one budget per call, and a finished utterance keeps its two rows in every step anyway, so the
                    group costs what it costs when EOS ends the short ones).  Audio-seconds/s counts each utterance's own frames
                    (steps - max_delay) at 86.13 frames/s over the wall time of the decoder side, encoder passes included, codec excluded on both
                    legs; live share = the utterances' own slot-steps over 4 x the steps that ran.
  (c) admission     wall time of one tts_hip_dia_stream_admit (encoder pass, cross K/V fill, admit launch, synchronise) while 3 slots are live

A build without the session (hip.DiaEngine has no stream_begin) runs the lock-step legs only and writes
dia_stream_throughput_parent_before.json: that is how the parent commit was measured.
Usage: python profiles/dia_stream_bench.py [--out FILE] [--reps N]"""
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

SLOTS, LOOK_IN = 4, 16
WARM, STEPS = 16, 128
LENGTHS = [1000, 100, 300, 150, 700, 120, 500, 200, 900, 110, 400, 250]   # steps per utterance, 10:1
N_RAGGED = len(LENGTHS)
FRAMES_PER_S = 86.13
TEXT_LEN = 200


def med(v):
    return float(np.median(v))


def build_model(cfg, rng):
    pool16 = (rng.standard_normal(1 << 25, dtype=np.float32) * np.float32(0.02)).astype(np.float16).view(np.uint8)
    pool32 = (rng.standard_normal(1 << 22, dtype=np.float32) * np.float32(0.5)).view(np.uint8)
    EH, DH, A, kvH = cfg.enc_hidden, cfg.dec_hidden, cfg.dec_heads * cfg.head_dim, cfg.dec_kv_heads * cfg.head_dim
    tensors = []

    def mat(name, rows, cols):
        tensors.append(gguf.Tensor(name, gguf.F16, [cols, rows], pool16[: rows * cols * 2]))

    def vec(name, n):
        tensors.append(gguf.Tensor.from_array(name, np.ones(n, dtype=np.float32)))

    def table(name, rows, cols):
        tensors.append(gguf.Tensor(name, gguf.F32, [cols, rows], pool32[: rows * cols * 4]))

    # the head rows of EOS / PAD / BOS are zero, so sampler::max never selects them and the budgets alone set the lengths
    heads = pool16[: cfg.out_vocab * DH * 2].copy()
    heads[cfg.audio_vocab * DH * 2:] = 0
    for i in range(cfg.n_out):
        table(f"dia.decoder.embeddings.{i}", cfg.out_vocab, DH)
        tensors.append(gguf.Tensor(f"dia.decoder.heads.{i}", gguf.F16, [DH, cfg.out_vocab], heads))
    vec("dia.decoder.norm", DH)
    for l in range(cfg.dec_layers):
        p = f"dia.decoder.layers.{l}."
        for nm in ("pre_sa_norm", "pre_ca_norm", "pre_mlp_norm"):
            vec(p + nm, DH)
        for nm, r, c in (("self_q_proj", A, DH), ("self_k_proj", kvH, DH), ("self_v_proj", kvH, DH), ("self_o_proj", DH, A), ("cross_q_proj", A, DH),
                         ("cross_k_proj", A, EH), ("cross_v_proj", A, EH), ("cross_o_proj", DH, A), ("gate", cfg.dec_ffn, DH), ("up", cfg.dec_ffn, DH),
                         ("wo", DH, cfg.dec_ffn)):
            mat(p + nm, r, c)
    table("dia.encoder.embedding", cfg.enc_vocab, EH)
    vec("dia.encoder.norm", EH)
    for l in range(cfg.enc_layers):
        p = f"dia.encoder.layers.{l}."
        vec(p + "pre_sa_norm", EH)
        vec(p + "post_sa_norm", EH)
        for nm, r, c in (("q_proj", A, EH), ("k_proj", A, EH), ("v_proj", A, EH), ("o_proj", EH, A), ("gate", cfg.enc_ffn, EH), ("up", cfg.enc_ffn, EH),
                         ("wo", EH, cfg.enc_ffn)):
            mat(p + nm, r, c)

    class M:
        pass

    m = M()
    m.cfg, m.tensors = cfg, tensors
    return m


def step_time(eng, a, toks, have_session, reps):
    cfg = eng.cfg
    for s in range(SLOTS):
        eng.encode_slot(s, toks, TEXT_LEN)
    lock, sess = [], []
    for _ in range(reps + 1):               # the first repetition captures the graph and is dropped
        eng.gen_begin(SLOTS, cfg.max_gen, **a)
        eng.gen_launch(WARM)
        eng.gen_wait(take=False)
        t = time.perf_counter()
        eng.gen_launch(STEPS)
        _, steps, done, _ = eng.gen_wait(take=False)
        lock.append((time.perf_counter() - t) / STEPS * 1e3)
        assert not done.any() and (steps == WARM + STEPS).all()
    lock = lock[1:]
    out = {"lockstep_gen_launch_ms_per_step": round(med(lock), 4), "lockstep_runs_ms": [round(x, 4) for x in lock],
           "lockstep_spread_ms": round(max(lock) - min(lock), 4)}
    if not have_session:
        return out
    for _ in range(reps + 1):
        eng.stream_begin(SLOTS, cfg.max_gen, **a)
        eng.stream_admit(list(range(SLOTS)), [toks] * SLOTS, [TEXT_LEN] * SLOTS)
        assert eng.stream_run(WARM) == []
        t = time.perf_counter()
        fin = eng.stream_run(STEPS)
        sess.append((time.perf_counter() - t) / STEPS * 1e3)
        assert fin == []
        eng.stream_end()
    sess = sess[1:]
    out.update({"session_stream_run_ms_per_step": round(med(sess), 4), "session_runs_ms": [round(x, 4) for x in sess],
                "session_minus_lockstep_ms": round(med(sess) - med(lock), 4), "session_over_lockstep": round(med(sess) / med(lock), 4)})
    return out


def ragged(eng, a, texts, have_session, reps):
    cfg = eng.cfg
    budgets = [n + 1 for n in LENGTHS]
    frames = sum(n - cfg.max_delay for n in LENGTHS)
    res = {"utterances": N_RAGGED, "slots": SLOTS, "lengths_steps": LENGTHS, "audio_seconds": round(frames / FRAMES_PER_S, 3)}
    ts, ran = [], 0
    for _ in range(reps):
        t = time.perf_counter()
        ran = 0
        for g0 in range(0, N_RAGGED, SLOTS):
            for s in range(SLOTS):
                eng.encode_slot(s, texts[g0 + s], TEXT_LEN)
            got = eng.generate(SLOTS, max(budgets[g0:g0 + SLOTS]), **a)
            ran += max(len(g) for g in got)
        ts.append(time.perf_counter() - t)
    res["generate_batch_groups"] = {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "steps_run": ran,
                                    "audio_seconds_per_s": round(frames / FRAMES_PER_S / med(ts), 3),
                                    "live_share_of_slot_steps": round(sum(LENGTHS) / (SLOTS * ran), 4)}
    if not have_session:
        return res
    ts, runs, lens = [], 0, None
    for _ in range(reps):
        t = time.perf_counter()
        eng.stream_begin(SLOTS, cfg.max_gen, **a)
        free, slot_utt, lens, nxt, steps_run = list(range(SLOTS)), {}, [0] * N_RAGGED, 0, 0
        while nxt < N_RAGGED or slot_utt:
            take = []
            while nxt < N_RAGGED and free:
                take.append((free.pop(0), nxt))
                nxt += 1
            if take:
                eng.stream_admit([s for s, _ in take], [texts[u] for _, u in take], [TEXT_LEN] * len(take), budgets=[budgets[u] for _, u in take])
                slot_utt.update(take)
            fin = eng.stream_run(LOOK_IN)
            steps_run += LOOK_IN
            for s, n in fin:
                u = slot_utt.pop(s)
                lens[u] = len(eng.stream_collect(s, n))
                free.append(s)
        eng.stream_end()
        ts.append(time.perf_counter() - t)
        runs = steps_run
    assert lens == LENGTHS, lens
    res["session"] = {"seconds": round(med(ts), 4), "runs_s": [round(x, 4) for x in ts], "look_in_steps": LOOK_IN, "steps_run_upper_bound": runs,
                      "audio_seconds_per_s": round(frames / FRAMES_PER_S / med(ts), 3), "live_share_of_slot_steps": round(sum(LENGTHS) / (SLOTS * runs), 4),
                      "speedup_over_groups": round(res["generate_batch_groups"]["seconds"] / med(ts), 4)}
    return res


def admission(eng, a, toks, reps):
    cfg = eng.cfg
    ts = []
    for _ in range(reps + 1):
        eng.stream_begin(SLOTS, cfg.max_gen, **a)
        eng.stream_admit([0, 1, 2], [toks] * 3, [TEXT_LEN] * 3)
        assert eng.stream_run(LOOK_IN) == []
        t = time.perf_counter()
        eng.stream_admit([3], [toks], [TEXT_LEN])
        ts.append((time.perf_counter() - t) * 1e3)
        assert eng.stream_run(LOOK_IN) == []
        eng.stream_end()
    ts = ts[1:]
    return {"live_slots": 3, "admit_one_ms": round(med(ts), 3), "runs_ms": [round(x, 3) for x in ts]}


def main():
    have_session = hasattr(hip.DiaEngine, "stream_begin")
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "dia_stream_throughput.json" if have_session else "dia_stream_throughput_parent_before.json"))
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
    out = {"setup": {"model": "synthetic Dia-1.6B (encoder 12 x 1024, decoder 18 x 2048, 16 / 4 heads x 128, ffn 8192, 9 x 1028 logits), fp16, 4 slots = 8 rows",
                     "text_bytes": TEXT_LEN, "warm_steps": WARM, "timed_steps": STEPS, "reps": args.reps, "mix_reps": args.mix_reps, "selection": "sampler::max",
                     "session": have_session, "timing": "host wall clock around the blocking calls, median of the runs listed",
                     "command": "python profiles/dia_stream_bench.py --reps %d --mix-reps %d%s" % (args.reps, args.mix_reps,
                                                                                                 "" if have_session else " (this script on a build of the parent commit)")}}
    out["step_time"] = step_time(eng, a, texts[0], have_session, args.reps)
    print("step", json.dumps(out["step_time"]), flush=True)
    out["ragged_mix"] = ragged(eng, a, texts, have_session, args.mix_reps)
    print("ragged", json.dumps(out["ragged_mix"]), flush=True)
    if have_session:
        out["admission"] = admission(eng, a, texts[1], args.reps)
        print("admission", json.dumps(out["admission"]), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
