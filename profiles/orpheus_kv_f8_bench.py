"""The measurement behind profiles/orpheus_kv_f8.json / orpheus_kv_f8_parent_before.json: the Orpheus decoder step over the fp32 K/V cache, the fp16 cache
(TTS_HIP_FLAG_KV_F16) and the opt-in e4m3 cache (tts_hip_orpheus_desc::kv_type = TTS_HIP_KV_F8_E4M3), Orpheus-3B shapes, Q4_0 matrices, synthetic weights.
Built on profiles/orpheus_kv_f16_bench.py (the one-sequence leg is its function) and the 128 / 256-slot legs of orpheus_stream_bench.py --many-rows.

One invocation is one process on one tree: it imports tts_cpp_amd from the WORKING DIRECTORY, so the same file measures any built checkout.  Every cache
type the tree has runs in the same process, alternating repetition by repetition; a tree without hip.KV_F8_E4M3 (the parent) runs the fp32 and fp16 legs:

    (cd PARENT_CHECKOUT && python THIS_FILE --out orpheus_kv_f8_parent_before.json)
    (cd THIS_CHECKOUT   && python THIS_FILE --out orpheus_kv_f8.json)
    python THIS_FILE --report orpheus_kv_f8_parent_before.json orpheus_kv_f8.json

  one_sequence   the captured one-row step, positions 1108 .. 1507 (orpheus_kv_f16_bench.one_sequence); ms per step, a warm-up then --reps repetitions
  lock_step      tts_hip_orpheus_gen_launch at 8, 32 and 64 rows, every row behind a prompt of P - 8 ids, P = 512 and 1536: 8 steps of warm-up, then --reps
                 timed stretches of 24 steps each, one after the other in the same generation (positions P .. P + 24 reps - 1), the cache types taking
                 turns stretch by stretch; ms per step (a host clock around gen_launch + gen_wait, which ends in a device synchronise)
  attention      24 further steps of the same generations under tts_hip_profile (eager, every launch between events): ms per step in the attention
                 launches (class attn_self) and the K/V bytes they are asked to read
  slots          tts_hip_orpheus_stream_run at 128 and 256 slots, every slot behind a prompt of 480 ids (n_ctx 1024): 8 steps of warm-up, then --reps
                 timed stretches of 24 steps in the same session, the cache types taking turns; ms per step; then one profiled step: attn_self ms
  --trace-256    nothing is timed: a 256-slot session over ONE cache type (--kv) runs 8 + 24 steps, for a rocprofv3 --kernel-trace --stats run of its own
                 (per-kernel times of attn_gqa_kernel<128, false, KV>)

Every figure is the list of its repetitions; the report prints median (min .. max)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

NO_STOP = 0xFFFFFFFF
CTX = 1700
ROWS = (8, 32, 64)
POSITIONS = (512, 1536)
SLOTS = (128, 256)
SLOT_CTX, SLOT_PROMPT = 1024, 480
WARM, STEPS = 8, 24


def r4(v):
    return [round(float(x), 4) for x in v]


def attn_self(eng, hip):
    import ctypes
    st = hip.KStat()
    eng._chk(eng.L.tts_hip_profile_get(eng.ctx, hip.KCLASSES.index("attn_self"), ctypes.byref(st)))
    return st


def measure(args):
    root = os.getcwd()
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "profiles"))
    import tts_cpp_amd  # noqa: F401
    from tts_cpp_amd import gguf, hip, synth
    import orpheus_kv_f16_bench as b16
    import secondary_bench as sb
    assert os.path.dirname(os.path.abspath(hip.__file__)).startswith(root), hip.__file__
    f8 = getattr(hip, "KV_F8_E4M3", None)
    kinds = [k for k in args.kv.split(",") if k != "f8" or f8 is not None]
    how = {"f32": ({}, 4), "f16": ({"flags": hip.FLAG_KV_F16}, 2), "f8": ({"kv_type": f8}, 1)}
    reps = args.reps

    tensors = sb.orpheus_tensors(synth.orpheus_3b(ctx=CTX, weight_type=gguf.Q4_0), np.random.default_rng(7))[0]

    def build(ctx):      # the same tensors under either context length
        cfg = synth.orpheus_3b(ctx=ctx, weight_type=gguf.Q4_0)
        return cfg, sb._Model(cfg, tensors)

    def engine(cfg, model, kind, max_seqs):
        eng = hip.OrpheusEngine(cfg, max_seqs=max_seqs, **how[kind][0])
        eng.load(model)
        assert int(eng.debug_read("l_kv_elem", 1)[0]) == how[kind][1]
        return eng

    prng = np.random.default_rng(11)
    if args.trace_256:
        cfg, model = build(SLOT_CTX)
        eng = engine(cfg, model, kinds[0], 256)
        eng.stream_begin(256, WARM + STEPS + 2, NO_STOP)
        eng.stream_admit(list(range(256)), [prng.integers(0, cfg.vocab, SLOT_PROMPT).astype(np.uint32) for _ in range(256)])
        assert eng.stream_run(WARM + STEPS) == []
        eng.stream_end()
        eng.close()
        return
    res = {"shapes": "orpheus-3b Q4_0, n_ctx %d (slots legs: %d)" % (CTX, SLOT_CTX), "kv": kinds, "reps": reps, "one_sequence_ms_per_step": {}, "lock_step_ms_per_step": {},
           "attention_ms_per_step": {}, "attention_kv_bytes_per_step": {}, "slots_ms_per_step": {}, "slots_attention_ms_per_profiled_step": {}}

    def save():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    cfg, model = build(CTX)
    ones = {k: engine(cfg, model, k, 1) for k in kinds}
    prompt = prng.integers(0, cfg.vocab, b16.ONE_PROMPT).astype(np.uint32)
    out = {k: [] for k in kinds}
    for k in kinds:
        b16.one_sequence(ones[k], prompt)      # warm-up: the graph is captured, every shape has run
    for _ in range(reps):
        for k in kinds:
            out[k].append(b16.one_sequence(ones[k], prompt))
    res["one_sequence_ms_per_step"] = {k: r4(v) for k, v in out.items()}
    print("one sequence", json.dumps(res["one_sequence_ms_per_step"]), flush=True)
    save()
    for e in ones.values():
        e.close()
    many = {k: engine(cfg, model, k, max(ROWS)) for k in kinds}
    for P in POSITIONS:
        for B in ROWS:
            prompts = [prng.integers(0, cfg.vocab, P - WARM).astype(np.uint32) for _ in range(B)]
            leg = "%d rows, positions %d..%d" % (B, P, P + STEPS * reps - 1)
            out = {k: [] for k in kinds}
            for k in kinds:
                many[k].gen_begin(prompts, WARM + STEPS * (reps + 1) + 1, NO_STOP)
                many[k].gen_launch(WARM)
                many[k].gen_wait()
            for _ in range(reps):
                for k in kinds:
                    t = time.perf_counter()
                    many[k].gen_launch(STEPS)
                    many[k].gen_wait()
                    out[k].append((time.perf_counter() - t) / STEPS * 1e3)
            res["lock_step_ms_per_step"][leg] = {k: r4(v) for k, v in out.items()}
            att = {}
            for k in kinds:
                e = many[k]
                e.profile(True)
                e.gen_launch(STEPS)
                e.gen_wait()
                st = attn_self(e, hip)
                e.profile(False)
                att[k] = (st.ms_total / STEPS, st.bytes_total / STEPS)
                e.gen_launch(1)
                assert all(e.gen_wait()[1])
            res["attention_ms_per_step"][leg] = {k: round(v[0], 4) for k, v in att.items()}
            res["attention_kv_bytes_per_step"][leg] = {k: int(v[1]) for k, v in att.items()}
            print(leg, json.dumps(res["lock_step_ms_per_step"][leg]), "attention", json.dumps(res["attention_ms_per_step"][leg]), flush=True)
            save()
    for e in many.values():
        e.close()
    if args.legs == "all":
        cfg, model = build(SLOT_CTX)
        for B in SLOTS:
            prompts = [prng.integers(0, cfg.vocab, SLOT_PROMPT).astype(np.uint32) for _ in range(B)]
            engs = {k: engine(cfg, model, k, B) for k in kinds}
            leg = "%d slots, positions %d..%d" % (B, SLOT_PROMPT + WARM, SLOT_PROMPT + WARM + STEPS * reps - 1)
            out = {k: [] for k in kinds}
            for k in kinds:
                engs[k].stream_begin(B, WARM + STEPS * reps + 8, NO_STOP)
                engs[k].stream_admit(list(range(B)), prompts)
                assert engs[k].stream_run(WARM) == []
            for _ in range(reps):
                for k in kinds:
                    t = time.perf_counter()
                    fin = engs[k].stream_run(STEPS)
                    out[k].append((time.perf_counter() - t) / STEPS * 1e3)
                    assert fin == []
            res["slots_ms_per_step"][leg] = {k: r4(v) for k, v in out.items()}
            att = {}
            for k in kinds:      # one eager step with every launch timed (slower as a whole than the timed steps above; only its attention figure is kept)
                e = engs[k]
                e.profile(True)
                e.stream_run(1)
                st = attn_self(e, hip)
                e.profile(False)
                e.stream_end()
                att[k] = round(st.ms_total, 4)
            res["slots_attention_ms_per_profiled_step"][leg] = att
            print(leg, json.dumps(res["slots_ms_per_step"][leg]), "attention of one profiled step", json.dumps(att), flush=True)
            save()
            for e in engs.values():
                e.close()


def report(files):
    def mmm(v):
        return "%.4f (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))
    for fn in files:
        d = json.load(open(fn))
        print(fn, "(%s)" % d["shapes"])
        for k, v in d["one_sequence_ms_per_step"].items():
            print("  one sequence %-4s %s ms per step" % (k, mmm(v)))
        for leg, kinds in d["lock_step_ms_per_step"].items():
            for k, v in kinds.items():
                print("  %-34s %-4s %s ms per step   attention %.4f" % (leg, k, mmm(v), d["attention_ms_per_step"][leg][k]))
        for leg, kinds in d["slots_ms_per_step"].items():
            for k, v in kinds.items():
                print("  %-34s %-4s %s ms per step   attention of one profiled step %.4f" % (leg, k, mmm(v), d["slots_attention_ms_per_profiled_step"][leg][k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--kv", default="f32,f16,f8", help="cache types to measure (f8 is dropped on a tree without it)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="all", choices=["all", "rows"], help="rows: without the 128 / 256-slot legs")
    ap.add_argument("--trace-256", action="store_true", help="run a 256-slot session over the first cache type of --kv and time nothing (for rocprofv3)")
    ap.add_argument("--report", nargs="+", metavar="FILE")
    args = ap.parse_args()
    if args.report:
        return report(args.report)
    measure(args)


if __name__ == "__main__":
    main()
