"""The measurement behind profiles/orpheus_kv_f16.json / orpheus_kv_f16_parent_before.json: the Orpheus decoder step with the fp32 K/V cache and with
the opt-in fp16 cache (TTS_HIP_FLAG_KV_F16), Orpheus-3B shapes, Q4_0 matrices, synthetic weights.

One invocation is one process on one tree: it imports tts_cpp_amd from the WORKING DIRECTORY, so the same file measures any built checkout.  On a tree
that has the flag both cache types run in the same process, alternating repetition by repetition; on a tree without it (the parent) only the fp32 legs:

    (cd PARENT_CHECKOUT && python THIS_FILE --kv f32 --out orpheus_kv_f16_parent_before.json)
    (cd THIS_CHECKOUT   && python THIS_FILE --out orpheus_kv_f16.json)
    python THIS_FILE --report orpheus_kv_f16_parent_before.json orpheus_kv_f16.json

  one_sequence   the captured one-row step (tts_hip_orpheus_generate_greedy): a prompt of 1100 ids, then the time of 408 ids less the time of 8 ids over the
                 400 steps between them — positions 1108 .. 1507; ms per step
  lock_step      tts_hip_orpheus_gen_launch at 8, 32 and 64 rows, every row with a prompt of P - 8 ids: 8 steps of warm-up, then 24 timed steps at positions
                 P .. P + 23, P = 512 and 1536; ms per step (a host clock around gen_launch + gen_wait, which ends in a device synchronise)
  attention      the same lock-step steps run once more under tts_hip_profile (eager, every launch between events): ms per step in the attention launches
                 (class attn_self: attn_gqa_*_kernel [+ attn_gqa_combine_kernel], 28 per step) and the K/V bytes they are asked to read.  Profiling turns the
                 fused projections off, so only the attention figure of that run is reported.  null on a tree whose Llama forward is not instrumented.

Every figure is the list of its repetitions; the report prints min / median / max."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

NO_STOP = 0xFFFFFFFF
CTX = 1600
ONE_PROMPT, ONE_SHORT, ONE_LONG = 1100, 8, 408
ROWS = (8, 32, 64)
POSITIONS = (512, 1536)
WARM, STEPS = 8, 24


def r4(v):
    return [round(float(x), 4) for x in v]


def one_sequence(eng, prompt):
    t = time.perf_counter()
    assert len(eng.generate_greedy(prompt, ONE_SHORT, NO_STOP)) == ONE_SHORT
    a = time.perf_counter() - t
    t = time.perf_counter()
    assert len(eng.generate_greedy(prompt, ONE_LONG, NO_STOP)) == ONE_LONG
    b = time.perf_counter() - t
    return (b - a) / (ONE_LONG - ONE_SHORT) * 1e3


def lock_step(eng, prompts, profile=False):
    """-> ms per step, or under profile (ms per step in the attention launches, K/V bytes per step they are asked to read)"""
    eng.gen_begin(prompts, WARM + STEPS + 1, NO_STOP)
    eng.gen_launch(WARM)
    eng.gen_wait()
    if profile:
        eng.L.tts_hip_profile(eng.ctx, 1)
    t = time.perf_counter()
    eng.gen_launch(STEPS)
    eng.gen_wait()
    ms = (time.perf_counter() - t) / STEPS * 1e3
    if profile:
        import ctypes
        from tts_cpp_amd import hip
        st = hip.KStat()
        eng._chk(eng.L.tts_hip_profile_get(eng.ctx, hip.KCLASSES.index("attn_self"), ctypes.byref(st)))
        eng._chk(eng.L.tts_hip_profile(eng.ctx, 0))
        ms = (st.ms_total / STEPS, st.bytes_total / STEPS) if st.launches else None
    eng.gen_launch(1)
    assert all(eng.gen_wait()[1])
    return ms


def measure(args):
    root = os.getcwd()
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "profiles"))
    import tts_cpp_amd  # noqa: F401
    from tts_cpp_amd import gguf, hip, synth
    import secondary_bench as sb
    assert os.path.dirname(os.path.abspath(hip.__file__)).startswith(root), hip.__file__
    flag = getattr(hip, "FLAG_KV_F16", None)
    kinds = [k for k in args.kv.split(",") if k == "f32" or flag is not None]
    assert kinds, "this tree has no fp16 K/V cache"
    cfg = synth.orpheus_3b(ctx=CTX, weight_type=gguf.Q4_0)
    tensors, _ = sb.orpheus_tensors(cfg, np.random.default_rng(7))
    model = sb._Model(cfg, tensors)
    prng = np.random.default_rng(11)
    res = {"shapes": "orpheus-3b Q4_0, ctx %d" % CTX, "kv": kinds, "one_sequence_ms_per_step": {k: [] for k in kinds}, "lock_step_ms_per_step": {},
           "attention_ms_per_step": {}, "attention_kv_bytes_per_step": {}}

    def engine(kind, max_seqs):
        eng = hip.OrpheusEngine(cfg, max_seqs=max_seqs, **({"flags": flag} if kind == "f16" else {}))
        eng.load(model)
        if kind == "f16":
            assert int(eng.debug_read("l_kv_elem", 1)[0]) == 2
        return eng

    ones = {k: engine(k, 1) for k in kinds}
    prompt = prng.integers(0, cfg.vocab, ONE_PROMPT).astype(np.uint32)
    for k in kinds:
        one_sequence(ones[k], prompt)      # warm-up: the graph is captured, every shape has run
    for _ in range(args.reps):
        for k in kinds:
            res["one_sequence_ms_per_step"][k].append(one_sequence(ones[k], prompt))
    print("one sequence, positions %d..%d" % (ONE_PROMPT + ONE_SHORT, ONE_PROMPT + ONE_LONG - 1), json.dumps({k: r4(v) for k, v in res["one_sequence_ms_per_step"].items()}), flush=True)
    for e in ones.values():
        e.close()
    if args.legs == "one":
        res["one_sequence_ms_per_step"] = {k: r4(v) for k, v in res["one_sequence_ms_per_step"].items()}
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    many = {k: engine(k, max(ROWS)) for k in kinds}
    for P in POSITIONS:
        for B in ROWS:
            prompts = [prng.integers(0, cfg.vocab, P - WARM).astype(np.uint32) for _ in range(B)]
            leg = "%d rows, positions %d..%d" % (B, P, P + STEPS - 1)
            out = {k: [] for k in kinds}
            for k in kinds:
                lock_step(many[k], prompts)      # warm-up
            for _ in range(args.reps):
                for k in kinds:
                    out[k].append(lock_step(many[k], prompts))
            res["lock_step_ms_per_step"][leg] = {k: r4(v) for k, v in out.items()}
            att = {k: lock_step(many[k], prompts, profile=True) for k in kinds}
            res["attention_ms_per_step"][leg] = {k: None if v is None else round(v[0], 4) for k, v in att.items()}
            res["attention_kv_bytes_per_step"][leg] = {k: None if v is None else int(v[1]) for k, v in att.items()}
            print(leg, json.dumps(res["lock_step_ms_per_step"][leg]), "attention", json.dumps(res["attention_ms_per_step"][leg]), flush=True)
    for e in many.values():
        e.close()
    res["one_sequence_ms_per_step"] = {k: r4(v) for k, v in res["one_sequence_ms_per_step"].items()}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


def report(files):
    def mmm(v):
        return "%.4f / %.4f / %.4f" % (min(v), statistics.median(v), max(v))
    for fn in files:
        d = json.load(open(fn))
        print(fn, "(%s)" % d["shapes"])
        for k, v in d["one_sequence_ms_per_step"].items():
            print("  one sequence %-4s %s ms per step" % (k, mmm(v)))
        for leg, kinds in d["lock_step_ms_per_step"].items():
            for k, v in kinds.items():
                a = d["attention_ms_per_step"][leg][k]
                print("  %-34s %-4s %s ms per step   attention %s" % (leg, k, mmm(v), "-" if a is None else "%.4f" % a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--kv", default="f32,f16", help="cache types to measure (f16 is dropped on a tree without the flag)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="all", choices=["all", "one"], help="one: the one-sequence leg only")
    ap.add_argument("--report", nargs="+", metavar="FILE")
    args = ap.parse_args()
    if args.report:
        return report(args.report)
    measure(args)


if __name__ == "__main__":
    main()
