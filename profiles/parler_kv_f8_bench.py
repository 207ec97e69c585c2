"""The measurement behind profiles/parler_kv_f8.json / parler_kv_f8_parent_before.json: the Parler decoder step of a greedy session over the fp32 K/V
cache, the fp16 cache (kv_type = F16) and the opt-in e4m3 cache (tune("kv_f8")), Parler-Mini shapes, fp16 matrices, synthetic weights, no codec.
Modelled on profiles/orpheus_kv_f8_bench.py and profiles/parler_voices_bench.py.

One invocation is one process on one tree: it imports tts_cpp_amd from the WORKING DIRECTORY, so the same file measures any built checkout.  Every cache
type the tree has runs in the same process, taking turns repetition by repetition; a tree without the tune key (the parent) runs the fp32 and fp16 legs:

    (cd PARENT_CHECKOUT && python THIS_FILE --out parler_kv_f8_parent_before.json)
    (cd THIS_CHECKOUT   && python THIS_FILE --out parler_kv_f8.json)

  step        stream_run at 1023 slots (forwards of 1024 rows) and at 8 slots, every slot behind a prompt of 16 ids (short) or 200 ids (long): WARM steps of
              warm-up (they capture the graph), then --reps timed stretches of STEPS steps in the same session, the cache types taking turns stretch by
              stretch; ms per step (a host clock around the blocking stream_run call)
  attn_self   PROF further steps of the same sessions under tts_hip_profile (eager, every launch between events): ms per step in the self-attention
              launches and the K/V bytes they are asked to read

The e4m3 cache runs twice: "e4m3" with the row-major reader attn_rows_f8_kernel (tune "attn_rows_f8_min" at its default, 256 rows) and "e4m3_attn_kernel"
with attn_rows_f8_min = 0 (attn_kernel at every row count, what the parent of the reader ran); a tree without a key skips the legs that name it.  256 slots
is the reader's four-slice form, 8 slots never reach it.  --extra NAME=key:value,... adds a context with further tune keys to the turns (the sweep over the
reader's keys in flight was run that way on a build that held three instantiations); --kinds restricts the turns.  profiles/parler_kv_f8_rows.json
/ parler_kv_f8_rows_parent_before.json are this file's output at --slots 1023,256,8.
Every figure is the list of its repetitions with its median and max - min."""
import argparse
import json
import os
import sys
import time

import numpy as np

WARM, STEPS, PROF = 8, 16, 4
LEGS = (("short", 16), ("long", 200))
SLOTS = (1023, 256, 8)


def stat(v):
    return {"median": round(float(np.median(v)), 4), "spread": round(float(max(v) - min(v)), 4), "runs": [round(float(x), 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", default=",".join(str(s) for s in SLOTS))
    ap.add_argument("--kinds", default="", help="comma list of the contexts that run (default: all)")
    ap.add_argument("--extra", action="append", default=[], help="NAME=key:value,key:value: one more context, with these tune keys")
    args = ap.parse_args()
    root = os.getcwd()
    sys.path.insert(0, root)
    import tts_cpp_amd  # noqa: F401
    from tts_cpp_amd import gguf, hip, synth
    assert os.path.dirname(os.path.abspath(hip.__file__)).startswith(root), hip.__file__
    reps = args.reps
    total = WARM + STEPS * reps + PROF + 2
    kvpos = max(p for _, p in LEGS) + total + 8
    cfg = synth.parler_mini(weight_type=gguf.F16, max_gen=kvpos)
    model = synth.build(cfg)
    how = {"f32": dict(kv_type=gguf.F32), "f16": dict(kv_type=gguf.F16), "e4m3": dict(kv_type=gguf.F32, tune={"kv_f8": 1}),
           "e4m3_attn_kernel": dict(kv_type=gguf.F32, tune={"kv_f8": 1, "attn_rows_f8_min": 0})}
    for x in args.extra:
        name, keys = x.split("=", 1)
        how[name] = dict(kv_type=gguf.F32, tune={k: int(v) for k, v in (kv.split(":") for kv in keys.split(","))})
    if args.kinds:
        how = {k: how[k] for k in args.kinds.split(",")}
    res = {"shapes": "synthetic Parler-Mini (24 x 1024, 16 heads, ffn 4096, 9 x 1088 logits), fp16 matrices, no codec, %d cached positions" % kvpos,
           "warm_steps": WARM, "timed_steps": STEPS, "profiled_steps": PROF, "reps": reps, "step_ms": {}, "attn_self_ms_per_step": {}, "attn_self_kv_bytes_per_step": {}}
    rng = np.random.default_rng(3)
    for slots in [int(s) for s in args.slots.split(",")]:
        engs = {}
        for kind, kw in how.items():
            try:
                eng = hip.HipEngine(cfg, max_seqs=slots + 1, kv_positions=kvpos, flags=hip.FLAG_NO_DAC, **kw)
            except hip.HipError:      # a tree without the key
                assert "tune" in kw, kind
                continue
            eng.load(model)
            engs[kind] = eng
        for name, plen in LEGS:
            prompts = [rng.integers(3, cfg.prompt_vocab, plen).astype(np.uint32) for _ in range(slots)]
            leg = "%d slots, %s: positions %d..%d" % (slots, name, plen + WARM, plen + WARM + STEPS * reps - 1)
            out = {k: [] for k in engs}
            for k, e in engs.items():
                e.stream_begin(slots, total, sampling=None)      # (the synthetic heads never emit EOS)
                e.stream_admit(list(range(slots)), prompts)
                assert e.stream_run(WARM) == []
            for _ in range(reps):
                for k, e in engs.items():
                    t = time.perf_counter()
                    fin = e.stream_run(STEPS)
                    out[k].append((time.perf_counter() - t) / STEPS * 1e3)
                    assert fin == []
            att, byt = {}, {}
            for k, e in engs.items():
                e.profile(True)
                before = e.profile_get()["attn_self"]
                e.stream_run(PROF)
                after = e.profile_get()["attn_self"]
                e.profile(False)
                e.stream_end()
                att[k] = round((after["ms_total"] - before["ms_total"]) / PROF, 4)
                byt[k] = int((after["bytes_total"] - before["bytes_total"]) / PROF)
            res["step_ms"][leg] = {k: stat(v) for k, v in out.items()}
            res["attn_self_ms_per_step"][leg] = att
            res["attn_self_kv_bytes_per_step"][leg] = byt
            print(leg, json.dumps({k: res["step_ms"][leg][k]["median"] for k in out}), "attn_self", json.dumps(att), flush=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        for e in engs.values():
            e.close()


if __name__ == "__main__":
    main()
