"""The measurement behind profiles/dia_many_rows.json / dia_many_rows_parent_before.json: the Dia device loop's step at 8 .. 128 utterance slots, on the
16-feature GEMM (contexts of at most 64 slots by default) and on the tiled route (tune("dia_tile_min_rows"), the default above 64 slots).  Dia-1.6B shapes,
synthetic fp16 matrices (secondary_bench.dia_tensors), fp32 and fp16 K/V caches.  After profiles/dia_kv_f16_bench.py and profiles/orpheus_stream_bench.py.

It imports tts_cpp_amd from the WORKING DIRECTORY, so the same file measures any built checkout.  One process runs every leg of its tree once (the weights
are synthesised once per process); the orchestrator starts the parent's process and this tree's in turn, --reps times, so two builds are compared in
alternating processes and a figure's spread is the spread between processes:

    python THIS_FILE --parent PARENT_CHECKOUT --reps 5 --out dia_many_rows.json --parent-out dia_many_rows_parent_before.json
    python THIS_FILE --report dia_many_rows_parent_before.json dia_many_rows.json

One leg: a context of `ctx` slots, `live` of them encoded with a 200-byte sentence and stepped by the greedy loop of tts_hip_dia_gen_begin (max_gen 2100):
on to the position, 16 steps of warm-up, then the timed steps; ms per step from a host clock around gen_launch + gen_wait (one look-in inside).  Legs:
  parent      8, 9, 12, 16, 32, 64 slots on contexts of that size (9 and 12: the 18- and 24-row steps that settle the large contexts' threshold)
  this tree   the same with the key off (the default there: the parent's launches) and on (9 .. 64 slots; 8 slots are 16 rows, the streaming route on
              every context); 64 live utterances on a 128-slot context; 128 slots
--far adds the legs at position 2000 (8 and 64 slots, 64 live of 128): 2000 steps to get there, so they run in the first --far-reps repetitions only.
--profile: one eager 256-row step (128 slots, position 100) under tts_hip_profile, by class.
Every figure is the list of its repetitions; the report prints median and max - min."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

MAX_GEN = 2100
WARM = 16
DELAY = [0, 8, 9, 10, 11, 12, 13, 14, 15]


def _setup():
    root = os.getcwd()
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "profiles"))
    import tts_cpp_amd  # noqa: F401
    from tts_cpp_amd import gguf, hip, synth
    import secondary_bench as sb
    assert os.path.dirname(os.path.abspath(hip.__file__)).startswith(root), hip.__file__
    cfg = synth.dia_1_6b(weight_type=gguf.F16, max_gen=MAX_GEN)
    rng = np.random.default_rng(3)
    tensors, _ = sb.dia_tensors(cfg, rng)
    toks = np.zeros(cfg.max_ctx, dtype=np.uint32)
    toks[:200] = rng.integers(32, 127, 200)
    return gguf, hip, cfg, sb._Model(cfg, tensors), toks


def _engine(gguf, hip, cfg, model, toks, ctx, live, kv, key):
    eng = hip.DiaEngine(cfg, max_utterances=ctx, **({"kv_type": gguf.F16} if kv == "f16" else {}))
    if key is not None:
        eng.tune("dia_tile_min_rows", key)
    eng.load(model)
    for u in range(live):
        eng.encode_slot(u, toks, 200)
    return eng


def one_leg(env, ctx, live, kv, key, positions, steps):
    gguf, hip, cfg, model, toks = env
    eng = _engine(gguf, hip, cfg, model, toks, ctx, live, kv, key)
    eng.gen_begin(live, MAX_GEN, DELAY, cfg.bos, cfg.eos, cfg.pad, 15)
    out, at = {}, 0
    for P in positions:
        eng.gen_launch(P - WARM - at)
        eng.gen_wait(take=False)
        eng.gen_launch(WARM)
        eng.gen_wait(take=False)
        t = time.perf_counter()
        eng.gen_launch(steps)
        _, done_steps, done, _ = eng.gen_wait(take=False)
        out[str(P)] = round((time.perf_counter() - t) / steps * 1e3, 4)
        at = P + steps
        assert not done.any() and min(done_steps) >= at - 1, (done_steps, done)
    try:
        out["di_tiled"] = int(eng.debug_read("di_tiled", 1)[0])
    except Exception:      # a tree without the route
        out["di_tiled"] = 0
    eng.close()
    return out


def legs_of(tree, far):
    """(name, ctx slots, live, key) of a tree's legs; key None = the context's default.  9 and 12 slots are the 18- and 24-row steps that settle the
    threshold of the large contexts (16 slots: 32 rows)"""
    if tree == "parent":
        L = [("%d slots" % s, s, s, None) for s in ((8, 64) if far else (8, 9, 12, 16, 32, 64))]
    elif far:
        L = [("8 slots, key off", 8, 8, None), ("64 slots, key off", 64, 64, None), ("64 live of 128 slots", 128, 64, None)]
    else:
        L = [("%d slots, key off" % s, s, s, None) for s in (8, 9, 12, 16, 32, 64)] + [("%d slots, key on" % s, s, s, 17) for s in (9, 12, 16, 32, 64)]
        L += [("64 live of 128 slots", 128, 64, None), ("128 slots", 128, 128, None)]
    return L


def run_tree(args):
    env = _setup()
    positions = [2000] if args.far else [100]
    res = {}
    for name, ctx, live, key in legs_of(args.tree, args.far):
        for kv in args.kv.split(","):
            r = one_leg(env, ctx, live, kv, key, positions, args.steps)
            res["%s, %s cache" % (name, kv)] = r
            print("#", name, kv, json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(res))


def run_profile(args):
    gguf, hip, cfg, model, toks = env = _setup()
    res = {}
    for kv in args.kv.split(","):
        eng = _engine(*env, 128, 128, kv, None)
        ids = np.full((128, cfg.n_out), cfg.bos, dtype=np.uint32)
        pos = np.full(128, 100, dtype=np.uint32)
        eng.step_batch(ids, pos)
        hip.engine_profile(eng, 1)
        for _ in range(3):
            eng.step_batch(ids, pos)
        st = hip.engine_profile_get(eng)
        hip.engine_profile(eng, 0)
        res[kv] = {k: {"ms_per_step": round(v["ms_total"] / 3, 4), "launches_per_step": v["launches"] // 3} for k, v in st.items() if v["launches"]}
        res[kv]["di_tiled"] = int(eng.debug_read("di_tiled", 1)[0])
        eng.close()
    print(json.dumps(res))


def orchestrate(args):
    me = os.path.abspath(__file__)
    outs = {"this": {}, "parent": {}}
    meta = {"shapes": "dia-1.6b, fp16 matrices, max_gen %d, 200-byte sentences; ms per step of the device loop" % MAX_GEN, "steps_timed": args.steps}

    def child(tree, cwd, far):
        cmd = [sys.executable, me, "--tree", tree, "--kv", args.kv, "--steps", str(args.steps)] + (["--far"] if far else [])
        p = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=1100)
        sys.stderr.write(p.stderr[-4000:])
        if p.returncode != 0:
            raise SystemExit("%s tree: exit %d: nothing more is started on this device" % (tree, p.returncode))
        for name, r in json.loads(p.stdout.strip().splitlines()[-1]).items():
            slot = outs[tree].setdefault(name, {})
            for k, v in r.items():
                slot.setdefault(k, []).append(v)
        dump()

    def dump():
        for tree, fn in (("this", args.out), ("parent", args.parent_out)):
            if fn and outs[tree]:
                own = {k: v for k, v in meta.items() if tree == "this" or k != "profile_256_rows_eager"}      # the profiled step is this tree's
                with open(fn, "w") as f:
                    json.dump(dict(own, tree=tree, ms_per_step=outs[tree]), f, indent=1)

    for rep in range(args.reps):
        if args.parent:
            child("parent", args.parent, False)
        child("this", os.getcwd(), False)
        if args.far and rep < args.far_reps:
            if args.parent:
                child("parent", args.parent, True)
            child("this", os.getcwd(), True)
    if args.with_profile:
        p = subprocess.run([sys.executable, me, "--profile", "--kv", args.kv], capture_output=True, text=True, timeout=600)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode == 0:
            meta["profile_256_rows_eager"] = json.loads(p.stdout.strip().splitlines()[-1])
        dump()


def report(files):
    for fn in files:
        d = json.load(open(fn))
        print(fn, "(%s)" % d["shapes"])
        for name, by in d["ms_per_step"].items():
            for k, v in by.items():
                if k != "di_tiled":
                    print("  %-36s position %-5s median %.4f  max - min %.4f  (%d)  tiled launches %s" % (name, k, statistics.median(v), max(v) - min(v), len(v), by.get("di_tiled", ["-"])[0]))
        for kv, classes in d.get("profile_256_rows_eager", {}).items():
            print("  eager 256-row step, %s cache:" % kv, json.dumps(classes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--parent-out")
    ap.add_argument("--kv", default="f32,f16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64, help="timed steps per leg")
    ap.add_argument("--far", action="store_true", help="also the legs at position 2000, in the first --far-reps repetitions")
    ap.add_argument("--far-reps", type=int, default=2)
    ap.add_argument("--with-profile", action="store_true")
    ap.add_argument("--tree", help="internal: run the legs of 'this' or 'parent' tree in this process")
    ap.add_argument("--profile", action="store_true", help="internal: the eager 256-row step by class")
    ap.add_argument("--report", nargs="+", metavar="FILE")
    args = ap.parse_args()
    if args.report:
        return report(args.report)
    if args.profile:
        return run_profile(args)
    if args.tree:
        return run_tree(args)
    orchestrate(args)


if __name__ == "__main__":
    main()
