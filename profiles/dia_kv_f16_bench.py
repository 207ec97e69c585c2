"""The measurement behind profiles/dia_kv_f16.json / dia_kv_f16_parent_before.json: the Dia device loop's step with the fp32 K/V caches and with the
opt-in fp16 caches (tts_hip_dia_desc::kv_type), Dia-1.6B shapes, synthetic fp16 matrices (secondary_bench.dia_tensors).

It imports tts_cpp_amd from the WORKING DIRECTORY, so the same file measures any built checkout.  Every leg runs in a process of its own (a fresh child
per repetition, the cache types alternating), so a figure's spread is the spread between processes; on a tree without kv_type (the parent) only fp32 runs:

    (cd PARENT_CHECKOUT && python THIS_FILE --kv f32 --out dia_kv_f16_parent_before.json)
    (cd THIS_CHECKOUT   && python THIS_FILE --out dia_kv_f16.json)
    python THIS_FILE --report dia_kv_f16_parent_before.json dia_kv_f16.json

One leg: S utterance slots (2 S rows), every slot encoded with a 200-byte sentence, the greedy loop of tts_hip_dia_gen_begin with max_gen 2100.  The loop
runs to position 84, then 16 steps of warm-up, then 128 timed steps at positions 100..227; on to 1934, 16 steps, then 128 timed steps at 1950..2077.  ms per
step from a host clock around gen_launch + gen_wait (which ends in a device synchronise; one look-in per 128 steps is inside).  To alternate two trees
process by process, run both with --reps 1 in turn and join the files: python THIS_FILE --merge OUT.json PART1.json PART2.json ...

profiles/dia_kv_f16_u.json holds a run of this script on a build that also held the fp16 EXT kernel (now attn_gqa_wave_kernel<128, U, true, _Float16>) at U = 8 ("f16": all eight passes requested at
once, "f16_u4": the four rolling slots that stayed), 4 slots, two processes each, 48 timed steps at positions 100..147 and 2000..2047.
Every figure is the list of its repetitions; the report prints min / median / max."""
import argparse
import inspect
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

MAX_GEN = 2100
POSITIONS = (100, 1950)
WARM, STEPS = 16, 128
DELAY = [0, 8, 9, 10, 11, 12, 13, 14, 15]


def leg(kind, slots):
    """one process, one cache type, one slot count -> {position: ms per step}"""
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
    kw = {"kv_type": gguf.F16} if kind == "f16" else {}
    eng = hip.DiaEngine(cfg, max_utterances=slots, **kw)
    eng.load(sb._Model(cfg, tensors))
    if kw:
        assert int(eng.debug_read("di_kv_elem", 1)[0]) == 2
    toks = np.zeros(cfg.max_ctx, dtype=np.uint32)
    toks[:200] = rng.integers(32, 127, 200)
    for u in range(slots):
        eng.encode_slot(u, toks, 200)
    eng.gen_begin(slots, MAX_GEN, DELAY, cfg.bos, cfg.eos, cfg.pad, 15)
    out, at = {}, 0
    for P in POSITIONS:
        eng.gen_launch(P - WARM - at)
        eng.gen_wait(take=False)
        eng.gen_launch(WARM)
        eng.gen_wait(take=False)
        t = time.perf_counter()
        eng.gen_launch(STEPS)
        _, steps, done, _ = eng.gen_wait(take=False)
        out[str(P)] = (time.perf_counter() - t) / STEPS * 1e3
        at = P + STEPS
        assert not done.any() and min(steps) >= at - 1, (steps, done)      # every slot is still generating at the timed positions
    eng.close()
    return out


def measure(args):
    root = os.getcwd()
    sys.path.insert(0, root)
    import tts_cpp_amd  # noqa: F401
    from tts_cpp_amd import hip
    has = "kv_type" in inspect.signature(hip.DiaEngine.__init__).parameters
    kinds = [k for k in args.kv.split(",") if k == "f32" or has]
    assert kinds and all(k in ("f32", "f16") for k in kinds), "cache types are f32 and f16; this tree may have no fp16 K/V caches for Dia"
    slot_counts = [int(s) for s in args.slots.split(",")]
    res = {"shapes": "dia-1.6b, fp16 matrices, max_gen %d, 200-byte sentences" % MAX_GEN, "kv": kinds, "steps_timed": STEPS, "ms_per_step": {}}
    for S in slot_counts:
        figs = {k: {str(P): [] for P in POSITIONS} for k in kinds}
        for _ in range(args.reps):
            for k in kinds:      # alternating, a fresh process each
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", k, "--slots", str(S)], capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    print("%d slots %s: exit %d\n%s" % (S, k, p.returncode, p.stderr[-1500:]), flush=True)
                    if p.returncode < 0 or p.returncode in (134, 139):
                        raise SystemExit("a leg crashed: nothing more is started on this device")
                    continue
                one = json.loads(p.stdout.strip().splitlines()[-1])
                for P, v in one.items():
                    figs[k][P].append(round(v, 4))
        name = "%d slots (%d rows)" % (S, 2 * S)
        res["ms_per_step"][name] = figs
        print(name, json.dumps(figs), flush=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def merge(out, parts):
    res = None
    for fn in parts:
        d = json.load(open(fn))
        if res is None:
            res = d
            continue
        for name, kinds in d["ms_per_step"].items():
            for k, by_pos in kinds.items():
                for P, v in by_pos.items():
                    res["ms_per_step"].setdefault(name, {}).setdefault(k, {}).setdefault(P, []).extend(v)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def report(files):
    def mmm(v):
        return "%.4f / %.4f / %.4f" % (min(v), statistics.median(v), max(v)) if v else "-"
    for fn in files:
        d = json.load(open(fn))
        print(fn, "(%s)" % d["shapes"])
        for name, kinds in d["ms_per_step"].items():
            for k, by_pos in kinds.items():
                for P, v in by_pos.items():
                    print("  %-20s %-7s position %-5s %s ms per step" % (name, k, P, mmm(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--kv", default="f32,f16", help="cache types to measure (f16 is dropped on a tree without kv_type)")
    ap.add_argument("--slots", default="4,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg", help="internal: run one leg in this process and print its JSON line")
    ap.add_argument("--report", nargs="+", metavar="FILE")
    ap.add_argument("--merge", nargs="+", metavar="FILE", help="OUT PART...: join the repetitions of several runs")
    args = ap.parse_args()
    if args.report:
        return report(args.report)
    if args.merge:
        return merge(args.merge[0], args.merge[1:])
    if args.leg:
        print(json.dumps(leg(args.leg, int(args.slots))))
        return
    measure(args)


if __name__ == "__main__":
    main()
