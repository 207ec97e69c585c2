"""The measurement behind profiles/orpheus_one_loop.json / orpheus_one_loop_parent_before.json: the Orpheus lock-step loop of a commit against
its parent commit, at the shapes of orpheus_stream_bench.py (Orpheus-3B Q4_0, 32-id prompts, 56 timed steps after 8; ragged mix of 24 utterances
of 40 .. 400 ids at 8 slots, lengths set by the end of a cache of 448 positions).

One invocation is one process on one tree: it imports tts_cpp_amd from the WORKING DIRECTORY, so the same file measures any built checkout:

    (cd PARENT_CHECKOUT && python THIS_FILE --out parent_1.json --ids parent_ids_1.json)
    (cd THIS_CHECKOUT   && python THIS_FILE --out new_1.json --ids new_ids_1.json --runlens 7,14,28,56 --against parent_ids_1.json)

Alternate the two within one session on one GPU, at least three pairs, in both orders; the parent's own runs give its spread between processes.
A leg passes when this commit's median lies inside the parent's min .. max over its runs, or below it (`--report` prints that per leg).

  legs   stream_run and gen_launch, ms per step, at 8 and 32 rows, greedy and sampled (top_k 50); the uniform sampled session again after the
         gen_launch legs (leg (a) of orpheus_stream_bench.py --mixed); the ragged mix as three generate_batch groups — with --runlens once per
         run length of generate_batch (tune("orpheus_batch_run"); a tree without that key takes no --runlens) — and as one session
  ids    --ids saves the ragged mix's ids; --against counts the utterances whose ids equal the generate_batch ids saved by another run
  --no-ragged   the per-step legs only

    python THIS_FILE --report parent_*.json -- new_*.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

NO_STOP = 0xFFFFFFFF
SMP = dict(top_k=50, temperature=1.0, repetition_penalty=1.0, top_p=1.0)
STEPS, WARM = 56, 8
LOOK_IN = 28
N_RAGGED, SLOTS, CAP = 24, 8, 512
RAGGED_CTX = 448
RAGGED_LENGTHS = [40, 400, 120, 60, 280, 80, 200, 48, 360, 100, 160, 44, 240, 72, 320, 56, 140, 400, 90, 180, 52, 300, 64, 220]


def r4(v):
    return [round(float(x), 4) for x in v]


def session_steps(eng, B, prompts, uni, sampled, reps):
    out = []
    for _ in range(reps):
        eng.stream_begin(B, WARM + STEPS + 2, NO_STOP, sampled=sampled, **SMP)
        eng.stream_admit(list(range(B)), prompts, uni if sampled else None)
        assert eng.stream_run(WARM) == []
        t = time.perf_counter()
        fin = eng.stream_run(STEPS)
        out.append((time.perf_counter() - t) / STEPS * 1e3)
        assert fin == []
        eng.stream_end()
    return r4(out)


def batch_steps(eng, prompts, uni, sampled, reps):
    kw = dict(uniforms=uni[:, :WARM + STEPS + 1], **SMP) if sampled else {}
    out = []
    for _ in range(reps):
        eng.gen_begin(prompts, WARM + STEPS + 1, NO_STOP, **kw)
        eng.gen_launch(WARM)
        eng.gen_wait()
        t = time.perf_counter()
        eng.gen_launch(STEPS)
        eng.gen_wait()
        out.append((time.perf_counter() - t) / STEPS * 1e3)
        eng.gen_launch(1)
        assert all(eng.gen_wait()[1])
    return r4(out)


def groups(eng, prompts):
    got = []
    for g0 in range(0, N_RAGGED, SLOTS):
        got += [ids.tolist() for ids in eng.generate_batch(prompts[g0:g0 + SLOTS], CAP, NO_STOP)]
    return got


def session(eng, prompts):
    eng.stream_begin(SLOTS, CAP, NO_STOP)
    free, slot_utt, out, nxt = list(range(SLOTS)), {}, [None] * N_RAGGED, 0
    while nxt < N_RAGGED or slot_utt:
        while nxt < N_RAGGED and free:
            s = free.pop(0)
            eng.stream_admit([s], [prompts[nxt]])
            slot_utt[s] = nxt
            nxt += 1
        for s, cnt in eng.stream_run(LOOK_IN):
            out[slot_utt.pop(s)] = eng.stream_collect(s, cnt).tolist()
            free.append(s)
    eng.stream_end()
    return out


def timed(fn, reps):
    ts, got = [], None
    for _ in range(reps):
        t = time.perf_counter()
        got = fn()
        ts.append(time.perf_counter() - t)
    return r4(ts), got


def measure(args):
    root = os.getcwd()
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "profiles"))
    import tts_cpp_amd  # noqa: F401
    from tts_cpp_amd import gguf, hip, synth
    import secondary_bench as sb
    assert os.path.dirname(os.path.abspath(hip.__file__)).startswith(root), hip.__file__
    res = {"per_step": {}, "mixed_a_uniform_sampled": {}, "ragged": {}}
    cfg = synth.orpheus_3b(ctx=1024, weight_type=gguf.Q4_0)
    tensors, _ = sb.orpheus_tensors(cfg, np.random.default_rng(7))
    model = sb._Model(cfg, tensors)
    prng = np.random.default_rng(11)
    for B in [int(x) for x in args.rows.split(",")]:
        eng = hip.OrpheusEngine(cfg, max_seqs=B)
        eng.load(model)
        prompts = [prng.integers(0, cfg.vocab, 32).astype(np.uint32) for _ in range(B)]
        uni = prng.random((B, WARM + STEPS + 2), dtype=np.float32)
        eng.generate_batch(prompts, 4, NO_STOP)
        res["per_step"][str(B)] = {}
        for mode in ("greedy", "sampled"):   # the session first: its history in the process is then the same in both trees
            run = session_steps(eng, B, prompts, uni, mode == "sampled", args.reps)
            gen = batch_steps(eng, prompts, uni, mode == "sampled", args.reps)
            res["per_step"][str(B)][mode] = {"gen_launch_ms_per_step": gen, "stream_run_ms_per_step": run}
        res["mixed_a_uniform_sampled"][str(B)] = session_steps(eng, B, prompts, uni, True, args.reps)
        print(B, json.dumps(res["per_step"][str(B)]), "mixed (a)", res["mixed_a_uniform_sampled"][str(B)], flush=True)
        eng.close()
    ids = {}
    if not args.no_ragged:
        cfg2 = synth.orpheus_3b(ctx=RAGGED_CTX, weight_type=gguf.Q4_0)
        eng = hip.OrpheusEngine(cfg2, max_seqs=SLOTS)
        eng.load(sb._Model(cfg2, tensors))
        rp = [np.random.default_rng(100 + i).integers(0, cfg.vocab, RAGGED_CTX + 1 - n).astype(np.uint32) for i, n in enumerate(RAGGED_LENGTHS)]
        groups(eng, rp[:SLOTS] * 3)   # warm-up
        for rl in [int(x) for x in args.runlens.split(",")] if args.runlens else [None]:
            if rl is not None:
                eng.tune("orpheus_batch_run", rl)
            name = "groups" if rl is None else "groups_run_%d" % rl
            res["ragged"]["generate_batch_" + name.replace("groups", "groups_s")], ids[name] = timed(lambda: groups(eng, rp), args.reps)
            assert [len(g) for g in ids[name]] == RAGGED_LENGTHS
            print("ragged", name, res["ragged"]["generate_batch_" + name.replace("groups", "groups_s")], flush=True)
        res["ragged"]["session_s"], ids["session"] = timed(lambda: session(eng, rp), args.reps)
        print("ragged session", res["ragged"]["session_s"], flush=True)
        eng.close()
        if args.against:
            ref = json.load(open(args.against))
            ref = ref.get("groups") or next(v for k, v in ref.items() if k.startswith("groups"))
            res["ragged"]["utterances_with_the_other_runs_generate_batch_ids"] = {k: sum(a == b for a, b in zip(v, ref)) for k, v in ids.items()}
            print("ids", res["ragged"]["utterances_with_the_other_runs_generate_batch_ids"], flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    if args.ids and ids:
        with open(args.ids, "w") as f:
            json.dump(ids, f)


def flatten(files):
    """{leg: every run of every process}"""
    legs = {}
    for fn in files:
        d = json.load(open(fn))
        for B, modes in d["per_step"].items():
            for mode, v in modes.items():
                for k, runs in v.items():
                    legs.setdefault("%s, %s rows %s" % (k, B, mode), []).extend(runs)
        for B, runs in d["mixed_a_uniform_sampled"].items():
            legs.setdefault("--mixed leg (a), %s rows" % B, []).extend(runs)
        for k, runs in d["ragged"].items():
            if isinstance(runs, list):
                legs.setdefault("ragged " + k, []).extend(runs)
    return legs


def report(parent_files, new_files):
    par, new = flatten(parent_files), flatten(new_files)
    for k, v in new.items():
        p = par.get(k) or (par.get("ragged generate_batch_groups_s") if k.startswith("ragged generate_batch_groups_s_run_") else None)
        if not p:
            continue
        m = statistics.median(v)
        print("%-50s parent %.4f / %.4f / %.4f (%d runs)  this commit %.4f (%d runs)  %s" % (k, min(p), statistics.median(p), max(p), len(p), m, len(v),
              "under" if m < min(p) else "inside" if m <= max(p) else "ABOVE the parent's slowest run by %.2f %%" % ((m / max(p) - 1) * 100)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--ids", help="where the ragged mix's ids go (generate_batch groups and session)")
    ap.add_argument("--against", help="ids file of another run: count the utterances with its generate_batch ids")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default="8,32")
    ap.add_argument("--runlens", default="", help="comma list: generate_batch's run length (tune orpheus_batch_run)")
    ap.add_argument("--no-ragged", action="store_true")
    ap.add_argument("--report", nargs="+", metavar="FILE", help="parent files, then --, then this commit's files")
    args, rest = ap.parse_known_args()
    if args.report:
        return report(args.report, [r for r in rest if r != "--"])
    measure(args)


if __name__ == "__main__":
    main()
