"""The raw bits behind profiles/attn_kv_unify.json: what the Llama / Dia attention kernels and cache writers leave, for comparing two builds of the tree.

One invocation is one process on one tree: like the bench files here it imports tts_cpp_amd — and the three GPU attention test files, whose case tables it
drives — from the WORKING DIRECTORY, so the same file runs against any built checkout:

    (cd PARENT_CHECKOUT && python THIS_FILE --out parent.npz)
    (cd THIS_CHECKOUT   && python THIS_FILE --out new.npz)
    python THIS_FILE --compare parent.npz new.npz
(--one-layer records, in the same format, ORPHEUS_CALLS on a one-layer model over the fp16 cache: every launch of the plain fp16 wave kernel on inputs that
do not depend on an earlier attention output.)

Nothing is restated: the checkers of tests/test_gpu_llama_attention.py and tests/test_gpu_dia_kv_f16.py (_check) are replaced by a recorder, and the files' own
drivers run their own tables with their own fixed seeds —
  fp32 cache   ORPHEUS_CALLS at attn_wave 1 and 0, the captured step and the lock-step rows of test_gpu_llama_attention, its DIA_CASES;
  fp16 cache   the same tables through tests/test_gpu_orpheus_kv_f16.py, and CASES of tests/test_gpu_dia_kv_f16.py.
The recorder keeps, per checker call, the attention output rows (the engine read them back through tts_hip_debug_read) and, per cache, the K / V rows up to
the last key any row read — the rows the writers appended — as uint32 bit patterns."""
import argparse
import itertools
import json
import os
import sys
import zlib

import numpy as np


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def record(out_path):
    root = os.getcwd()
    for p in (os.path.join(root, "oracle"), os.path.join(root, "tests"), root):
        sys.path.insert(0, p)
    import test_gpu_dia_kv_f16 as td
    import test_gpu_llama_attention as ta
    import test_gpu_orpheus_kv_f16 as tk

    arrays, same_as, first, group, calls = {}, {}, {}, ["?"], [0]

    def put(name, a):
        """rows met before (a cross cache is read again at every step) are stored once: same_as names the first array with these bits"""
        b = _bits(a)
        h = (b.shape, zlib.crc32(b.tobytes()))
        if h in first and np.array_equal(arrays[first[h]], b):
            same_as[name] = first[h]
        else:
            first[h] = name
            arrays[name] = b

    def keep(tag, out, rows):
        """the recorder behind both _check signatures"""
        calls[0] += 1
        key = f"{group[0]}/{tag}"
        assert key + "/out" not in arrays, key
        arrays[key + "/out"] = _bits(out).reshape(len(rows), -1)
        caches = {}
        for T, K, V in rows:
            caches[(id(K), id(V))] = (max(T, caches.get((id(K), id(V)), (0,))[0]), K, V)
        for i, (T, K, V) in enumerate(caches.values()):
            put(f"{key}/K{i}", K[:T])
            put(f"{key}/V{i}", V[:T])

    def ta_check(tag, kernel, nz, Q, out, rows, scale, nkv, log, sharp_rows=None):
        keep(tag, out, rows)
        log.append(dict(tag=tag, kernel=kernel, nz=nz, keys=(min(t for t, _, _ in rows), max(t for t, _, _ in rows))))

    def td_check(tag, kernel, nz, Q, out, rows, nkv, log, sharp_rows=None):
        keep(tag, out, rows)
        log.append(dict(tag=tag, kernel=kernel, nz=nz))

    ta._check, td._check = ta_check, td_check

    def each(fn):
        """a parametrised test run over the product of its own parametrize marks"""
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        names = [[n.strip() for n in m.args[0].split(",")] for m in marks]
        for combo in itertools.product(*[m.args[1] for m in marks]):
            kw = {}
            for ns, vals in zip(names, combo):
                kw.update(zip(ns, vals if len(ns) > 1 else (vals,)))
            fn(**kw)

    group[0] = "f32"
    for wave in (1, 0):
        assert not ta._orpheus_sequence(wave)[2]
    each(ta.test_orpheus_captured_step)
    ta.test_orpheus_lockstep_rows_with_their_own_slots()
    for case in ta.DIA_CASES:
        assert not ta._dia_run(*case)[2]
    group[0] = "f16"
    for wave in (1, 0):
        assert not tk._sequence(wave)[1]
    each(tk.test_f16_cache_captured_step)
    tk.test_f16_cache_lockstep_rows_with_their_own_slots()
    for case in td.CASES:
        assert not td._run(*case)[2]
    np.savez(out_path, same_as=np.array(json.dumps(same_as, sort_keys=True)), **arrays)
    print(json.dumps({"checker_calls": calls[0], "arrays": len(arrays), "stored_once": len(same_as), "out": out_path}))


def record_one_layer(out_path):
    """The plain fp16 wave kernel alone: ORPHEUS_CALLS on a ONE-layer model over the fp16 cache.  Layer 0's query and K / V rows come from the embeddings, so no
    launch reads anything an earlier attention output reached, and two builds with bit-identical writers hand every launch identical inputs."""
    root = os.getcwd()
    for p in (os.path.join(root, "oracle"), os.path.join(root, "tests"), root):
        sys.path.insert(0, p)
    import test_gpu_llama_attention as ta
    from tts_cpp_amd import hip, synth

    model = synth.build_orpheus(synth.orpheus_tiny(hidden=512, heads=ta.NH, kv_heads=ta.NKV, layers=1, vocab=ta.VOCAB, ctx=ta.CTX))
    ids = ta._orpheus_ids()
    eng = hip.OrpheusEngine(model.cfg, flags=hip.FLAG_KV_F16)
    eng.load(model)
    arrays = {}
    for p0, n in ta.ORPHEUS_CALLS:
        eng.decode(ids[p0:p0 + n], p0)
        nz = ta._plan(n, p0 + n)
        arrays[f"f16/one layer {'unsplit' if nz == 1 else 'wave'} nz={nz} pos {p0}..{p0 + n - 1}/out"] = _bits(eng.debug_read("l_att", n * ta.A)).reshape(n, -1)
    eng.close()
    np.savez(out_path, same_as=np.array("{}"), **arrays)
    print(json.dumps({"checker_calls": len(arrays), "arrays": len(arrays), "out": out_path}))


def _load(path):
    """{name: array}, the arrays stored once under every name they were recorded under"""
    n = np.load(path)
    out = {k: n[k] for k in n.files if k != "same_as"}
    out.update({k: out[v] for k, v in json.loads(str(n["same_as"])).items()})
    return out


def compare(a_path, b_path):
    a, b = _load(a_path), _load(b_path)
    assert sorted(a) == sorted(b), "the two runs recorded different cases"
    rep = {"cases": sum(1 for k in a if k.endswith("/out")), "arrays": len(a), "differing": {}, "crc32": {}}
    for k in sorted(a):
        x, y = a[k], b[k]
        crc = [zlib.crc32(v.tobytes()) & 0xFFFFFFFF for v in (x, y)]
        if k.endswith("/out"):
            rep["crc32"][k] = f"{crc[0]:08x}"
        if x.shape != y.shape or not np.array_equal(x, y):
            # distance in units in the last place of the fp32 patterns (sign-magnitude -> a monotone integer line)
            line = lambda u: np.where(u >> 31, -(u & 0x7FFFFFFF).astype(np.int64), (u & 0x7FFFFFFF).astype(np.int64))  # noqa: E731
            ulps = int(np.abs(line(x) - line(y)).max()) if x.shape == y.shape else -1
            rep["differing"][k] = {"crc32": [f"{c:08x}" for c in crc], "words": int((x != y).sum()) if x.shape == y.shape else -1, "max_ulps": ulps}
    # per group: one CRC over every array of the group in key order (K / V rows included)
    def crc_all(n, g):
        c = 0
        for k in sorted(n):
            if k.startswith(g + "/"):
                c = zlib.crc32(n[k].tobytes(), c)
        return f"{c & 0xFFFFFFFF:08x}"

    for g in ("f32", "f16"):
        rep[f"crc32_all_{g}"] = [crc_all(n, g) for n in (a, b)]
    rep["verdict"] = "bit-identical" if not rep["differing"] else "differs"
    print(json.dumps(rep, indent=1))
    return 0 if not rep["differing"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--one-layer", action="store_true", help="record the one-layer run (the plain fp16 wave kernel on identical inputs) instead of the case tables")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.one_layer:
        sys.exit(record_one_layer(args.out or "attn_kv_bits_one_layer.npz"))
    record(args.out or "attn_kv_bits.npz")
