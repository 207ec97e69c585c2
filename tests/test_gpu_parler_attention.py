"""GPU: Parler's attention kernels (csrc/parler_kernels.h: attn_kernel in its 256- and 1024-thread forms, its key-sliced form with the fold by the last
workgroup, attn_combine_kernel, attn_rows_kernel<8> with four slices and with one, attn_short_kernel) past their first key pass and their first slice,
up to 1041 cached keys, against a float64 softmax . V (tests/attn_reference.py, head width 64) of what the launch itself read: the query rows, the rows'
positions and cache slots, the cache rows and the output rows are fetched back from the device (tts_hip_debug_read "q", "pos", "seq", "k:", "v:",
"cross:", "att", "att16", "part:<nz>"), so nothing but the attention is between the two numbers.  Reading them switches nothing (tts_hip_set_debug would).

Every launch goes through one checker (_check), every row and head of it:
  fp32 rows ("att", and the float64 fold of the slices "part" holds when the out projection folds them): max|out - ref| / max|ref| < BAR;
  fp16 rows ("att16"): per element |out - ref| <= 2^-11 |ref| + 2^-25 + BAR max|ref| — round-to-nearest fp16 of a value within BAR of the reference;
  T = 1: the row is V[0] within the same bar.

BAR = min(4 x F32_WORST, 1e-5), the recipe of tests/test_gpu_llama_attention.py: F32_WORST is the worst distance, over every row of this file, of the
same formula evaluated in numpy float32 on the tensors read back (1.79e-6, measured on the MI355X run recorded in DESIGN.md, printed per launch under -s),
so BAR = 7.16e-6; the margin of 4 is for the kernels' other, equally legitimate summation orders and for expf.  Measured kernel distances over the 306
launches of the file: 1.0e-7 .. 6.4e-7 for fp32 rows, 3.6e-4 .. 4.8e-4 (the fp16 rounding) for fp16 rows.

Sharpness (a condition on the reference alone, asserted for every checked row with more than one key): removing any one of the boundary keys
{0, NKG - 1, NKG, pass - 1, pass, chunk - 1, chunk, T - 1} of the row (_edges: the geometry of the kernel the launch took) moves the float64 reference by
at least 10 x BAR (fp32 rows) or 10 x (2^-11 + BAR) (fp16 rows), so one dropped, duplicated or stale key cannot pass (measured: 1.3e-2 at the least).
tests/test_attn_reference_cpu.py holds the same condition against the oracle's cache rows of the same model and ids.

The model is synth.tiny widened to 1048 positions and 5001 prompt ids (hidden 256, 4 heads of 64, 2 layers; _model says what else differs); the last layer is read.  Caches are filled
by ascending prefill pieces and steps, each of them a checked launch.  The kernel, the slice count and the output buffer of a launch are restated from
attn_nsplit / run_attn / enqueue_forward (_plan) and asserted against the table of the case, so a change of the dispatch shows up here and not as a
silently untested kernel."""
import functools

import numpy as np
import pytest

import attn_reference as ar
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

F32_WORST = 1.79e-6         # measured: the 7-row piece at positions 1032 .. 1038 of the 8-slice table (DESIGN.md lists every case)
BAR = min(4 * F32_WORST, 1e-5)
SHARP32 = 10 * BAR
SHARP16 = 10 * (2.0 ** -11 + BAR)
NH, HD = 4, 64
H = NH * HD
SCALE = 0.125               # 1 / sqrtf(64)
CTX = 1048                  # positions 0 .. 1040 are used: 1041 keys at the most
PV = 5001
KV_IDS = {gguf.F32: "kv32", gguf.F16: "kv16"}


@functools.lru_cache(maxsize=None)
def _model(wtype):
    """synth.tiny at 1048 positions and 5001 prompt ids, its prompt embedding a hundred times as large (std 2): the table then outweighs the positional embedding
    (amplitude 0.02, half of whose channels hardly move with the position), whose common part otherwise makes the V rows of a cache near copies of their mean —
    at 1040 keys dropping one would move a row by 4e-3 of its maximum, below what an fp16 row can show (2e-2 with this table)"""
    m = synth.build(synth.tiny(ctx=CTX, prompt_vocab=PV, weight_type=wtype))
    t = m.by_name["decoder.embed_prompts"]
    t2 = gguf.Tensor.from_array(t.name, (t.to_f32().reshape(PV, H) * np.float32(100.0)).astype(np.float32), t.type)
    m.tensors[[x.name for x in m.tensors].index(t.name)] = t2
    m.by_name[t.name] = t2
    return m


@functools.lru_cache(maxsize=None)
def _ids(n_seqs):
    """prompt ids [n_seqs][CTX] and audio ids [n_seqs][n_out]"""
    rng = np.random.default_rng(0x9A71)
    cfg = _model(gguf.F32).cfg
    return rng.integers(3, PV, (n_seqs, CTX)).astype(np.uint32), rng.integers(0, cfg.audio_vocab, (n_seqs, cfg.n_out)).astype(np.uint32)


def _plan(R, f16w, override=0, fused=True, cross_E=0, short=True):
    """-> (kernel, slices, output buffer) of the last attention launch of a forward of R rows: attn_nsplit, run_attn and enqueue_forward restated.
    f16w: fp16 matrices (the out projection reads fp16 rows; up to 4 rows it folds the slices itself)"""
    if cross_E:
        return ("short" if cross_E <= 32 and short else "attn256", 1, "att")
    out = "att16" if f16w else "att"
    nz = min(override, 16) if override > 0 else (8 if fused and R * NH <= 64 else 1)
    if nz == 1:
        if R >= 256:
            return "rows", (1 if R >= 1024 else 4), out
        return ("attn1024" if NH * R < 128 else "attn256"), 1, out
    if R <= 4 and f16w:
        return "defer", nz, "part"
    return ("fused" if fused else "combine"), nz, out


def _edges(kernel, nz, T):
    """the keys next to a key-group, pass or slice edge: attn_kernel has NKG = threads / 16 key groups and passes of 4 NKG keys, attn_rows_kernel<8> passes of
    8 keys in order, attn_short_kernel 8 / 16 / 32 register slots; slices are ceil(T / nz) keys"""
    chunk = -(-T // nz)
    if kernel == "short":
        return (7, 8, 15, 16)
    if kernel == "rows":
        return (7, 8, chunk - 1, chunk)
    nkg = 64 if kernel == "attn1024" else 16
    return (nkg - 1, nkg, 4 * nkg - 1, 4 * nkg, chunk - 1, chunk)


def _check(tag, kernel, nz, output, Q, out, rows, log):
    """rows: per row (T, key of its cache, K, V) — K / V the cache rows [>= T][H] that row read.  Rows of one cache are evaluated together."""
    R = len(rows)
    Q, out = np.asarray(Q).reshape(R, H), np.asarray(out, dtype=np.float64).reshape(R, H)
    half = output == "att16"
    sharp_bar = SHARP16 if half else SHARP32
    groups = {}
    for r, row in enumerate(rows):
        groups.setdefault(row[1], []).append(r)
    Ts_all = [row[0] for row in rows]
    worst = dict(tag=tag, kernel=kernel, nz=nz, output=output, rows=R, keys=(min(Ts_all), max(Ts_all)), kd=0.0, f32=0.0, sharp=np.inf)
    bad, blunt = [], []
    for rs in groups.values():
        K, V = rows[rs[0]][2], rows[rs[0]][3]
        Ts = [rows[r][0] for r in rs]
        ref = ar.attention_rows(Q[rs], K, V, Ts, SCALE, NH, NH, hd=HD)
        f32 = ar.attention_rows(Q[rs], K, V, Ts, SCALE, NH, NH, dtype=np.float32, hd=HD)
        shifts = ar.drop_shifts(Q[rs], K, V, Ts, SCALE, NH, NH, lambda i, T: ar.edge_keys(T, _edges(kernel, nz, T)) if T > 1 else [], hd=HD)
        for i, r in enumerate(rs):
            for h in range(NH):
                sl = slice(h * HD, (h + 1) * HD)
                den = np.abs(ref[i, sl]).max()
                err = np.abs(out[r, sl] - ref[i, sl])
                kd = float(err.max() / den)
                kd = kd if np.isfinite(kd) else np.inf      # a NaN row must show in the worst distance, not vanish in max()
                worst["kd"] = max(worst["kd"], kd)
                worst["f32"] = max(worst["f32"], float(np.abs(f32[i, sl] - ref[i, sl]).max() / den))
                ok = bool((err <= 2.0 ** -11 * np.abs(ref[i, sl]) + 2.0 ** -25 + BAR * den).all()) if half else kd < BAR
                if Ts[i] == 1:       # one key: the row is V[0]
                    ok = ok and np.array_equal(ref[i, sl], np.asarray(V[0, sl], dtype=np.float64))
                if not ok:
                    bad.append((r, h, Ts[i], kd))
            if shifts[i]:
                j, s = min(shifts[i].items(), key=lambda kv: kv[1])
                worst["sharp"] = min(worst["sharp"], s)
                if not s >= sharp_bar:
                    blunt.append((r, Ts[i], j, s))
    print(f"[pattn] {tag:<40s} {kernel:<8s} nz={nz:<2d} {output:<5s} rows={R:<4d} keys={worst['keys'][0]}..{worst['keys'][1]}  kernel {worst['kd']:.2e}"
          f"  float32 {worst['f32']:.2e}  least boundary key {worst['sharp']:.2e}")
    log.append(worst)
    assert not blunt, f"{tag}: dropping a boundary key moves the reference by less than {sharp_bar:.1e} at (row, keys, key, shift) {blunt[:6]}: change the ids / seed"
    assert not bad, (f"{tag} ({kernel}, nz={nz}, {output}): outside the bar ({'fp16 rounding of ' if half else ''}{BAR:.1e}) at (row, head, keys, max distance) "
                     f"{bad[:6]}{' ...' if len(bad) > 6 else ''}")


def _fetch_and_check(eng, tag, plan, want_pos, want_seq, log, failures, cross_E=0):
    """the last attention launch of the forward that just ran: what it read, what it wrote, the check"""
    kernel, nz, output = plan
    R, L = len(want_pos), eng.cfg.layers
    q = eng.debug_read("q", R * H).reshape(R, H)
    if output == "part":   # no attention row exists in memory: the out projection folds the slices
        p = eng.debug_read(f"part:{nz}", R * NH * nz * 66).reshape(R, NH, nz, 66)
        out = np.stack([np.concatenate([ar.fold_partials(p[r, h, :, 0], p[r, h, :, 1], p[r, h, :, 2:]) for h in range(NH)]) for r in range(R)])
    else:
        out = eng.debug_read(output, R * H).reshape(R, H)
    if cross_E:
        K, V = (eng.debug_read(f"cross:{L - 1}:{i}", cross_E * H).reshape(cross_E, H) for i in (0, 1))
        rows = [(cross_E, 0, K, V)] * R
    else:
        pos, seq = (eng.debug_read(w, R).astype(np.int64) for w in ("pos", "seq"))
        assert pos.tolist() == list(want_pos) and seq.tolist() == list(want_seq), tag
        need = {}
        for p_, s_ in zip(want_pos, want_seq):
            need[s_] = max(need.get(s_, 0), p_ + 1)
        cache = {s_: tuple(eng.debug_read(f"{w}:{L - 1}:{s_}", n * H).reshape(n, H) for w in "kv") for s_, n in need.items()}
        rows = [(p_ + 1, s_) + cache[s_] for p_, s_ in zip(want_pos, want_seq)]
        if nz > 1:   # the slices' markers: -inf exactly where a slice holds no key
            m = eng.debug_read(f"part:{nz}", R * NH * nz * 66).reshape(R, NH, nz, 66)[:, :, :, 0]
            for r, p_ in enumerate(want_pos):
                chunk = -(-(p_ + 1) // nz)
                assert (np.isneginf(m[r]) == (np.arange(nz) * chunk >= p_ + 1)[None, :]).all(), (tag, r, p_ + 1, m[r].tolist())
    try:
        _check(tag, kernel, nz, output, q, out, rows, log)
    except AssertionError as e:      # go on: the later launches read caches this one did not write wrongly (the attention rows feed only later layers' inputs)
        failures.append(str(e))


def _engine(wtype, kv, max_seqs, kv_positions=CTX, override=0, fused=True, cross=False, monkeypatch=None, tune=None):
    model = _model(wtype)
    if override:
        monkeypatch.setenv("TTS_HIP_ATTN_NSPLIT", str(override))      # read when the context is created
    else:
        monkeypatch.delenv("TTS_HIP_ATTN_NSPLIT", raising=False)
    monkeypatch.delenv("TTS_HIP_ATTN_ROWS", raising=False)
    eng = hip.HipEngine(model.cfg, max_seqs=max_seqs, kv_type=kv, use_cross_attn=cross, kv_positions=kv_positions, tune=dict(tune or {}, **({} if fused else {"attn_fused": 0})))
    monkeypatch.delenv("TTS_HIP_ATTN_NSPLIT", raising=False)
    eng.load(model)
    return eng


def _run_calls(eng, calls, col, f16w, override, fused, tag):
    """calls: ("p", seq, first position, rows, want...) a prefill piece, ("s", [(seq, position), ...], want...) a step; want[col] = (kernel, slices)"""
    n_seqs = 1 + max(max(c[1] if c[0] == "p" else max(s for s, _ in c[1]) for c in calls), 0)
    ids, audio = _ids(16 if n_seqs <= 16 else n_seqs)
    log, failures = [], []
    for c in calls:
        if c[0] == "p":
            _, s, p0, n = c[:4]
            eng.prefill(s, ids[s, p0:p0 + n], p0)
            want_pos, want_seq, name, want = range(p0, p0 + n), [s] * n, f"piece seq {s} pos {p0}..{p0 + n - 1}", c[4:]
        else:
            want_seq, want_pos = [s for s, _ in c[1]], [p for _, p in c[1]]
            lg = eng.step(audio[want_seq], want_pos, want_seq)
            assert np.isfinite(lg).all()
            name, want = f"step {len(want_pos)} rows", c[2:]
        plan = _plan(len(want_pos), f16w, override, fused)
        assert plan[:2] == want[min(col, len(want) - 1)], (name, plan)
        _fetch_and_check(eng, f"{tag} {name}", plan, want_pos, want_seq, log, failures)
    assert not failures, "\n".join(failures)
    return log


# --------------------------------------------------------------------------------------------------------------------------------------------
# self-attention, one kernel form per table.  U / W: attn_kernel unsplit with 256 / 1024 threads; F: 8 slices, folded by the last workgroup;
# D: 8 slices left for the out projection (fp16 matrices, up to 4 rows)
# --------------------------------------------------------------------------------------------------------------------------------------------
U, W, F, D = ("attn256", 1), ("attn1024", 1), ("fused", 8), ("defer", 8)

# 32 .. 255 rows: the 255 rows at positions 0 .. 254 hold T = 1, 15, 16, 17 (the key groups), 63, 64, 65 (the first pass), 128, 129; the later pieces reach 1040
CALLS_256 = [("p", 0, 0, 255, U), ("p", 0, 255, 40, U), ("p", 0, 295, 255, U), ("p", 0, 550, 255, U), ("p", 0, 805, 203, U), ("p", 0, 1008, 32, U)]
# 17 .. 31 rows (64 key groups, passes of 256 keys): T across 63 / 64 / 65, 255 / 256 / 257, 512 / 513, and a piece that ends at 1040
CALLS_1024 = [("p", 0, 0, 40, U), ("p", 0, 40, 31, W), ("p", 0, 71, 170, U), ("p", 0, 241, 20, W), ("p", 0, 261, 240, U), ("p", 0, 501, 17, W), ("p", 0, 518, 255, U),
              ("p", 0, 773, 240, U), ("p", 0, 1013, 27, W)]
# up to 16 rows: 8 slices.  T = 1, 2, 7, 8, 9 (empty slices); chunk 16 -> 17 at T = 128, 129, 136, 137; 64 -> 65 at 512, 513, 520, 521; 130 at 1040; long and
# short rows in one launch (the steps).  Second column: fp16 matrices — up to 4 rows the slices stay in `part`, 5 .. 16 rows leave fp16 rows
CALLS_SLICED = [("p", 0, 0, 1, F, D), ("p", 0, 1, 1, F, D), ("p", 0, 2, 3, F, D), ("p", 0, 5, 1, F, D), ("p", 0, 6, 3, F, D), ("p", 0, 9, 16, F), ("p", 0, 25, 20, W),
                ("p", 0, 45, 82, U), ("p", 0, 127, 3, F, D), ("p", 0, 130, 5, F), ("p", 0, 135, 3, F, D), ("p", 0, 138, 255, U), ("p", 0, 393, 118, U), ("p", 0, 511, 3, F, D),
                ("p", 0, 514, 5, F), ("p", 0, 519, 3, F, D), ("p", 0, 522, 255, U), ("p", 0, 777, 255, U), ("p", 0, 1032, 7, F), ("p", 0, 1039, 1, F, D),
                ("p", 1, 0, 1, F, D), ("p", 2, 0, 6, F), ("p", 3, 0, 7, F), ("p", 4, 0, 20, W),
                ("s", [(0, 1039)], F, D), ("s", [(0, 1039), (1, 1), (2, 6), (3, 7)], F, D), ("s", [(0, 1039), (1, 1), (2, 6), (3, 7), (4, 20)], F),
                ("s", [(0, 1039), (1, 1), (2, 6), (3, 7), (4, 20)] + [(s, 0) for s in range(5, 16)], F)]
# TTS_HIP_ATTN_NSPLIT: every row count takes the sliced kernel; T < nz at the first pieces
CALLS_NSPLIT = [("p", 0, 0, 1), ("p", 0, 1, 3), ("p", 0, 4, 16), ("p", 0, 20, 40), ("p", 0, 60, 100), ("p", 0, 160, 255), ("p", 0, 415, 255), ("p", 0, 670, 255),
                ("p", 0, 925, 100), ("p", 0, 1025, 15), ("p", 1, 0, 2), ("p", 2, 0, 7), ("s", [(0, 1039), (1, 2), (2, 7), (3, 0)])]


@pytest.mark.parametrize("kv", [gguf.F32, gguf.F16], ids=KV_IDS.get)
@pytest.mark.parametrize("name,calls", [("256-threads", CALLS_256), ("1024-threads", CALLS_1024), ("8-slices", CALLS_SLICED)], ids=["256-threads", "1024-threads", "8-slices"])
def test_self_attention_fp32_rows(name, calls, kv, monkeypatch):
    """fp32 matrices: attn_kernel writes `att` — unsplit with 16 and with 64 key groups, and in 8 slices folded by the workgroup that finishes last"""
    eng = _engine(gguf.F32, kv, 16, monkeypatch=monkeypatch)
    log = _run_calls(eng, calls, 0, False, 0, True, f"f32 {KV_IDS[kv]} {name}")
    eng.close()
    assert len(log) == len(calls) and all(e["output"] == "att" for e in log)
    assert max(e["keys"][1] for e in log) == 1040 and min(e["keys"][0] for e in log) == 1


@pytest.mark.parametrize("kv", [gguf.F32, gguf.F16], ids=KV_IDS.get)
def test_self_attention_fp16_matrices_deferred_fold_and_fp16_rows(kv, monkeypatch):
    """fp16 matrices over the table of the 8-slice case: up to 4 rows the out projection folds the slices (no attention row in memory: `part` folded in float64
    checks the sliced key passes); 5 .. 16 rows: the in-kernel fold writes `att16`; 17 .. 255 rows: the unsplit forms write `att16`"""
    eng = _engine(gguf.F16, kv, 16, monkeypatch=monkeypatch)
    log = _run_calls(eng, CALLS_SLICED, 1, True, 0, True, f"f16 {KV_IDS[kv]} 8-slices")
    eng.close()
    kinds = {(e["kernel"], e["output"]) for e in log}
    assert kinds == {("defer", "part"), ("fused", "att16"), ("attn1024", "att16"), ("attn256", "att16")}


@pytest.mark.parametrize("kv", [gguf.F32, gguf.F16], ids=KV_IDS.get)
@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "combine"])
@pytest.mark.parametrize("nsplit", [4, 16])
def test_self_attention_forced_slice_count(nsplit, fused, kv, monkeypatch):
    """TTS_HIP_ATTN_NSPLIT = 4 and 16 (16 fills the folds' register arrays) at 1 .. 255 rows; tune("attn_fused", 0): attn_combine_kernel folds instead"""
    eng = _engine(gguf.F32, kv, 4, override=nsplit, fused=bool(fused), monkeypatch=monkeypatch)
    want = ("fused" if fused else "combine", nsplit)
    log = _run_calls(eng, [c + (want,) for c in CALLS_NSPLIT], 0, False, nsplit, bool(fused), f"f32 {KV_IDS[kv]} nsplit {nsplit} {'fused' if fused else 'combine'}")
    eng.close()
    assert len(log) == len(CALLS_NSPLIT) and all((e["kernel"], e["nz"], e["output"]) == want + ("att",) for e in log)


# --------------------------------------------------------------------------------------------------------------------------------------------
# attn_rows_kernel<8>: one workgroup per row, every row its own cache slot and length
# --------------------------------------------------------------------------------------------------------------------------------------------
def _rows_case(eng, f16w, Ts, tag):
    """slot r gets a prompt of Ts[r] - 1 ids (one batched prefill: its forwards run the same dispatch, the last of them is checked), then one step of every slot
    at its next position: row r reads Ts[r] keys"""
    n = len(Ts)
    ids, audio = _ids(n)
    prompts = [ids[s, :T - 1] for s, T in enumerate(Ts)]
    eng.prefill_batch(prompts)
    flat = [(s, j) for s, p in enumerate(prompts) for j in range(len(p))]
    rmax = 1024 if f16w else 256
    last = flat[len(flat) - ((len(flat) - 1) % rmax + 1):]
    log, failures = [], []
    _fetch_and_check(eng, f"{tag} last prefill forward", _plan(len(last), f16w), [j for _, j in last], [s for s, _ in last], log, failures)
    lg = eng.step(audio[:n], [T - 1 for T in Ts], list(range(n)))
    assert np.isfinite(lg).all()
    plan = _plan(n, f16w)
    _fetch_and_check(eng, f"{tag} step {n} rows", plan, [T - 1 for T in Ts], list(range(n)), log, failures)
    assert not failures, "\n".join(failures)
    return plan, log


ROWS256_T = (1, 2, 3, 4, 5, 31, 32, 33, 64, 65)          # 1 .. 3: empty slices; 31 .. 33: slices of 8 and 9 keys (one pass, one pass and a key)
ROWS256_LONG = {5: 1040, 77: 1041, 200: 1040, 255: 1041}  # a handful of long rows among the short ones


@pytest.mark.parametrize("kv", [gguf.F32, gguf.F16], ids=KV_IDS.get)
@pytest.mark.parametrize("wtype", [gguf.F32, gguf.F16], ids=["f32", "f16"])
def test_rows_kernel_four_slices_and_combine_at_256_rows(wtype, kv, monkeypatch):
    """256 rows: attn_rows_kernel<8> in four slices + attn_combine_kernel; fp32 matrices (a forward carries 256 rows at the most): `att`, fp16: `att16`"""
    Ts = [ROWS256_LONG.get(r, ROWS256_T[r % len(ROWS256_T)]) for r in range(256)]
    eng = _engine(wtype, kv, 256, monkeypatch=monkeypatch)
    plan, log = _rows_case(eng, wtype == gguf.F16, Ts, f"{'f16' if wtype == gguf.F16 else 'f32'} {KV_IDS[kv]} rows256")
    eng.close()
    assert plan == ("rows", 4, "att16" if wtype == gguf.F16 else "att") and log[-1]["keys"] == (1, 1041)


ROWS1024_T = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 128, 129)


@pytest.mark.parametrize("kv", [gguf.F32, gguf.F16], ids=KV_IDS.get)
def test_rows_kernel_one_slice_at_1024_rows(kv, monkeypatch):
    """1024 rows (fp16 matrices lift the cap of a forward to 1024): attn_rows_kernel<8> over all keys of a row, passes of 8 keys, `att16`"""
    Ts = [ROWS1024_T[(r + r // 12) % len(ROWS1024_T)] for r in range(1024)]
    eng = _engine(gguf.F16, kv, 1024, kv_positions=136, monkeypatch=monkeypatch)
    plan, log = _rows_case(eng, True, Ts, f"f16 {KV_IDS[kv]} rows1024")
    eng.close()
    assert plan == ("rows", 1, "att16") and log[-1]["keys"] == (1, 129)


# --------------------------------------------------------------------------------------------------------------------------------------------
# cross-attention (fp32 matrices: no fold takes it into a GEMM; q and att end the forward holding the last layer's cross-attention)
# --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,short", [(1, 1), (7, 1), (8, 1), (9, 1), (16, 1), (17, 1), (31, 1), (32, 1), (33, 1), (64, 1), (65, 1), (8, 0)])
def test_cross_attention(E, short, monkeypatch):
    """attn_short_kernel with 8 / 16 / 32 register slots at E <= 32 (a slot beyond E re-reads the last row); attn_kernel with T_fixed at E > 32 and, with
    tune("attn_short", 0), at E = 8; forwards of 1, 5, 40 and 256 rows"""
    eng = _engine(gguf.F32, gguf.F32, 1, kv_positions=264, cross=True, monkeypatch=monkeypatch, tune=None if short else {"attn_short": 0})
    enc = (np.random.default_rng(0xC4055 + E).standard_normal((E, H)) * 0.5).astype(np.float32)
    eng.set_text_encoding(enc)
    ids, _ = _ids(16)
    plan = _plan(0, False, cross_E=E, short=bool(short))
    assert plan[0] == ("short" if E <= 32 and short else "attn256")
    log, failures = [], []
    for n in (1, 5, 40, 256):
        eng.prefill(0, ids[1, :n], 0)
        _fetch_and_check(eng, f"cross E={E} short={short} {n} rows", plan, range(n), [0] * n, log, failures, cross_E=E)
    eng.close()
    assert not failures, "\n".join(failures)
    assert len(log) == 4
