"""GPU: the five attention kernels of the Orpheus / Dia steps (csrc/llama_kernels.h: attn_gqa_kernel<128, SPLIT, float> unsplit and split,
attn_gqa_wave_kernel<128, 4, false, float>, its EXT form attn_gqa_wave_kernel<128, 3, true, float>, attn_gqa_combine_kernel) past their first batch of 64 keys, their first round of
64 * nz keys and up to the last cache row, against a float64 softmax . V (tests/attn_reference.py) of what the launch itself read: the rotated query,
the cache rows and the output rows are fetched back from the device (tts_hip_debug_read), so nothing but the attention is between the two numbers.

Every engine call goes through one checker (_check): for every row and head, max|out - ref| / max|ref| < BAR.

BAR: the same formula evaluated in numpy float32 on the tensors read back stays within F32_WORST = 1.61e-6 of float64 over every row of this file
(measured on the MI355X run recorded in DESIGN.md, printed per call under -s); the bar is 4 x that = 6.44e-6 — the kernels sum in other, equally
legitimate orders and use expf — and never above 1e-5.  Measured kernel distances: 1.0e-7 .. 4.3e-7.

Sharpness (a condition on the reference alone, asserted for every checked row): removing any one of the boundary keys {0, 15, 16, 63, 64, Rd - 1, Rd,
T - 1} of the row (Rd: its round or chunk size) moves the float64 reference by at least 10 x BAR, so one dropped, duplicated or stale key cannot pass
(measured: 1.9e-3 at the least, 4.0e-4 on Dia's cross rows).  One kind of row cannot meet it whatever the ids: the unconditional guidance rows of Dia's cross-attention read the
encoding of an all-zero text, whose V rows are copies of one another (dropping a key moves them by 1e-10), so nothing distinguishes their keys; their
distance is checked all the same, the condition is asserted on the conditional rows of the same launch.

The models are tiny (hidden 512, 4 heads on 2 k/v heads, 2 layers, vocabulary 5001 with random ids so that no two keys carry the same V row), the key
counts are the smallest that cross each loop boundary.  The split count nz and the kernel a call takes are restated from launch_attn_gqa (_plan) and
asserted against the table of the case, so a change of the dispatch shows up here and not as a silently untested kernel."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import attn_reference as ar
import oracle as orc
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

F32_WORST = 1.61e-6         # measured: the 255-row piece at positions 0..254 (DESIGN.md lists every call)
BAR = min(4 * F32_WORST, 1e-5)
SHARP = 10 * BAR
NH, NKV, HD = 4, 2, 128
A = NH * HD
VOCAB = 5001


def _powf(x, y):
    """the host's powf (theta_scale is computed with it in float32)"""
    try:
        f = ctypes.CDLL("libm.so.6").powf
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
        return float(f(x, y))
    except OSError:
        return float(np.float32(x) ** np.float32(y))


def _plan(rows, max_keys, split_max=8, cap=4 * NH * 16, fixed=False):
    """launch_attn_gqa's split count"""
    nz = 1
    if split_max > 1 and NH * rows <= 256:
        nz = split_max if fixed else min(split_max, max(1, max_keys // 128))
        while nz > 1 and rows * NH * nz > cap:
            nz -= 1
    return nz


def _round(kernel, nz, T):
    """Rd of a row: the 64-key batch of the unsplit kernel, the slice of the split kernel, the U = 4 passes of 16 nz keys of the wave kernel,
    the U = 3 register slots of 16 nz keys its EXT form re-requests after"""
    return {"unsplit": 64, "split": -(-T // nz), "wave": 64 * nz, "ext": 48 * nz}[kernel]


def _check(tag, kernel, nz, Q, out, rows, scale, nkv, log, sharp_rows=None):
    """rows: per row (T, K, V) — K / V the cache rows [>= T][nkv * HD] that row read.  Rows of one cache are evaluated together.
    sharp_rows: the rows the sharpness condition is asserted on (default: all)"""
    Q, out = np.asarray(Q).reshape(len(rows), A), np.asarray(out).reshape(len(rows), A)
    groups = {}
    for r, (T, K, V) in enumerate(rows):
        groups.setdefault((id(K), id(V)), []).append(r)
    worst = dict(tag=tag, kernel=kernel, nz=nz, rows=len(rows), keys=(min(t for t, _, _ in rows), max(t for t, _, _ in rows)), kd=0.0, f32=0.0, sharp=np.inf)
    bad, blunt = [], []
    for rs in groups.values():
        K, V = rows[rs[0]][1], rows[rs[0]][2]
        Ts = [rows[r][0] for r in rs]
        ref = ar.attention_rows(Q[rs], K, V, Ts, scale, NH, nkv)
        f32 = ar.attention_rows(Q[rs], K, V, Ts, scale, NH, nkv, dtype=np.float32)
        shifts = ar.drop_shifts(Q[rs], K, V, Ts, scale, NH, nkv, lambda i, T: ar.boundary_keys(T, _round(kernel, nz, T)) if T > 1 else [])
        for i, r in enumerate(rs):
            den = np.abs(ref[i]).max()
            kd = float(np.abs(out[r] - ref[i]).max() / den)
            worst["kd"] = max(worst["kd"], kd)
            worst["f32"] = max(worst["f32"], float(np.abs(f32[i] - ref[i]).max() / den))
            if shifts[i] and (sharp_rows is None or r in sharp_rows):
                j, s = min(shifts[i].items(), key=lambda kv: kv[1])
                worst["sharp"] = min(worst["sharp"], s)
                if not s >= SHARP:
                    blunt.append((r, Ts[i], j, s))
            if not kd < BAR:
                bad.append((r, Ts[i], kd))
    print(f"[attn] {tag:<44s} {kernel:<7s} nz={nz} rows={worst['rows']:<3d} keys={worst['keys'][0]}..{worst['keys'][1]}  kernel {worst['kd']:.2e}  float32 {worst['f32']:.2e}"
          f"  least boundary key {worst['sharp']:.2e}")
    log.append(worst)
    assert not blunt, f"{tag}: dropping a boundary key moves the reference by less than {SHARP:.1e} at (row, keys, key, shift) {blunt[:6]}: change the ids / seed"
    assert not bad, f"{tag} ({kernel}, nz={nz}): max|out - ref| / max|ref| >= {BAR:.1e} at (row, keys, distance) {bad[:6]}{' ...' if len(bad) > 6 else ''}"


# --------------------------------------------------------------------------------------------------------------------------------------------
# Orpheus
# --------------------------------------------------------------------------------------------------------------------------------------------
CTX = 1061                                           # not a multiple of 16: the wave kernel's clamp to the last cache row is live
SCALE = float(np.float32(1.0) / np.sqrt(np.float32(HD)))


@functools.lru_cache(maxsize=None)
def _orpheus_model():
    return synth.build_orpheus(synth.orpheus_tiny(hidden=512, heads=NH, kv_heads=NKV, layers=2, vocab=VOCAB, ctx=CTX))


@functools.lru_cache(maxsize=None)
def _orpheus_ids():
    return np.random.default_rng(0x0A77).integers(0, VOCAB, CTX).astype(np.uint32)


def _orpheus_read(eng, n, slot_of=None):
    """the last layer of the last forward: queries, outputs, positions of its n rows, and the cache rows of every slot they read"""
    cfg = eng.cfg
    q = eng.debug_read("l_q", n * A).reshape(n, A)
    out = eng.debug_read("l_att", n * A).reshape(n, A)
    pos = eng.debug_read("l_pos", n).astype(np.int64)
    caches = {}
    for s in sorted(set(slot_of or [0])):
        caches[s] = tuple(eng.debug_read(f"l_{w}:{cfg.layers - 1}:{s}", cfg.ctx * NKV * HD).reshape(cfg.ctx, NKV * HD) for w in "kv")
    return q, out, pos, caches


# the calls of the one-sequence case, ascending through the cache: (first position, rows).  Position 511 is decoded as a call of its own and then again
# inside the 100-row piece at 500 (the same ids: the piece rewrites those cache rows).
ORPHEUS_CALLS = [(0, 255), (255, 1), (256, 1), (257, 254), (511, 1), (500, 100), (600, 40), (640, 1), (641, 3), (644, 20), (664, 256), (920, 103),
                 (1023, 1), (1024, 1), (1025, 35), (1060, 1)]
# one-row calls: position -> nz;  T = position + 1
ONE_ROW_NZ = {255: 2, 256: 2, 511: 4, 640: 5, 1023: 8, 1024: 8, 1060: 8}


@functools.lru_cache(maxsize=None)
def _orpheus_sequence(wave):
    """runs ORPHEUS_CALLS once per kernel choice; every call is checked as it is made -> (log of the checks, {position: logits} of the one-row calls)"""
    model, ids = _orpheus_model(), _orpheus_ids()
    eng = hip.OrpheusEngine(model.cfg)
    eng.tune("attn_wave", wave)
    eng.load(model)
    log, logits, failures = [], {}, []
    for p0, n in ORPHEUS_CALLS:
        lg, _ = eng.decode(ids[p0:p0 + n], p0)
        q, out, pos, caches = _orpheus_read(eng, n)
        assert pos.tolist() == list(range(p0, p0 + n))
        nz = _plan(n, p0 + n)
        kernel = "unsplit" if nz == 1 else ("wave" if wave else "split")
        if n == 1:
            assert nz == ONE_ROW_NZ[p0]
            logits[p0] = lg
        K, V = caches[0]
        try:
            _check(f"orpheus eager wave={wave} pos {p0}..{p0 + n - 1}", kernel, nz, q, out, [(int(p) + 1, K, V) for p in pos], SCALE, NKV, log)
        except AssertionError as e:      # go on: the later calls read caches this one did not write wrongly (the attention output feeds only the logits)
            failures.append(str(e))
    eng.close()
    return log, logits, failures


def _entry(log, p0, n):
    return next(e for e in log if e["tag"].endswith(f"pos {p0}..{p0 + n - 1}"))


@pytest.mark.parametrize("wave", [1, 0])
def test_orpheus_eager_decode_ascending_through_the_cache(wave):
    """cases 1 and 2.  wave=1: one-row / 3-row / 20-row calls take attn_gqa_wave_kernel<128, 4, false, float> + the combine (two full rounds at T = 256, 512, 1024; one key in a
    third round at 257 and 1025; five slices at 641; the last cache row at 1061; nz = 3 from the partials cap at 20 rows); the pieces — the 100 rows at
    500 with T = 501..600, every T mod 64 — take the unsplit attn_gqa_kernel<128, false, float>.  wave=0: the same calls through its split form <128, true, float>."""
    log, _, failures = _orpheus_sequence(wave)
    assert len(log) == len(ORPHEUS_CALLS)
    want = "wave" if wave else "split"
    for p0, nz in ONE_ROW_NZ.items():
        e = _entry(log, p0, 1)
        assert (e["kernel"], e["nz"]) == (want, nz)
    assert (_entry(log, 641, 3)["kernel"], _entry(log, 641, 3)["nz"]) == (want, 5)
    assert (_entry(log, 644, 20)["kernel"], _entry(log, 644, 20)["nz"]) == (want, 3)       # 20 rows x 4 heads x nz <= 256 partials
    assert _entry(log, 500, 100)["kernel"] == "unsplit" and _entry(log, 500, 100)["keys"] == (501, 600)
    assert not failures, "\n".join(failures)


def test_orpheus_eager_decode_logits_match_the_oracle_at_high_positions():
    """case 5: the same calls fed to the oracle; the logits of the one-row calls at positions >= 511 at the F32 bar of the decoder tests (adds the rope and
    the cache append at high positions to what the attention checks cover)"""
    _, logits, _ = _orpheus_sequence(1)
    o = orc.OrpheusOracle(_orpheus_model(), act_mode=1)
    ids = _orpheus_ids()
    seen = 0
    for p0, n in ORPHEUS_CALLS:
        ref = o.decode(ids[p0:p0 + n], p0)
        if n == 1 and p0 >= 511:
            err = float(np.abs(logits[p0] - ref).max() / np.abs(ref).max())
            print(f"[attn] orpheus logits vs oracle at position {p0}: {err:.2e}")
            assert err < 2e-4, p0
            seen += 1
    assert seen == 5


@pytest.mark.parametrize("split", [8, 3])
@pytest.mark.parametrize("n_prompt,max_new,T", [(3, 2, 4), (509, 5, 513), (600, 3, 602)])
def test_orpheus_captured_step(n_prompt, max_new, T, split):
    """case 3: generate_greedy, then the last replay of the captured step read back (attn_gqa_wave_kernel<128, 4, false, float> at a split count fixed for every position: 8, or 3 —
    no power of two).  3 ids: all keys in slice 0, the other slices leave -inf partials for the combine; 509 ids + 4 replays: position 512, at 8 slices a
    single key in round two; 600 ids: a ragged second round.  T comes from the position read back (the step's selection has already advanced it by one)."""
    model, ids = _orpheus_model(), _orpheus_ids()
    eng = hip.OrpheusEngine(model.cfg)
    eng.tune("attn_split", split)
    eng.load(model)
    toks = eng.generate_greedy(ids[:n_prompt], max_new, stop_id=VOCAB + 5)
    assert len(toks) == max_new
    q, out, pos, caches = _orpheus_read(eng, 1)
    assert int(pos[0]) == T                      # the last forward ran at position T - 1 over T keys
    K, V = caches[0]
    log = []
    _check(f"orpheus captured split={split} prompt {n_prompt}", "wave", split, q, out, [(int(pos[0]), K, V)], SCALE, NKV, log)
    eng.close()


def test_orpheus_lockstep_rows_with_their_own_slots():
    """case 4: four utterances of 2, 70, 333 and 600 prompt ids, one lock-step step: attn_gqa_kernel<128, true, float> with row_seq and the slot stride, nz = 4 from the
    longest row; the row with 3 keys has chunks of one key and an empty fourth slice; K / V are read per slot"""
    model = _orpheus_model()
    rng = np.random.default_rng(0x10C)
    lens = [2, 70, 333, 600]
    prompts = [rng.integers(0, VOCAB, n).astype(np.uint32) for n in lens]
    eng = hip.OrpheusEngine(model.cfg, max_seqs=4)
    eng.load(model)
    first = eng.generate_batch(prompts, 1, stop_id=VOCAB + 5)
    slots = [0, 1, 2, 3]
    eng.step_batch(slots, [int(f[0]) for f in first], lens, want_logits=False)
    q, out, pos, caches = _orpheus_read(eng, 4, slot_of=slots)
    assert pos.tolist() == lens
    nz = _plan(4, max(lens) + 1)
    assert nz == 4
    log = []
    _check("orpheus lock-step 4 slots", "split", nz, q, out, [(int(p) + 1,) + caches[s] for p, s in zip(pos, slots)], SCALE, NKV, log)
    eng.close()


# --------------------------------------------------------------------------------------------------------------------------------------------
# Dia
# --------------------------------------------------------------------------------------------------------------------------------------------
DIA_STEPS = (127, 128, 255, 256, 300)     # utterance 0's positions at the checked steps; utterance 1 stops at 70
DIA_STOP1 = 70
MAX_GEN = 320


@functools.lru_cache(maxsize=None)
def _dia_model(wtype):
    # 4997 audio codes: an output vocabulary of 5001
    return synth.build_dia(synth.dia_tiny(enc_heads=4, dec_hidden=512, dec_heads=NH, dec_repeat=2, max_gen=MAX_GEN, max_ctx=256, audio_vocab=VOCAB - 4, weight_type=wtype))


@functools.lru_cache(maxsize=None)
def _dia_run(max_ctx, wtype, wave):
    """two utterances stepped eagerly with debug on (the slice merge is attn_gqa_combine_kernel then), every attention launch of the checked steps against
    float64 -> (log of the self checks, log of the cross checks, failures)"""
    base = _dia_model(wtype)
    cfg = dataclasses.replace(base.cfg, max_ctx=max_ctx)          # the weights do not depend on the text context
    assert cfg.out_vocab == VOCAB and cfg.dec_kv_heads == NKV
    eng = hip.DiaEngine(cfg, max_utterances=2)
    eng.tune("attn_wave", wave)
    eng.load(base)
    eng.set_debug(True)
    # sentences a few bytes shorter than max_ctx: the zero K rows behind them take part in the softmax, the last key among them.  (Behind a short sentence most
    # keys are padding whose V rows are near copies of each other: dropping one of them moves nothing, and the sharpness condition says so.)
    trng = np.random.default_rng(0x7E47)
    for u, n_pad in enumerate((3, 9)):
        body = "".join(trng.choice(list("abcdefghijklmnopqrstuvwxyz    "), max_ctx - n_pad - 3))      # dia_tokenize adds the speaker tag, a space and the full stop
        toks, n = orc.dia_tokenize(f"[S{u + 1}] " + body.strip(" ").ljust(len(body), "e"), max_ctx)
        assert n == max_ctx - n_pad
        eng.encode_slot(u, toks, n)
    rng = np.random.default_rng(0xD1A)
    ids = rng.integers(0, cfg.audio_vocab, (2, MAX_GEN, cfg.n_out)).astype(np.uint32)
    theta_scale = _powf(10000.0, -2.0 / HD)
    kvH = NKV * HD
    self_log, cross_log, failures = [], [], []

    def check_step(pos_of):
        R = 2 * len(pos_of)
        nz_self = _plan(R, max(pos_of) + 1, cap=4 * NH * 16)
        nz_cross = _plan(R, max_ctx, cap=4 * NH * 16)
        ext = bool(wave) and max_ctx <= 16 * nz_cross * 8
        for layer in range(cfg.dec_layers):
            for kind in ("self", "cross"):
                meta = eng.debug_read(f"di_attn:{layer}:{kind}:meta", 64)
                n_parts, part_stride, ld, rows = (int(v) for v in meta[:4])
                assert rows == R
                pos, kend, seq = (meta[4 + i * R: 4 + (i + 1) * R].astype(np.int64) for i in range(3))
                assert pos.tolist() == [p for p in pos_of for _ in range(2)]
                qbuf = eng.debug_read(f"di_attn:{layer}:{kind}:q", (n_parts - 1) * part_stride + R * ld + 1)
                out = eng.debug_read(f"di_attn:{layer}:{kind}:out", R * A)
                if kind == "self":
                    assert n_parts == 1 and ld == A + 2 * kvH and kend.tolist() == (pos + 1).tolist()
                    Q = qbuf.reshape(R, ld)[:, :A]
                    cache = {int(s): tuple(eng.debug_read(f"di_{w}:{layer}:{int(s)}", MAX_GEN * kvH).reshape(MAX_GEN, kvH) for w in "kv") for s in set(seq.tolist())}
                    nz, nkv = nz_self, NKV
                    kernel = "unsplit" if nz == 1 else "split"
                else:
                    assert ld == A and kend.tolist() == [max_ctx] * R
                    assert (n_parts > 1) == (wtype == gguf.F16)        # fp16 matrices: the projection leaves K-slice slabs, the attention kernel folds them
                    Q = np.stack([ar.rope_neox(ar.fold_slabs(qbuf, n_parts, part_stride, r, ld, A), int(pos[r]), theta_scale, NH) for r in range(R)])
                    cache = {int(s): tuple(eng.debug_read(f"di_c{w}:{layer}:{int(s)}", max_ctx * A).reshape(max_ctx, A) for w in "kv") for s in set(seq.tolist())}
                    nz, nkv = nz_cross, NH
                    kernel = "unsplit" if nz == 1 else ("ext" if ext else "split")
                try:
                    _check(f"dia {kind} L{layer} ctx {max_ctx} {'f16' if wtype == gguf.F16 else 'f32'} wave={wave} pos {'/'.join(map(str, pos_of))}", kernel, nz, Q, out,
                           [(int(kend[r]),) + cache[int(seq[r])] for r in range(R)], 1.0, nkv, self_log if kind == "self" else cross_log,
                           sharp_rows=None if kind == "self" else range(0, R, 2))      # cross: the conditional rows (the module docstring says why)
                except AssertionError as e:
                    failures.append(str(e))

    for s in range(DIA_STEPS[-1] + 1):
        if s <= DIA_STOP1:
            eng.step_batch(ids[:, s], [s, s])
        elif s in DIA_STEPS:                   # both utterances with their own positions: one launch holds rows of s + 1 and 71 keys
            eng.step_batch(np.stack([ids[0, s], ids[1, DIA_STOP1]]), [s, DIA_STOP1])
        else:
            eng.step_batch(ids[:1, s], [s], slots=[0])
        if s == 0:
            check_step([0, 0])                 # position 0: no rotation of the cross query
        elif s in DIA_STEPS:
            check_step([s, DIA_STOP1])
    eng.close()
    return self_log, cross_log, failures


DIA_CASES = [(256, gguf.F16, 1), (256, gguf.F32, 1), (384, gguf.F32, 1), (320, gguf.F32, 1), (1024, gguf.F32, 1), (256, gguf.F32, 0)]
DIA_IDS = ["ctx256-f16", "ctx256-f32", "ctx384-f32", "ctx320-f32", "ctx1024-f32", "ctx256-f32-nowave"]


@pytest.mark.parametrize("max_ctx,wtype,wave", DIA_CASES[:2], ids=DIA_IDS[:2])
def test_dia_self_attention(max_ctx, wtype, wave):
    """case 6: rows of 301 and 71 keys in one launch (row_seq, a slot stride); nz = 1 up to 255 keys (attn_gqa_kernel<128, false, float>, batches two and three of 64 keys), nz = 2 from 256
    (its split form <128, true, float> + combine: chunks of two full batches at 256, two full batches and one key at 257)"""
    self_log, _, failures = _dia_run(max_ctx, wtype, wave)
    by_pos = {e["tag"].split("pos ")[1]: (e["kernel"], e["nz"]) for e in self_log}
    assert by_pos == {"0/0": ("unsplit", 1), "127/70": ("unsplit", 1), "128/70": ("unsplit", 1), "255/70": ("split", 2), "256/70": ("split", 2), "300/70": ("split", 2)}
    bad = [f for f in failures if " self " in f]
    assert not bad, "\n".join(bad)
    assert len(self_log) == 12


@pytest.mark.parametrize("max_ctx,wtype,wave", DIA_CASES, ids=DIA_IDS)
def test_dia_cross_attention(max_ctx, wtype, wave):
    """case 7: the cross-attention of the same steps over all max_ctx text positions (the K rows beyond the sentence are zero and take part), the query folded from its
    slabs and rotated by the kernel itself — restated here from the raw slabs; position 0 has no rotation, 300 a large theta.  256: attn_gqa_wave_kernel<128, 3, true, float> (EXT)
    at nz = 2, all 8 passes; 384: nz = 3; 320: 2 x 128 < 320, attn_gqa_kernel<128, true, float> with the fold and the rope; 1024: nz = 8; wave=0: the split kernel at 256"""
    _, cross_log, failures = _dia_run(max_ctx, wtype, wave)
    want = {(256, 1): ("ext", 2), (384, 1): ("ext", 3), (320, 1): ("split", 2), (1024, 1): ("ext", 8), (256, 0): ("split", 2)}[(max_ctx, wave)]
    bad = [f for f in failures if " cross " in f]
    assert not bad, "\n".join(bad)
    assert len(cross_log) == 12 and all((e["kernel"], e["nz"]) == want for e in cross_log)
