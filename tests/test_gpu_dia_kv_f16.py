"""GPU: the opt-in fp16 self and cross K/V caches of a Dia context (tts_hip_dia_desc::kv_type = TTS_HIP_F16, include/tts_hip.h).

1. the writers: what llama_rope_kv_kernel<_Float16> stores into the cross cache (tts_hip_dia_encode_slot, NH = 0) and into the self cache (dia_forward) is
   np.float16 of what llama_rope_kv_kernel<float> stores, bit for bit, the zero K rows behind the sentence and the V rows there included;
2. re-encoding a slot touches that slot alone (the memset behind the sentence counts elements of the cache's size), and a session's begin clears position 0
   of a never-encoded slot without reaching the encoded one (dia_stream_clear_kernel<_Float16>);
3. the readers — attn_gqa_wave_kernel<128, 4, true, _Float16> (EXT), attn_gqa_kernel<128, false / true, _Float16> — against the float64 softmax . V of what the launch
   itself read (tests/attn_reference.py), with the scheme, the positions and the bar of test_gpu_llama_attention's Dia cases restated here: BAR =
   min(4 x 1.61e-6, 1e-5) of max|ref|.  The cache rows come back widened exactly, so the cache's rounding is on both sides and the arithmetic between the two
   numbers is fp32 on the values the reference sees: no wider bar is due.  Sharpness as there: removing a boundary key moves the reference by >= 10 x BAR on
   the conditional rows (the unconditional rows read the encoding of an all-zero text, whose V rows are copies of one another);
4. steps against the oracle, which keeps fp32 K/V, at the bars tests/test_gpu_dia.py holds fp16-matrix contexts to (2e-3 raw, 8e-3 guided);
5. the equalities the API promises, inside fp16 mode; 6. the runner's switch; 7. the refusal of any other kv_type.
(The kernel is instantiated at one U, so there is no comparison of bits across U.)

Measured on MI355X (printed under -s; DESIGN.md, "fp16 K/V caches of a Dia context"): kernel distances 0.9e-7 .. 3.0e-7 of max|ref| (bar 6.44e-6) — the new
EXT kernel 0.9e-7 .. 2.0e-7, the split kernel on cross rows 1.2e-7 .. 2.1e-7, self rows 1.1e-7 .. 3.0e-7; least boundary-key shift 4.0e-4 (bar 6.44e-5);
logits against the oracle: see test_f16_cache_steps_against_the_oracle."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import attn_reference as ar
import oracle as orc
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

F32_WORST = 1.61e-6         # tests/test_gpu_llama_attention.py: the float32 evaluation of the same formula against float64
BAR = min(4 * F32_WORST, 1e-5)
SHARP = 10 * BAR
NH, NKV, HD = 4, 2, 128
A = NH * HD
KVH = NKV * HD
VOCAB = 5001
MAX_GEN = 320
DIA_STEPS = (127, 128, 255, 256, 300)     # utterance 0's positions at the checked steps; utterance 1 stops at 70
DIA_STOP1 = 70


def _powf(x, y):
    """the host's powf (theta_scale is computed with it in float32)"""
    try:
        f = ctypes.CDLL("libm.so.6").powf
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
        return float(f(x, y))
    except OSError:
        return float(np.float32(x) ** np.float32(y))


@functools.lru_cache(maxsize=None)
def _model(wtype):
    # 4997 audio codes: an output vocabulary of 5001
    return synth.build_dia(synth.dia_tiny(enc_heads=4, dec_hidden=512, dec_heads=NH, dec_repeat=2, max_gen=MAX_GEN, max_ctx=256, audio_vocab=VOCAB - 4, weight_type=wtype))


def _engine(model, cfg=None, kv=gguf.F16, n=2, tune=None, **kw):
    eng = hip.DiaEngine(cfg or model.cfg, max_utterances=n, kv_type=kv, **kw)
    for k, v in (tune or {}).items():
        eng.tune(k, v)
    eng.load(model)
    return eng


def _elem(eng):
    return int(eng.debug_read("di_kv_elem", 1)[0])


def _sentences(max_ctx, pads=(3, 9)):
    """one sentence per slot, pads[u] bytes short of max_ctx: the zero K rows behind them take part in the softmax, the last key among them"""
    trng = np.random.default_rng(0x7E47)
    out = []
    for u, n_pad in enumerate(pads):
        body = "".join(trng.choice(list("abcdefghijklmnopqrstuvwxyz    "), max_ctx - n_pad - 3))      # dia_tokenize adds the speaker tag, a space and the full stop
        toks, n = orc.dia_tokenize(f"[S{u % 2 + 1}] " + body.strip(" ").ljust(len(body), "e"), max_ctx)
        assert n == max_ctx - n_pad
        out.append((toks, n))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rounded(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def _cross(eng, layer, row, max_ctx=256):
    return tuple(eng.debug_read(f"di_c{w}:{layer}:{row}", max_ctx * A).reshape(max_ctx, A) for w in "kv")


def _self(eng, layer, row):
    return tuple(eng.debug_read(f"di_{w}:{layer}:{row}", MAX_GEN * KVH).reshape(MAX_GEN, KVH) for w in "kv")


# ---- 1. the writers ---------------------------------------------------------------------------------------------------------------------
def test_stored_rows_are_the_fp32_rows_rounded_once():
    model = _model(gguf.F16)
    cfg = model.cfg
    e32, e16 = _engine(model, kv=gguf.F32), _engine(model, kv=gguf.F16)
    assert (_elem(e32), _elem(e16)) == (4, 2)
    sent = _sentences(cfg.max_ctx)
    for eng in (e32, e16):
        for u, (toks, n) in enumerate(sent):
            eng.encode_slot(u, toks, n)
    live = False
    for layer in range(cfg.dec_layers):
        for row in range(4):
            n = sent[row // 2][1]
            (k32, v32), (k16, v16) = _cross(e32, layer, row), _cross(e16, layer, row)
            assert max(np.abs(k32).max(), np.abs(v32).max()) < 65504
            assert _same_bits(k16, _rounded(k32)) and _same_bits(v16, _rounded(v32)), (layer, row)      # the encoder does not depend on any cache
            assert not k32[n:].any() and not k16[n:].any(), (layer, row)                                # K behind the sentence: zero, as in a cleared cache
            assert k32[:n].any(axis=1).all() and v16[n:].any(axis=1).all(), (layer, row)                # V is stored for all positions
            live = live or not _same_bits(k16, k32)
    assert live                                                                                         # the rounding is live: the fp32 rows are not fp16 numbers
    # the self cache: layer 0's input is the embedding of the given ids, the same in both engines whatever the deeper layers and the cross cache did
    rng = np.random.default_rng(0xD1A)
    written = {0: [], 1: []}
    for p0, p1 in ((0, 7), (1, 8), (127, 9), (128, 200)):
        ids = rng.integers(0, cfg.audio_vocab, (2, cfg.n_out)).astype(np.uint32)
        for eng in (e32, e16):
            eng.step_batch(ids, [p0, p1])
        written[0].append(p0); written[1].append(p1)
    for row in range(4):
        w = np.zeros(MAX_GEN, dtype=bool)
        w[written[row // 2]] = True
        for name, a, b in zip("KV", _self(e32, 0, row), _self(e16, 0, row)):
            assert a[w].any(axis=1).all() and np.abs(a[w]).max() < 65504
            assert _same_bits(b[w], _rounded(a[w])), f"layer 0 self {name} rows of row slot {row} are not the fp32 rows rounded to nearest-even"
            assert not a[~w].any() and not b[~w].any(), f"an unwritten self {name} row of row slot {row} is not zero"
            assert not _same_bits(b[w], a[w])
    e32.close(); e16.close()


# ---- 2. a slot's rows are its own -------------------------------------------------------------------------------------------------------
def test_reencoding_a_slot_touches_only_that_slot():
    model = _model(gguf.F16)
    cfg = model.cfg
    e32, e16 = _engine(model, kv=gguf.F32), _engine(model, kv=gguf.F16)
    long0, long1 = _sentences(cfg.max_ctx)
    short, n_short = orc.dia_tokenize("[S2] a short one, forty bytes or so long.", cfg.max_ctx)
    assert 30 < n_short < 60
    e16.encode_slot(0, *long0)
    e16.encode_slot(1, *long1)
    before = {(l, r): _cross(e16, l, r) for l in range(cfg.dec_layers) for r in (2, 3)}
    old0 = {(l, r): _cross(e16, l, r) for l in range(cfg.dec_layers) for r in (0, 1)}
    e16.encode_slot(0, short, n_short)
    e32.encode_slot(0, short, n_short)
    for (l, r), (k, v) in before.items():
        k2, v2 = _cross(e16, l, r)
        assert _same_bits(k, k2) and _same_bits(v, v2), f"slot 1's cross rows of layer {l}, row slot {r} changed when slot 0 was encoded again"
        assert k2[:long1[1]].any(axis=1).all()
    for l in range(cfg.dec_layers):
        for r in (0, 1):
            (k, v), (k32, v32) = _cross(e16, l, r), _cross(e32, l, r)
            assert not k[n_short:].any(), (l, r)                              # a memset of half the bytes would leave the old sentence's rows here
            assert k[:n_short].any(axis=1).all(), (l, r)                      # one of twice the bytes would zero the next row slot's first rows
            assert _same_bits(k, _rounded(k32)) and _same_bits(v, _rounded(v32)), (l, r)
        assert not _same_bits(_cross(e16, l, 0)[1], old0[(l, 0)][1])          # the conditional row's V rows are the new sentence's
    e32.close(); e16.close()


def _args(cfg):
    return dict(delay_pattern=[0, 8, 9, 10, 11, 12, 13, 14, 15], bos=cfg.bos, eos=cfg.eos, pad=cfg.pad, max_delay=cfg.max_delay)


def test_session_begin_clears_position_0_of_a_slot_never_encoded():
    """slot 1 never encoded: dia_stream_clear_kernel<_Float16> zeroes position 0 of its rows (what its parked rows attend over) and nothing of slot 0.  Offsets
    counted in 4-byte elements would land in slot 0's rows of the next layer."""
    model = _model(gguf.F16)
    cfg = model.cfg
    eng = _engine(model)
    eng.encode_slot(0, *_sentences(cfg.max_ctx)[0])
    before = {(l, r): _cross(eng, l, r) for l in range(cfg.dec_layers) for r in (0, 1)}
    eng.stream_begin(2, cfg.max_gen, **_args(cfg))
    for (l, r), (k, v) in before.items():
        k2, v2 = _cross(eng, l, r)
        assert _same_bits(k, k2) and _same_bits(v, v2) and k2[0].any() and v2[0].any(), (l, r)
    for l in range(cfg.dec_layers):
        for r in (2, 3):
            k, v = _cross(eng, l, r)
            assert not k[0].any() and not v[0].any()
    eng.stream_end()
    eng.close()


# ---- 3. the readers against float64 -----------------------------------------------------------------------------------------------------
def _plan(rows, max_keys, split_max=8, cap=4 * NH * 16, fixed=False):
    """launch_attn_gqa's split count"""
    nz = 1
    if split_max > 1 and NH * rows <= 256:
        nz = split_max if fixed else min(split_max, max(1, max_keys // 128))
        while nz > 1 and rows * NH * nz > cap:
            nz -= 1
    return nz


def _edges(kernel, nz, T):
    """the keys next to a batch, pass, slot-recycling or chunk edge of a row of T keys: 64-key batches (unsplit), chunks of ceil(T / nz) in batches of 64 (split),
    passes of 16 nz keys and the recycling of its 4 register slots (ext)"""
    if T <= 1:
        return []
    if kernel == "unsplit":
        return ar.boundary_keys(T, 64)
    if kernel == "split":
        return ar.boundary_keys(T, -(-T // nz))
    return ar.edge_keys(T, (15, 16, 16 * nz - 1, 16 * nz, 64 * nz - 1, 64 * nz))


def _check(tag, kernel, nz, Q, out, rows, nkv, log, sharp_rows=None):
    """rows: per row (T, K, V) — the cache rows that row read; scale 1.0 (Dia).  -> appends the worst figures to log, raises on a miss"""
    Q, out = np.asarray(Q).reshape(len(rows), A), np.asarray(out).reshape(len(rows), A)
    groups = {}
    for r, (T, K, V) in enumerate(rows):
        groups.setdefault((id(K), id(V)), []).append(r)
    worst = dict(tag=tag, kernel=kernel, nz=nz, kd=0.0, sharp=np.inf)
    bad, blunt = [], []
    for rs in groups.values():
        K, V = rows[rs[0]][1], rows[rs[0]][2]
        Ts = [rows[r][0] for r in rs]
        ref = ar.attention_rows(Q[rs], K, V, Ts, 1.0, NH, nkv)
        shifts = ar.drop_shifts(Q[rs], K, V, Ts, 1.0, NH, nkv, lambda i, T: _edges(kernel, nz, T))
        for i, r in enumerate(rs):
            kd = float(np.abs(out[r] - ref[i]).max() / np.abs(ref[i]).max())
            worst["kd"] = max(worst["kd"], kd)
            if shifts[i] and (sharp_rows is None or r in sharp_rows):
                j, s = min(shifts[i].items(), key=lambda kv: kv[1])
                worst["sharp"] = min(worst["sharp"], s)
                if not s >= SHARP:
                    blunt.append((r, Ts[i], j, s))
            if not kd < BAR:
                bad.append((r, Ts[i], kd))
    print(f"[dia kv f16] {tag:<52s} {kernel:<7s} nz={nz}  kernel {worst['kd']:.2e}  least boundary key {worst['sharp']:.2e}")
    log.append(worst)
    assert not blunt, f"{tag}: dropping a boundary key moves the reference by less than {SHARP:.1e} at (row, keys, key, shift) {blunt[:6]}"
    assert not bad, f"{tag} ({kernel}, nz={nz}): max|out - ref| / max|ref| >= {BAR:.1e} at (row, keys, distance) {bad[:6]}"


@functools.lru_cache(maxsize=None)
def _run(max_ctx, wtype, wave):
    """two utterances stepped eagerly with debug on over an fp16 cache, every attention launch of the checked steps against float64
    -> (log of the self checks, log of the cross checks, failures)"""
    base = _model(wtype)
    cfg = dataclasses.replace(base.cfg, max_ctx=max_ctx)          # the weights do not depend on the text context
    assert cfg.out_vocab == VOCAB and cfg.dec_kv_heads == NKV
    eng = _engine(base, cfg=cfg, tune={"attn_wave": wave})
    assert _elem(eng) == 2
    eng.set_debug(True)
    for u, (toks, n) in enumerate(_sentences(max_ctx)):
        eng.encode_slot(u, toks, n)
    rng = np.random.default_rng(0xD1A)
    ids = rng.integers(0, cfg.audio_vocab, (2, MAX_GEN, cfg.n_out)).astype(np.uint32)
    theta_scale = _powf(10000.0, -2.0 / HD)
    self_log, cross_log, failures = [], [], []

    def fp16_numbers(*arrays):
        return all(_same_bits(a, _rounded(a)) for a in arrays)

    def check_step(pos_of):
        R = 2 * len(pos_of)
        nz_self = _plan(R, max(pos_of) + 1)
        nz_cross = _plan(R, max_ctx)
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
                    assert n_parts == 1 and ld == A + 2 * KVH and kend.tolist() == (pos + 1).tolist()
                    Q = qbuf.reshape(R, ld)[:, :A]
                    cache = {int(s): _self(eng, layer, int(s)) for s in set(seq.tolist())}
                    nz, nkv = nz_self, NKV
                    kernel = "unsplit" if nz == 1 else "split"
                else:
                    assert ld == A and kend.tolist() == [max_ctx] * R
                    assert (n_parts > 1) == (wtype == gguf.F16)        # fp16 matrices: the projection leaves K-slice slabs, the attention kernel folds them
                    Q = np.stack([ar.rope_neox(ar.fold_slabs(qbuf, n_parts, part_stride, r, ld, A), int(pos[r]), theta_scale, NH) for r in range(R)])
                    cache = {int(s): _cross(eng, layer, int(s), max_ctx) for s in set(seq.tolist())}
                    nz, nkv = nz_cross, NH
                    kernel = "unsplit" if nz == 1 else ("ext" if ext else "split")
                assert all(fp16_numbers(*kv) for kv in cache.values())      # widened exactly: what the reference reads is what the kernel read
                try:
                    _check(f"dia {kind} L{layer} ctx {max_ctx} {'f16' if wtype == gguf.F16 else 'f32'} wave={wave} pos {'/'.join(map(str, pos_of))}", kernel, nz, Q, out,
                           [(int(kend[r]),) + cache[int(seq[r])] for r in range(R)], nkv, self_log if kind == "self" else cross_log,
                           sharp_rows=None if kind == "self" else range(0, R, 2))
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


CASES = [(256, gguf.F16, 1), (256, gguf.F32, 1), (384, gguf.F32, 1), (320, gguf.F32, 1), (1024, gguf.F32, 1), (256, gguf.F32, 0)]
CASE_IDS = ["ctx256-f16", "ctx256-f32", "ctx384-f32", "ctx320-f32", "ctx1024-f32", "ctx256-f32-nowave"]


@pytest.mark.parametrize("max_ctx,wtype,wave", CASES[:2], ids=CASE_IDS[:2])
def test_f16_cache_self_attention(max_ctx, wtype, wave):
    """rows of up to 301 and 71 keys in one launch (row_seq, the slot stride in elements): attn_gqa_kernel<128, false, _Float16> up to 255 keys, <128, true, _Float16> + combine from 256"""
    self_log, _, failures = _run(max_ctx, wtype, wave)
    by_pos = {e["tag"].split("pos ")[1]: (e["kernel"], e["nz"]) for e in self_log}
    assert by_pos == {"0/0": ("unsplit", 1), "127/70": ("unsplit", 1), "128/70": ("unsplit", 1), "255/70": ("split", 2), "256/70": ("split", 2), "300/70": ("split", 2)}
    bad = [f for f in failures if " self " in f]
    assert not bad, "\n".join(bad)
    assert len(self_log) == 12


@pytest.mark.parametrize("max_ctx,wtype,wave", CASES, ids=CASE_IDS)
def test_f16_cache_cross_attention(max_ctx, wtype, wave):
    """256: attn_gqa_wave_kernel<128, 4, true, _Float16> at nz = 2 (F16 matrices: the query folded from its slabs); 384: nz = 3; 1024: nz = 8; 320: 2 x 128 < 320,
    attn_gqa_kernel<128, true, _Float16> with the fold and the rope; wave=0: that kernel at 256"""
    _, cross_log, failures = _run(max_ctx, wtype, wave)
    want = {(256, 1): ("ext", 2), (384, 1): ("ext", 3), (320, 1): ("split", 2), (1024, 1): ("ext", 8), (256, 0): ("split", 2)}[(max_ctx, wave)]
    bad = [f for f in failures if " cross " in f]
    assert not bad, "\n".join(bad)
    assert len(cross_log) == 12 and all((e["kernel"], e["nz"]) == want for e in cross_log)


# ---- 4. against the oracle --------------------------------------------------------------------------------------------------------------
def _relerr(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def test_f16_cache_steps_against_the_oracle():
    """F32 matrices, fp16 caches, the oracle with fp32 K/V: one utterance, then a lock-step pair, steps 0..3.  The bars are those of an fp16-matrix context
    in tests/test_gpu_dia.py (2e-3 raw, 8e-3 guided, of max|oracle|)."""
    model = synth.build_dia(synth.dia_tiny(weight_type=gguf.F32))
    cfg = model.cfg
    texts = ["[S1] first one.", "[S2] the second is long."]
    rng = np.random.default_rng(11)
    ids = np.concatenate([np.full((1, 2, cfg.n_out), cfg.bos), rng.integers(0, cfg.audio_vocab, (3, 2, cfg.n_out))]).astype(np.uint32)
    worst_raw = worst_guided = 0.0
    for n_utt in (1, 2):
        eng = _engine(model, n=n_utt)
        assert _elem(eng) == 2
        oracles = []
        for u in range(n_utt):
            toks, n = orc.dia_tokenize(texts[u], cfg.max_ctx)
            eng.encode_slot(u, toks, n)
            o = orc.DiaOracle(model, act_mode=1)
            o.encode(toks, n)
            oracles.append(o)
        for s in range(4):
            lg, raw = eng.step_batch(ids[s, :n_utt], [s] * n_utt, want_raw=True)
            for u in range(n_utt):
                ref, ref_raw = oracles[u].step(ids[s, u], s, want_raw=True)
                worst_raw, worst_guided = max(worst_raw, _relerr(raw[u], ref_raw)), max(worst_guided, _relerr(lg[u], ref))
        eng.close()
    print(f"[dia kv f16] against the fp32-cache oracle, steps 0..3: raw {worst_raw:.2e} (bar 2e-3), guided {worst_guided:.2e} (bar 8e-3)")
    assert worst_raw < 2e-3       # measured on MI355X: 1.99e-4
    assert worst_guided < 8e-3    # measured on MI355X: 4.30e-4


# ---- 5. the equalities of the API, inside fp16 mode -------------------------------------------------------------------------------------
TEXTS = ["[S1] first one.", "[S2] the second is long.", "[S1] hi.", "[S1] a [S2] b [S1] c.", "[S2] number five."]
FILLER = "[S1] somebody else."
EXTRA = (2, 9, 5, 18, 6)          # budgets max_delay + these
SAMPLING = dict(top_k=8, repetition_penalty=1.3)


def test_captured_loop_equals_the_eager_loop():
    """max_gen 1024: the eager step's key-split count (max_gen / 128) is the captured step's fixed one, so both run the same launches.  The loop hands out
    ids, not logits: identical ids of 40 steps, greedy and sampled, say the logits behind every selection chose alike."""
    model = synth.build_dia(synth.dia_tiny(max_gen=1024, weight_type=gguf.F16), suppress_special=True)
    cfg = model.cfg
    uni = np.random.default_rng(3).random((40, 2, cfg.n_out), dtype=np.float32)
    got = []
    for flags in (0, hip.FLAG_NO_GRAPH):
        eng = _engine(model, flags=flags)
        for u in range(2):
            eng.encode_slot(u, *orc.dia_tokenize(TEXTS[u], cfg.max_ctx))
        got.append(eng.generate(2, 40, **_args(cfg)) + eng.generate(2, 40, uniforms=uni, **SAMPLING, **_args(cfg)))
        eng.close()
    assert len(got[0]) == 4 and all(len(a) == 39 for a in got[0])
    assert all(np.array_equal(a, b) for a, b in zip(*got))
    assert not np.array_equal(got[0][0], got[0][2])


@pytest.mark.parametrize("piece", [1, 5, 64])
def test_generate_equals_the_gen_pieces(piece):
    model = synth.build_dia(synth.dia_tiny(weight_type=gguf.F16), suppress_special=True)
    cfg = model.cfg
    eng = _engine(model)
    for u in range(2):
        eng.encode_slot(u, *orc.dia_tokenize(TEXTS[u], cfg.max_ctx))
    budget = cfg.max_delay + 9
    want = eng.generate(2, budget, **_args(cfg))
    eng.gen_begin(2, budget, **_args(cfg))
    for _ in range(budget + 2):
        eng.gen_launch(piece)
        out, steps, done, _ = eng.gen_wait()
        if done.all():
            break
    assert done.all() and steps.tolist() == [len(w) for w in want]
    for u in range(2):
        assert np.array_equal(out[u, :steps[u]], want[u]), (piece, u)
    eng.close()


def _session(eng, n_slots, utts, budgets, uniforms=None, run=4, **sampling):
    """utts through one session: the first n_slots at once, the rest as slots free up -> (ids per utterance, slot per utterance, admissions beside live slots,
    look-ins that found a parked slot beside a live one)"""
    cfg = eng.cfg
    eng.stream_begin(n_slots, cfg.max_gen, sampled=uniforms is not None, **sampling, **_args(cfg))
    out, slot_of, in_slot = [None] * len(utts), [None] * len(utts), {}
    free, nxt, refills, parked_beside_live = list(range(n_slots)), 0, 0, 0

    def admit():
        nonlocal nxt
        take = []
        while free and nxt < len(utts):
            take.append((free.pop(0), nxt))
            nxt += 1
        if take:
            eng.stream_admit([s for s, _ in take], [utts[u][0] for _, u in take], [utts[u][1] for _, u in take], budgets=[budgets[u] for _, u in take],
                             uniforms=None if uniforms is None else np.stack([uniforms[u] for _, u in take]))
            for s, u in take:
                in_slot[s], slot_of[u] = u, s
        return len(take)

    admit()
    for _ in range(200):
        if not in_slot:
            break
        for s, steps in eng.stream_run(run):
            out[in_slot.pop(s)] = eng.stream_collect(s, steps)
            free.append(s)
        free.sort()
        live = len(in_slot)
        if admit() and live:
            refills += 1
        if free and in_slot:
            parked_beside_live += 1      # nothing left to admit: the free slot stays parked over the next run
    assert not in_slot and nxt == len(utts)
    eng.stream_end()
    return out, slot_of, refills, parked_beside_live


def _reference(model, n_slots, slot, utt, budget, filler, uniforms=None, **sampling):
    """tts_hip_dia_generate on a fresh fp16-cache context with n_utt = n_slots: the utterance in `slot`, any encoded sentence in the others"""
    cfg = model.cfg
    eng = _engine(model, n=n_slots)
    for s in range(n_slots):
        eng.encode_slot(s, *(utt if s == slot else filler))
    outs = [eng.generate(n_slots, budget, **_args(cfg))[slot]]
    if uniforms is not None:
        u = np.random.default_rng(99).random((budget, n_slots, cfg.n_out), dtype=np.float32)
        u[:, slot, :] = uniforms[:budget]
        outs.append(eng.generate(n_slots, budget, uniforms=u, **sampling, **_args(cfg))[slot])
    eng.close()
    return outs


def test_session_equals_lockstep_generation():
    model = synth.build_dia(synth.dia_tiny(weight_type=gguf.F16), suppress_special=True)
    cfg = model.cfg
    utts = [orc.dia_tokenize(t, cfg.max_ctx) for t in TEXTS]
    filler = orc.dia_tokenize(FILLER, cfg.max_ctx)
    budgets = [cfg.max_delay + e for e in EXTRA]
    uni = np.random.default_rng(5).random((len(utts), cfg.max_gen, cfg.n_out), dtype=np.float32)
    eng = _engine(model)
    assert _elem(eng) == 2
    greedy, slots, refills, parked = _session(eng, 2, utts, budgets)
    assert refills >= 1 and parked >= 1 and all(slots.count(s) >= 2 for s in range(2))
    sampled, slots_s, _, _ = _session(eng, 2, utts, budgets, uniforms=uni, **SAMPLING)
    assert slots_s == slots
    eng.close()
    for u in range(len(utts)):
        ref_g, ref_s = _reference(model, 2, slots[u], utts[u], budgets[u], filler, uniforms=uni[u], **SAMPLING)
        assert greedy[u].shape == ref_g.shape and np.array_equal(greedy[u], ref_g), (u, slots[u])
        assert sampled[u].shape == ref_s.shape and np.array_equal(sampled[u], ref_s), (u, slots[u])
    assert not np.array_equal(sampled[0], greedy[0])


def test_mixed_session_with_two_samplers_equals_each_utterances_own_run():
    model = synth.build_dia(synth.dia_tiny(weight_type=gguf.F16), suppress_special=True)
    cfg = model.cfg
    settings = [dict(top_k=8, repetition_penalty=1.3), dict(top_k=20, top_p=0.9, temperature=0.8, repetition_penalty=1.1)]
    utts = [orc.dia_tokenize(t, cfg.max_ctx) for t in TEXTS[:2]]
    filler = orc.dia_tokenize(FILLER, cfg.max_ctx)
    budgets = [cfg.max_delay + 9, cfg.max_delay + 5]
    uni = np.random.default_rng(6).random((2, cfg.max_gen, cfg.n_out), dtype=np.float32)
    eng = _engine(model)
    eng.stream_begin_mixed(2, cfg.max_gen, **_args(cfg))
    eng.stream_admit_mixed([0, 1], [u[0] for u in utts], [u[1] for u in utts], settings, budgets=budgets, uniforms=uni)
    fin = []
    for _ in range(20):
        eng.stream_launch(4)             # the launch / wait form of stream_run
        fin += eng.stream_wait()[3]
        if len(fin) == 2:
            break
    got = {s: eng.stream_collect(s, steps) for s, steps in fin}
    eng.stream_end()
    eng.close()
    assert sorted(got) == [0, 1]
    for u in range(2):
        ref = _engine(model)
        for s in range(2):
            ref.encode_slot(s, *(utts[u] if s == u else filler))
        col = np.random.default_rng(99).random((budgets[u], 2, cfg.n_out), dtype=np.float32)
        col[:, u, :] = uni[u, :budgets[u]]
        want = ref.generate(2, budgets[u], uniforms=col, **settings[u], **_args(cfg))[u]
        ref.close()
        assert got[u].shape == want.shape and np.array_equal(got[u], want), u


# ---- 6. the runner ----------------------------------------------------------------------------------------------------------------------
RTEXTS = [" Hi there [S2] ok", "[S1] another one.", "[S2] short", "[S1] the fourth one."]


def test_runner_reads_the_switch_at_load(tmp_path, monkeypatch):
    from tts_cpp_amd import runner
    path = synth.build_dia(synth.dia_tiny(max_gen=64), suppress_special=True).write_gguf(str(tmp_path / "dia.gguf"))
    hop = synth.dia_tiny().hop
    kw = dict(sample=0, max_tokens=40)
    monkeypatch.delenv("TTS_HIP_KV_F16", raising=False)
    plain = runner.Runner(path, sample=0)
    assert plain.kv_element_bytes() == 4
    plain_audio = plain.generate(RTEXTS[0], **kw)
    monkeypatch.setenv("TTS_HIP_KV_F16", "1")
    one = runner.Runner(path, sample=0)
    many = runner.Runner(path, sample=0, max_seqs=3)
    monkeypatch.delenv("TTS_HIP_KV_F16")         # read at load: the loaded runners keep their cache type
    assert (one.kv_element_bytes(), many.kv_element_bytes()) == (2, 2)
    singles, ids = [], []
    for t in RTEXTS:
        singles.append(one.generate(t, **kw))
        ids.append(one.last_tokens(1).copy())
    assert all(a.size > 10 * hop for a in singles)
    batch = many.generate_batch(RTEXTS[:3], **kw)
    for i in range(3):
        assert ids[i].size > 0 and np.array_equal(many.last_tokens(16 + i), ids[i]), i
        assert batch[i].shape == singles[i].shape and np.abs(batch[i] - singles[i]).max() < 1e-5, i
    stream = many.generate_stream(RTEXTS, **kw)
    assert len(stream) == len(RTEXTS)
    for a, b in zip(stream, singles):
        assert a.shape == b.shape and np.abs(a - b).max() < 1e-5
    chunks = many.generate_stream_chunked(RTEXTS, chunk_frames=8, **kw)
    for i, b in enumerate(singles):
        cat = np.concatenate([a for u, a, _ in chunks if u == i])
        assert cat.shape == b.shape and np.abs(cat - b).max() < 1e-5, i
        assert np.array_equal(many.last_tokens(16 + i), ids[i]), i
    assert np.array_equal(plain.generate(RTEXTS[0], **kw), plain_audio) and plain.kv_element_bytes() == 4      # unchanged beside fp16 runners in the process
    plain.close(); one.close(); many.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [2, 30, 0xFFFFFFFF])
def test_any_other_kv_type_is_refused(bad):
    cfg = synth.dia_tiny()
    with pytest.raises(hip.HipError, match=r"tts_hip_dia_create: kv_type"):
        hip.DiaEngine(cfg, kv_type=bad)
    eng = hip.DiaEngine(cfg, kv_type=gguf.F16)          # a valid create works afterwards
    model = synth.build_dia(cfg)
    eng.load(model)
    assert _elem(eng) == 2
    eng.close()
