"""GPU: the opt-in e4m3 self and cross K/V caches of a Dia context (tts_hip_tune "kv_f8") and their cross-attention reader, attn_cross_f8_body
(csrc/dia_f8_kernels.h).  Models, helpers and the bar (BAR = min(4 x 1.61e-6, 1e-5) of max|ref|) are those of tests/test_gpu_dia_kv_f16.py; the float64 reference
reads the cache rows widened exactly, so the rounding is on both sides.  Measured on MI355X (printed under -s): DESIGN.md §7."""
import dataclasses

import numpy as np
import pytest

import attn_reference as ar
import oracle as orc
from e4m3_reference import e4m3_round
from test_gpu_dia_kv_f16 import (A, BAR, DIA_STOP1, EXTRA, FILLER, HD, MAX_GEN, NH, NKV, RTEXTS, SAMPLING, SHARP, TEXTS, _args, _cross, _elem, _engine, _model, _plan,
                                 _powf, _relerr, _same_bits, _self, _sentences, _session)
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

F8 = {"kv_f8": 1}
THETA = _powf(10000.0, -2.0 / HD)


def _f8(model, tune=None, **kw):
    return _engine(model, kv=gguf.F32, tune=dict(F8, **(tune or {})), **kw)


def test_stored_rows_are_the_fp32_rows_rounded_once_and_a_slots_bytes_are_its_own():
    model = _model(gguf.F16)
    cfg = model.cfg
    e32, e8 = _engine(model, kv=gguf.F32), _f8(model)
    assert (_elem(e32), _elem(e8)) == (4, 1)
    sent = _sentences(cfg.max_ctx)
    short = orc.dia_tokenize("[S2] a short one, forty bytes or so long.", cfg.max_ctx)
    rows = [(l, r) for l in range(cfg.dec_layers) for r in range(4)]

    def same_as_rounded(lens):
        live = False
        for l, r in rows:
            (k32, v32), (k8, v8) = _cross(e32, l, r), _cross(e8, l, r)
            assert _same_bits(k8, e4m3_round(k32)) and _same_bits(v8, e4m3_round(v32)), (l, r)      # the encoder does not depend on any cache
            assert not k8[lens[r // 2]:].any() and k8[:lens[r // 2]].any(axis=1).all() and v8.any(axis=1).all(), (l, r)
            live = live or not _same_bits(k8, k32)
        assert live                                                                                  # the rounding is live
    for eng in (e32, e8):
        for u, (toks, n) in enumerate(sent):
            eng.encode_slot(u, toks, n)
    same_as_rounded([sent[0][1], sent[1][1]])
    slot1 = {(l, r): _cross(e8, l, r) for l, r in rows if r >= 2}
    for eng in (e32, e8):
        eng.encode_slot(0, *short)                        # the memset behind the sentence counts one-byte elements
    same_as_rounded([short[1], sent[1][1]])
    assert all(_same_bits(k, k2) and _same_bits(v, v2) for (l, r), (k, v) in slot1.items() for k2, v2 in [_cross(e8, l, r)])
    # the self cache: layer 0's input is the embedding of the given ids, the same in both engines
    rng = np.random.default_rng(0xD1A)
    written = ([0, 1, 127, 128], [7, 8, 9, 200])
    for p0, p1 in zip(*written):
        ids = rng.integers(0, cfg.audio_vocab, (2, cfg.n_out)).astype(np.uint32)
        for eng in (e32, e8):
            eng.step_batch(ids, [p0, p1])
    for row in range(4):
        w = np.zeros(MAX_GEN, dtype=bool)
        w[written[row // 2]] = True
        for a, b in zip(_self(e32, 0, row), _self(e8, 0, row)):
            assert a[w].any(axis=1).all() and _same_bits(b[w], e4m3_round(a[w])) and not _same_bits(b[w], a[w]) and not b[~w].any(), row
    e32.close(); e8.close()


def test_session_begin_clears_position_0_of_a_slot_never_encoded():
    """dia_stream_clear_kernel<kv_f8>: offsets counted in wider elements would land in slot 0's rows"""
    model = _model(gguf.F16)
    cfg = model.cfg
    eng = _f8(model)
    eng.encode_slot(0, *_sentences(cfg.max_ctx)[0])
    before = {(l, r): _cross(eng, l, r) for l in range(cfg.dec_layers) for r in (0, 1)}
    eng.stream_begin(2, cfg.max_gen, **_args(cfg))
    for (l, r), kv in before.items():
        assert all(_same_bits(a, b) and b[0].any() for a, b in zip(kv, _cross(eng, l, r))) and not any(a[0].any() for a in _cross(eng, l, r + 2)), (l, r)
    eng.stream_end()
    eng.close()


def _launch(eng, layer, kind, max_ctx, R):
    """one attention launch of the last step -> (the query rows it used [R][A], its rows [R][A], kend [R], (K, V) per row, slabs folded)"""
    meta = eng.debug_read(f"di_attn:{layer}:{kind}:meta", 4 + 3 * R)
    n_parts, part_stride, ld, rows = (int(v) for v in meta[:4])
    assert rows == R
    pos, kend, seq = (meta[4 + i * R: 4 + (i + 1) * R].astype(np.int64) for i in range(3))
    qbuf = eng.debug_read(f"di_attn:{layer}:{kind}:q", (n_parts - 1) * part_stride + R * ld + 1)
    out = eng.debug_read(f"di_attn:{layer}:{kind}:out", R * A).reshape(R, A)
    if kind == "self":
        Q = qbuf.reshape(R, ld)[:, :A]
        cache = {int(s): _self(eng, layer, int(s)) for s in set(seq.tolist())}
    else:
        Q = np.stack([ar.rope_neox(ar.fold_slabs(qbuf, n_parts, part_stride, r, ld, A), int(pos[r]), THETA, NH) for r in range(R)])
        cache = {int(s): _cross(eng, layer, int(s), max_ctx) for s in set(seq.tolist())}
    assert all(_same_bits(a, e4m3_round(a)) for kv in cache.values() for a in kv)                  # widened exactly: what the reference reads is what the kernel read
    return Q, out, kend, [cache[int(s)] for s in seq], n_parts


def _figures(tag, Q, out, kend, kv, nkv, keys):
    """-> (worst max|out - ref| / max|ref|, least shift of the reference when one of keys(r, T) is dropped from row r)"""
    worst, least = 0.0, np.inf
    for r, (K, V) in enumerate(kv):
        T = int(kend[r])
        ref = ar.attention_rows(Q[r:r + 1], K, V, [T], 1.0, NH, nkv)[0]
        worst = max(worst, float(np.abs(out[r] - ref).max() / np.abs(ref).max()))
        if T > 1 and keys(r, T):
            least = min(least, *ar.drop_shifts(Q[r:r + 1], K, V, [T], 1.0, NH, nkv, lambda i, t: keys(r, t))[0].values())
    print(f"[dia kv f8] {tag:<44s} kernel {worst:.2e} (bar {BAR:.2e})  least edge key {least:.2e} (bar {SHARP:.2e})")
    return worst, least


CROSS = [(256, gguf.F16, 6), (384, gguf.F32, 6), (1024, gguf.F32, 6), (320, gguf.F32, 6), (256, gguf.F32, 33)]


@pytest.mark.parametrize("bounded", (0, 1))
@pytest.mark.parametrize("max_ctx,wtype,slots", CROSS, ids=["ctx256-f16-nz2", "ctx384-nz3", "ctx1024-nz8", "ctx320-generic", "rows-33-slots"])
def test_cross_attention_against_float64(max_ctx, wtype, slots, bounded):
    """256 / 384 / 1024: attn_cross_f8_kernel<bounded> at nz = 2 / 3 / 8 (F16 matrices: the query folded from its slabs), positions 0 and 5; 320: 2 x 128 < 320, the
    generic split kernel over kv_f8, never bounded; 33 slots: 264 (head, row) pairs split no keys, attn_cross_f8_rows_kernel<bounded> in the first step of an eager
    session that admits two slots of three: the others are parked (kend = 1) and leave their one V row.  The shift is taken on the conditional rows over the
    edge keys with a K row: a zero-K key behind a short sentence weighs about 1 / pads over near-identical V rows and moves a row by 9e-6 (one key, 255 pads)
    to 6e-5 (31 keys of 1024) whatever the kernel does (measured on MI355X)"""
    base = _model(wtype)
    cfg = dataclasses.replace(base.cfg, max_ctx=max_ctx)              # the weights do not depend on the text context
    R = 2 * slots
    nz = _plan(R, max_ctx, cap=R * NH * 16)
    f8_form = nz == 1 or max_ctx <= 32 * nz * 4                        # launch_attn_gqa: attn_cross_f8_rows_kernel / attn_cross_f8_kernel, else attn_gqa_kernel<128, true, kv_f8>
    assert f8_form == (max_ctx != 320) and (nz == 1) == (slots == 33)
    edges = (lambda T: ar.edge_keys(T, (31, 32, 32 * nz - 1, 32 * nz, 128 * nz - 1, 128 * nz))) if f8_form else (lambda T: ar.boundary_keys(T, -(-T // nz)))
    lens = [(1, 33, 97, max_ctx)[u % 4] for u in range(slots)] if nz == 1 else [31, 32, 33, 32 * nz - 1, 32 * nz + 1, max_ctx - 3]
    live = [u for u in range(slots) if nz > 1 or u % 3]
    eng = _f8(base, cfg=cfg, n=slots, tune={"dia_cross_bounded": 1}, flags=hip.FLAG_NO_GRAPH)
    eng.set_debug(True)
    full = _sentences(max_ctx, pads=(0,))[0][0]
    sent = [(np.where(np.arange(max_ctx) < m, full, 0).astype(np.uint32), m) for m in lens]      # cut to m keys, dia_tokenize's zero padding behind
    for u, (toks, m) in enumerate(sent):
        eng.encode_slot(u, toks, m)
    eng.tune("dia_cross_bounded", bounded)
    ids = np.random.default_rng(0xD1A).integers(0, cfg.audio_vocab, (slots, cfg.n_out)).astype(np.uint32)
    figs = []
    for pos in (0, 5) if nz > 1 else (0,):
        if nz > 1:
            eng.step_batch(ids, [pos] * slots)
        else:
            eng.stream_begin(slots, cfg.max_gen, **_args(cfg))
            eng.stream_admit(live, [sent[u][0] for u in live], [sent[u][1] for u in live])
            eng.stream_run(1)
        assert int(eng.debug_read("di_cross_bounded", 1)[0]) == (cfg.dec_layers if bounded and f8_form else 0)
        for layer in range(cfg.dec_layers):
            Q, out, kend, kv, n_parts = _launch(eng, layer, "cross", max_ctx, R)
            assert kend.tolist() == [max_ctx if r // 2 in live else 1 for r in range(R)] and (n_parts > 1) == (wtype == gguf.F16)
            assert all(not kv[r][0][lens[r // 2]:].any() for r in range(R))
            figs.append(_figures(f"cross ctx {max_ctx} nz {nz} bounded {bounded} pos {pos} L{layer}", Q, out, kend, kv, NH,
                                 lambda r, T: [] if r % 2 else [k for k in {*edges(T), lens[r // 2] - 1} if k < lens[r // 2]]))
    if nz == 1:
        eng.stream_end()
    eng.close()
    assert all(least >= SHARP for _, least in figs) and all(worst < BAR for worst, _ in figs), figs


def test_self_attention_against_float64():
    """positions 0, 127, 128, 255, 300 beside a row of 71 keys: attn_gqa_kernel<128, false, kv_f8> up to 255 keys, <128, true, kv_f8> + combine from 256"""
    model = _model(gguf.F32)
    cfg = model.cfg
    eng = _f8(model)
    eng.set_debug(True)
    for u, (toks, n) in enumerate(_sentences(cfg.max_ctx)):
        eng.encode_slot(u, toks, n)
    ids = np.random.default_rng(0xD1A).integers(0, cfg.audio_vocab, (2, MAX_GEN, cfg.n_out)).astype(np.uint32)
    figs = []
    for s in range(301):
        pos = [s, min(s, DIA_STOP1)]
        if s <= DIA_STOP1 or s in (127, 128, 255, 300):
            eng.step_batch(np.stack([ids[0, s], ids[1, pos[1]]]), pos)
        else:
            eng.step_batch(ids[:1, s], [s], slots=[0])
        if s in (0, 127, 128, 255, 300):
            nz = _plan(4, s + 1)
            edges = (lambda T: ar.boundary_keys(T, 64)) if nz == 1 else (lambda T: ar.boundary_keys(T, -(-T // nz)))
            for layer in range(cfg.dec_layers):
                Q, out, kend, kv, _ = _launch(eng, layer, "self", cfg.max_ctx, 4)
                assert kend.tolist() == [s + 1, s + 1, pos[1] + 1, pos[1] + 1]
                figs.append(_figures(f"self pos {s}/{pos[1]} nz {nz} L{layer}", Q, out, kend, kv, NKV, lambda r, T: edges(T)))
    eng.close()
    assert all(least >= SHARP for _, least in figs) and all(worst < BAR for worst, _ in figs), figs


RAW_BAR, GUIDED_BAR = 5.96e-2, 9.72e-2      # twice the worst measured on MI355X: raw 2.98e-2, guided 4.86e-2


def test_f8_cache_steps_against_the_oracle():
    """F32 matrices, the oracle with fp32 K/V, one utterance then a lock-step pair, steps 0..3.  The bars' margin covers other seeds' rounding patterns, not other
    arithmetic; the floor is the fp16 cache's figure (1.99e-4 raw, 4.30e-4 guided): the rounding shows."""
    model = synth.build_dia(synth.dia_tiny(weight_type=gguf.F32))
    cfg = model.cfg
    rng = np.random.default_rng(11)
    ids = np.concatenate([np.full((1, 2, cfg.n_out), cfg.bos), rng.integers(0, cfg.audio_vocab, (3, 2, cfg.n_out))]).astype(np.uint32)
    worst_raw = worst_guided = 0.0
    for n_utt in (1, 2):
        eng = _f8(model, n=n_utt)
        oracles = []
        for u in range(n_utt):
            toks, n = orc.dia_tokenize(TEXTS[u], cfg.max_ctx)
            eng.encode_slot(u, toks, n)
            oracles.append(orc.DiaOracle(model, act_mode=1))
            oracles[u].encode(toks, n)
        for s in range(4):
            lg, raw = eng.step_batch(ids[s, :n_utt], [s] * n_utt, want_raw=True)
            for u in range(n_utt):
                ref, ref_raw = oracles[u].step(ids[s, u], s, want_raw=True)
                worst_raw, worst_guided = max(worst_raw, _relerr(raw[u], ref_raw)), max(worst_guided, _relerr(lg[u], ref))
        eng.close()
    print(f"[dia kv f8] against the fp32-cache oracle, steps 0..3: raw {worst_raw:.2e} (bar {RAW_BAR}), guided {worst_guided:.2e} (bar {GUIDED_BAR})")
    assert 1.99e-4 < worst_raw < RAW_BAR and 4.30e-4 < worst_guided < GUIDED_BAR


@pytest.mark.parametrize("what", ["captured-loop", "session"])
def test_equalities_inside_e4m3_mode(what):
    """captured loop ids = eager loop ids (max_gen 1024: the eager split count is the captured one); session ids = tts_hip_dia_generate at the same slot count"""
    model = synth.build_dia(synth.dia_tiny(weight_type=gguf.F16, **(dict(max_gen=1024) if what == "captured-loop" else {})), suppress_special=True)
    cfg = model.cfg
    utts = [orc.dia_tokenize(t, cfg.max_ctx) for t in TEXTS] + [orc.dia_tokenize(FILLER, cfg.max_ctx)]

    def generate(slot_utts, budget, flags=0, **kw):
        eng = _f8(model, flags=flags)
        for s, u in enumerate(slot_utts):
            eng.encode_slot(s, *utts[u])
        out = eng.generate(2, budget, **kw, **_args(cfg))
        eng.close()
        return out
    if what == "captured-loop":
        uni = np.random.default_rng(3).random((40, 2, cfg.n_out), dtype=np.float32)
        got = [generate((0, 1), 40, flags=f) + generate((0, 1), 40, flags=f, uniforms=uni, **SAMPLING) for f in (0, hip.FLAG_NO_GRAPH)]
        assert all(len(a) == 39 and np.array_equal(a, b) for a, b in zip(*got)) and not np.array_equal(got[0][0], got[0][2])
        return
    budgets = [cfg.max_delay + e for e in EXTRA]
    eng = _f8(model)
    greedy, slots, refills, parked = _session(eng, 2, utts[:-1], budgets)
    assert _elem(eng) == 1 and refills >= 1 and parked >= 1
    eng.close()
    for u, s in enumerate(slots):
        want = generate((u, -1) if s == 0 else (-1, u), budgets[u])[s]
        assert greedy[u].shape == want.shape and np.array_equal(greedy[u], want), (u, s)


def test_runner_reads_the_switch_at_load(tmp_path, monkeypatch):
    from tts_cpp_amd import runner
    path = synth.build_dia(synth.dia_tiny(max_gen=64), suppress_special=True).write_gguf(str(tmp_path / "dia.gguf"))
    kw = dict(sample=0, max_tokens=40)
    monkeypatch.delenv("TTS_HIP_KV_F16", raising=False)
    monkeypatch.setenv("TTS_HIP_DIA_KV_F8", "1")
    one, many = runner.Runner(path, sample=0), runner.Runner(path, sample=0, max_seqs=3)
    monkeypatch.setenv("TTS_HIP_KV_F16", "1")
    with pytest.raises(runner.RunnerError, match=r"TTS_HIP_DIA_KV_F8 and TTS_HIP_KV_F16"):
        runner.Runner(path, sample=0)
    monkeypatch.delenv("TTS_HIP_KV_F16")
    monkeypatch.delenv("TTS_HIP_DIA_KV_F8")              # read at load: the loaded runners keep their cache type
    assert (one.kv_element_bytes(), many.kv_element_bytes()) == (1, 1)
    singles = [one.generate(t, **kw) for t in RTEXTS]
    assert all(a.size > 10 * synth.dia_tiny().hop for a in singles)
    for got in (many.generate_batch(RTEXTS[:3], **kw), many.generate_stream(RTEXTS, **kw)):
        assert all(a.shape == b.shape and np.abs(a - b).max() < 1e-5 for a, b in zip(got, singles))
    one.close(); many.close()


def test_the_key_is_refused_after_load_and_on_an_fp16_kv_type():
    cfg = synth.dia_tiny()
    eng = hip.DiaEngine(cfg, kv_type=gguf.F16)
    with pytest.raises(hip.HipError, match="kv_f8.*TTS_HIP_F16"):
        eng.tune("kv_f8", 1)
    eng.close()
    eng = hip.DiaEngine(cfg, tune=F8)
    eng.load(synth.build_dia(cfg))
    assert _elem(eng) == 1
    with pytest.raises(hip.HipError, match="kv_f8 after tts_hip_finalize"):
        eng.tune("kv_f8", 0)
    eng.close()
