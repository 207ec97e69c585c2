"""GPU: Parler's opt-in e4m3 self-attention K/V cache (tts_hip_tune "kv_f8").  Writers: the cache rows equal e4m3_round of the fp32 engine's
rows bit for bit.  Readers: the attention rows against the float64 softmax . V (tests/attn_reference.py) of what the launch read back — q, the decoded cache
rows, pos, seq — under the bar of tests/test_gpu_parler_attention.py (7.16e-6 of max|ref|), and a
dropped boundary key must move that reference by ten times the bar.  Paths: captured generation and a session against the eager step loop.  Selection."""
import ctypes as C

import numpy as np
import pytest

import attn_reference as ar
import oracle as orc
from e4m3_reference import e4m3_round
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

BAR = 7.16e-6
NH, HD, H, SCALE = 4, 64, 256, 0.125
F8 = {"kv_f8": 1}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _engine(model, max_seqs, tune=None, **kw):
    eng = hip.HipEngine(model.cfg, max_seqs=max_seqs, use_cross_attn=False, tune=tune, **kw)
    eng.load(model)
    return eng


# ---- 1. writers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wtype,gain,flags", [(gguf.F16, 1.0, 0), (gguf.Q8_0, 1.0, 0), (gguf.F16, 4000.0, 0), (gguf.F32, 1.0, hip.FLAG_VALU_GEMM)],
                         ids=["f16", "q8_0", "f16-beyond-448", "f32-scalar-gemm"])
def test_cache_rows_are_the_fp32_rows_rounded_once(wtype, gain, flags):
    """prefill (9 rows: gemm16 / qgemm16), a 70-row prefill (the tiled fp16 and integer GEMMs), a one-row step and a lock-step step of three slots;
    fp32 matrices under FLAG_VALU_GEMM: gemv_valu_kernel's byte stores"""
    model = synth.build(synth.tiny(weight_type=wtype, kv_gain=gain))
    cfg, rng = model.cfg, np.random.default_rng(8)
    prompts = [rng.integers(3, cfg.prompt_vocab, n).astype(np.uint32) for n in (9, 70, 3)]
    audio = rng.integers(0, cfg.audio_vocab, (3, cfg.n_out)).astype(np.uint32)
    rows = {}
    for name, tune in (("f32", None), ("f8", F8)):
        eng = _engine(model, 3, tune, flags=flags)
        for s, p in enumerate(prompts):
            eng.prefill(s, p)
        eng.step(audio[:1], [9], [0])
        eng.step(audio, [10, 70, 3], [0, 1, 2])
        rows[name] = [eng.debug_read(f"{w}:0:{s}", n * H) for w in "kv" for s, n in ((0, 11), (1, 71), (2, 4))]
        eng.close()
    for a, b in zip(rows["f32"], rows["f8"]):
        assert np.isfinite(b).all() and np.array_equal(_bits(e4m3_round(a)), _bits(b))
    big = max(float(np.abs(a).max()) for a in rows["f32"])
    assert (big > 448.0) == (gain > 1.0) and max(float(np.abs(b).max()) for b in rows["f8"]) == (448.0 if gain > 1.0 else e4m3_round(np.float32([big]))[0])


# ---- 2. readers ---------------------------------------------------------------------------------------------------------------------------------
def _check(eng, pos, seq, edges):
    """the last layer's self-attention of the forward that just ran, every row and head of it"""
    R, L = len(pos), eng.cfg.layers
    q, out = eng.debug_read("q", R * H).reshape(R, H), eng.debug_read("att", R * H).reshape(R, H).astype(np.float64)
    assert eng.debug_read("pos", R).tolist() == list(pos) and eng.debug_read("seq", R).tolist() == list(seq)
    for s in sorted(set(seq)):
        rs = [r for r in range(R) if seq[r] == s]
        Ts = [pos[r] + 1 for r in rs]
        K, V = (eng.debug_read(f"{w}:{L - 1}:{s}", max(Ts) * H).reshape(max(Ts), H) for w in "kv")
        assert np.array_equal(_bits(e4m3_round(K)), _bits(K))       # what the launch read are e4m3 numbers
        ref = ar.attention_rows(q[rs], K, V, Ts, SCALE, NH, NH, hd=HD)
        shifts = ar.drop_shifts(q[rs], K, V, Ts, SCALE, NH, NH, lambda i, T: ar.edge_keys(T, edges(T)) if T > 1 else [], hd=HD)
        for i, r in enumerate(rs):
            for h in range(NH):
                sl = slice(h * HD, (h + 1) * HD)
                den, err = np.abs(ref[i, sl]).max(), np.abs(out[r, sl] - ref[i, sl])
                assert err.max() / den < BAR, (r, h, Ts[i], float(err.max() / den))
            if shifts[i]:
                assert min(shifts[i].values()) >= 10 * BAR, (r, Ts[i], shifts[i])


def _model(wtype, ctx):
    """synth.tiny with a prompt table a hundred times as large, as tests/test_gpu_parler_attention.py: the V rows of a cache are then no near copies of their mean"""
    m = synth.build(synth.tiny(ctx=ctx, prompt_vocab=5001, weight_type=wtype))
    t = m.by_name["decoder.embed_prompts"]
    t2 = gguf.Tensor.from_array(t.name, (t.to_f32().reshape(5001, H) * np.float32(100.0)).astype(np.float32), t.type)
    m.tensors[[x.name for x in m.tensors].index(t.name)] = t2
    m.by_name[t.name] = t2
    return m


@pytest.mark.parametrize("nsplit,fused", [(0, 1), (4, 1), (4, 0)], ids=["unsplit-and-8-slices", "4-slices-fused", "4-slices-combine"])
def test_attn_kernel_over_e4m3_rows(nsplit, fused, monkeypatch):
    """attn_kernel's e4m3 key pass: 16 key groups (255 and 40 rows), 64 key groups past their first pass of 256 keys (20 rows), in 8 slices folded by the last
    workgroup (5 rows), and under TTS_HIP_ATTN_NSPLIT = 4 with either fold"""
    if nsplit:
        monkeypatch.setenv("TTS_HIP_ATTN_NSPLIT", str(nsplit))
    monkeypatch.setenv("TTS_HIP_ATTN_ROWS", "4")     # no row-major reader over e4m3 rows: attn_kernel at every row count, whatever the threshold
    model = _model(gguf.F32, 320)
    eng = _engine(model, 1, dict(F8, **({} if fused else {"attn_fused": 0})), kv_positions=320)
    ids = np.random.default_rng(0x9A71).integers(3, 5001, 320).astype(np.uint32)
    p0 = 0
    for n in (255, 20, 5, 40):
        eng.prefill(0, ids[p0:p0 + n], p0)
        nkg = 64 if n == 20 and not nsplit else 16
        nz = nsplit or (8 if n == 5 else 1)
        _check(eng, list(range(p0, p0 + n)), [0] * n, lambda T: (nkg - 1, nkg, 4 * nkg - 1, 4 * nkg, -(-T // nz) - 1, -(-T // nz)))
        p0 += n
    eng.close()


# ---- 3. paths -----------------------------------------------------------------------------------------------------------------------------------
def test_captured_generation_and_session_equal_the_eager_step_loop():
    model = synth.build(synth.tiny(weight_type=gguf.F16))
    cfg, rng, n_steps = model.cfg, np.random.default_rng(3), 12
    prompts = [rng.integers(3, cfg.prompt_vocab, 2 + 3 * i).astype(np.uint32) for i in range(3)]
    eager = _engine(model, 3, F8, flags=hip.FLAG_NO_GRAPH)
    eager.prefill_batch(prompts)
    ids, want = np.full((3, cfg.n_out), cfg.bos, dtype=np.uint32), []
    for st in range(n_steps):
        tok = eager.step(ids, [len(p) + st for p in prompts], [0, 1, 2]).argmax(-1).astype(np.uint32)
        want.append(tok)
        ids = np.where(np.arange(cfg.n_out)[None, :] <= st, tok, cfg.bos).astype(np.uint32)
    eager.close()
    eng = _engine(model, 4, F8)      # (a session of 3 slots wants a spare cache slot)
    assert eng.debug_read("kv_elem", 1)[0] == 1
    eng.prefill_batch(prompts)
    toks, _ = eng.generate_greedy([len(p) for p in prompts], n_steps)
    assert np.array_equal(toks, np.stack(want))
    eng.reset()
    eng.stream_begin(3, n_steps)
    eng.stream_admit([0, 1, 2], prompts)
    done = dict(eng.stream_run(n_steps))
    for s in range(3):
        assert np.array_equal(eng.stream_collect(s, done[s]), np.stack(want)[:done[s], s])
    eng.stream_end()
    eng.stream_begin_mixed(3, n_steps)               # the same rows with a sampler record per slot (all greedy)
    eng.stream_admit_mixed([0, 1, 2], prompts, [None] * 3)
    done = dict(eng.stream_run(n_steps))
    for s in range(3):
        assert np.array_equal(eng.stream_collect(s, done[s]), np.stack(want)[:done[s], s])
    eng.stream_end()
    eng.prefill_batch(prompts)                       # gen_*: the captured loop in two launches
    u32p, got, ran = C.POINTER(C.c_uint32), np.zeros((n_steps, 3, cfg.n_out), dtype=np.uint32), C.c_uint32()
    eng._chk(eng.L.tts_hip_parler_gen_begin(eng.ctx, 3, np.array([len(p) for p in prompts], dtype=np.uint32).ctypes.data_as(u32p), n_steps, cfg.bos, cfg.eos, None, None))
    for n in (5, n_steps - 5):
        eng._chk(eng.L.tts_hip_parler_gen_launch(eng.ctx, n))
        eng._chk(eng.L.tts_hip_parler_gen_wait(eng.ctx, got.ctypes.data_as(u32p), None, C.byref(ran)))
    assert ran.value == n_steps and np.array_equal(got, np.stack(want))
    eng.close()


# ---- 4. selection -------------------------------------------------------------------------------------------------------------------------------
def test_selection(tmp_path, monkeypatch):
    model = synth.build(synth.tiny(weight_type=gguf.F16))
    for kv, esz in ((gguf.F32, 4), (gguf.F16, 2)):
        eng = hip.HipEngine(model.cfg, kv_type=kv)
        if kv == gguf.F16:
            with pytest.raises(hip.HipError, match="kv_f8.*TTS_HIP_F16"):
                eng.tune("kv_f8", 1)
        eng.load(model)
        assert eng.debug_read("kv_elem", 1)[0] == esz          # key off: as before
        with pytest.raises(hip.HipError, match="kv_f8 after tts_hip_finalize"):
            eng.tune("kv_f8", 1)
        eng.close()
    codec = hip.HipEngine(model.cfg, flags=hip.FLAG_NO_PARLER)
    with pytest.raises(hip.HipError, match="kv_f8 is the Parler decoder's key"):
        codec.tune("kv_f8", 1)
    codec.close()
    from tts_cpp_amd import runner
    path = model.write_gguf(str(tmp_path / "parler.gguf"))
    monkeypatch.delenv("TTS_HIP_KV_F16", raising=False)
    monkeypatch.setenv("TTS_HIP_PARLER_KV_F8", "1")
    r = runner.Runner(path, sample=0)
    assert r.kv_element_bytes() == 1
    r.close()
    monkeypatch.setenv("TTS_HIP_KV_F16", "1")
    with pytest.raises(runner.RunnerError, match=r"TTS_HIP_PARLER_KV_F8 and TTS_HIP_KV_F16"):
        runner.Runner(path, sample=0)
    monkeypatch.delenv("TTS_HIP_PARLER_KV_F8")
    r = runner.Runner(path, sample=0)
    assert r.kv_element_bytes() == 2                # key off: the fp16 cache as before
    r.close()


# ---- 5. cost of the format ----------------------------------------------------------------------------------------------------------------------
F8_ORACLE_BAR = 4 * 1.79e-2      # 4 x the largest e4m3 distance measured (docstring below), the project's rule for the Orpheus cache


def test_logits_against_the_fp32_cache_oracle():
    """The oracle keeps fp32 K/V, so this distance measures the format (three mantissa bits on every cached K and V), not the implementation (groups 1 and 2
    pin that).  The fp16-cache engine runs beside it under the bar the project holds an fp16 cache to (1e-2, tests/test_gpu_orpheus_kv_f16.py).
    Measured on MI355X, max|logits - ref| / max|ref| over the 8 steps:
      e4m3  1.79e-2 1.70e-2 1.52e-2 1.26e-2 1.41e-2 1.42e-2 1.42e-2 1.33e-2   -> bar 4 x 1.79e-2 = 7.16e-2
      fp16  6.77e-4 5.11e-4 4.82e-4 3.60e-4 4.27e-4 3.67e-4 4.73e-4 6.29e-4"""
    model = synth.build(synth.tiny(weight_type=gguf.F16))
    cfg = model.cfg
    engs = {"e4m3": hip.HipEngine(cfg, tune=F8), "fp16": hip.HipEngine(cfg, kv_type=gguf.F16)}      # with the cross-attention, as the oracle
    for e in engs.values():
        e.load(model)
    o = orc.ParlerOracle(model, act_mode=1, gelu_mode=1)
    prompt = np.random.default_rng(5).integers(3, cfg.prompt_vocab, 9).astype(np.uint32)
    o.decode(prompt, 0, audio=False, want_logits=False, want_hidden=True)
    for e in engs.values():
        e.prefill(0, prompt)
    ids, errs = np.full(cfg.n_out, cfg.bos, dtype=np.uint32), {k: [] for k in engs}
    for step in range(1, 9):
        pos = len(prompt) + step - 1
        ref = o.decode(ids, pos, audio=True)[0][:, 0, :]
        for k, e in engs.items():
            lg = e.step(ids[None], [pos])[0]
            errs[k].append(float(np.abs(lg - ref).max() / np.abs(ref).max()))
        toks = ref.argmax(-1).astype(np.uint32)      # teacher forcing with the oracle's ids
        ids = np.array([toks[i] if step > i else cfg.bos for i in range(cfg.n_out)], dtype=np.uint32)
    for k in engs:
        print(f"[parler kv {k}] logits against the fp32-cache oracle, 8 steps: " + " ".join(f"{x:.2e}" for x in errs[k]))
        engs[k].close()
    assert max(errs["fp16"]) < 1e-2, errs["fp16"]
    assert max(errs["e4m3"]) < F8_ORACLE_BAR, errs["e4m3"]
