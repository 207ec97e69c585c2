"""GPU: the opt-in fp16 K/V cache of an Orpheus context (TTS_HIP_FLAG_KV_F16, include/tts_hip.h).

1. the writers: what llama_rope_kv_kernel<_Float16> and gemv_q4_qkv_rope_kernel<4, 0 / 2, 2, _Float16> store is np.float16 of what their float instantiations store, bit for bit;
2. the readers: attn_gqa_kernel<128, false / true, _Float16> and attn_gqa_wave_kernel<128, 4, false, _Float16> against the float64 softmax . V of what the launch itself read, with
   the checker, the call tables and the bar of test_gpu_llama_attention (BAR = 6.44e-6 of max|ref|; the cache rows come back widened exactly, so the rounding
   of the cache is on both sides and nothing but the attention lies between the two numbers);
3. prompt + eight steps against the oracle, which keeps fp32 K/V, at the bar of the fp16-cache extension (1e-2, tests/test_gpu_parler.py);
4. the equalities the API promises, inside fp16 mode: captured step = eager step, lock-step batch = single generations, session = solo runs;
5. the runner's switch (TTS_HIP_KV_F16 in the environment at load); 6. the create calls that refuse the flag.

Measured on MI355X (printed under -s; DESIGN.md, "fp16 K/V cache of the Llama decoder"): kernel distances 0.9e-7 .. 4.8e-7 of max|ref| (bar 6.44e-6), least
boundary-key shift 1.97e-3 (bar 6.44e-5), logits against the oracle 3.8e-4 .. 6.7e-4 (bar 1e-2)."""
import numpy as np
import pytest

import oracle as orc
import test_gpu_llama_attention as ta
import test_gpu_orpheus_stream as ts
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

KVH = ta.NKV * ta.HD
F16 = hip.FLAG_KV_F16


def _tiny(wtype):
    """the tiny model of test_gpu_llama_attention with the matrices in wtype"""
    return synth.build_orpheus(synth.orpheus_tiny(hidden=512, heads=ta.NH, kv_heads=ta.NKV, layers=2, vocab=ta.VOCAB, ctx=ta.CTX, weight_type=wtype))


def _elem(eng):
    return int(eng.debug_read("l_kv_elem", 1)[0])


def _layer0(eng, slot=0):
    return tuple(eng.debug_read(f"l_{w}:0:{slot}", ta.CTX * KVH).reshape(ta.CTX, KVH) for w in "kv")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _assert_rounded(tag, e32, e16, written, slot=0):
    """layer 0 of slot `slot`: the fp16 engine's rows are np.float16 of the fp32 engine's for the written positions, every other row is zero in both"""
    for name, a, b in zip("KV", _layer0(e32, slot), _layer0(e16, slot)):
        w = np.zeros(ta.CTX, dtype=bool)
        w[list(written)] = True
        assert a[w].any(axis=1).all() and np.abs(a[w]).max() < 65504, tag       # every written row is there, inside the fp16 range
        assert _same_bits(b[w], a[w].astype(np.float16).astype(np.float32)), f"{tag}: {name} rows of slot {slot} are not the fp32 rows rounded to nearest-even"
        assert not a[~w].any() and not b[~w].any(), f"{tag}: an unwritten {name} row of slot {slot} is not zero"
        assert not _same_bits(b[w], a[w]), tag      # the rounding is live: these rows are not fp16 numbers to begin with


def _pair(model, tune=None, **kw):
    engines = []
    for flags in (0, F16):
        eng = hip.OrpheusEngine(model.cfg, flags=flags, **kw)
        for k, v in (tune or {}).items():
            eng.tune(k, v)
        eng.load(model)
        engines.append(eng)
    assert (_elem(engines[0]), _elem(engines[1])) == (4, 2)
    return engines


# ---- 1. the writers ---------------------------------------------------------------------------------------------------------------------
def test_rope_kv_kernel_stores_the_fp32_rows_rounded_once():
    """F16 matrices: a 255-row piece and two one-row steps, all through llama_rope_kv_kernel<float> / <_Float16>"""
    model, ids = _tiny(gguf.F16), ta._orpheus_ids()
    e32, e16 = _pair(model)
    for p0, n in ((0, 255), (255, 1), (256, 1)):
        for eng in (e32, e16):
            eng.decode(ids[p0:p0 + n], p0)
    _assert_rounded("rope_kv", e32, e16, range(257))
    e32.close(); e16.close()


@pytest.mark.parametrize("q4_rms", [1, 0])
def test_fused_q4_projection_stores_the_fp32_rows_rounded_once(q4_rms):
    """Q4_0 matrices, calls of 3, 1, 1 and 3 rows: gemv_q4_qkv_rope_kernel<4, 2, 2, KV> (the rms norm in its staging) and <4, 0, 2, KV> (q4_rms off), KV = float against _Float16"""
    model, ids = _tiny(gguf.Q4_0), ta._orpheus_ids()
    e32, e16 = _pair(model, tune={"q4_rms": q4_rms})
    for p0, n in ((0, 3), (3, 1), (4, 1), (5, 3)):
        for eng in (e32, e16):
            eng.decode(ids[p0:p0 + n], p0)
    _assert_rounded(f"q4 qkv rope, q4_rms={q4_rms}", e32, e16, range(8))
    e32.close(); e16.close()


def test_lockstep_rows_append_to_their_own_slots():
    """three cache slots fed through step_batch alone, ragged (2, 5 and 9 positions): llama_rope_kv_kernel's row_seq addressing with the slot stride in elements"""
    model = _tiny(gguf.F16)
    rng = np.random.default_rng(0x516)
    lens = [2, 5, 9]
    seqs = [rng.integers(0, ta.VOCAB, n).astype(np.uint32) for n in lens]
    e32, e16 = _pair(model, max_seqs=3)
    for t in range(max(lens)):
        slots = [s for s in range(3) if lens[s] > t]
        for eng in (e32, e16):
            eng.step_batch(slots, [int(seqs[s][t]) for s in slots], [t] * len(slots), want_logits=False)
    for s in range(3):
        _assert_rounded("lock-step", e32, e16, range(lens[s]), slot=s)
    e32.close(); e16.close()


# ---- 2. the readers against float64 -----------------------------------------------------------------------------------------------------
def _engine(model, **kw):
    eng = hip.OrpheusEngine(model.cfg, flags=F16, **kw)
    return eng


def _sequence(wave):
    """test_gpu_llama_attention._orpheus_sequence on the fp16 cache"""
    model, ids = ta._orpheus_model(), ta._orpheus_ids()
    eng = _engine(model)
    eng.tune("attn_wave", wave)
    eng.load(model)
    assert _elem(eng) == 2
    log, failures = [], []
    for p0, n in ta.ORPHEUS_CALLS:
        eng.decode(ids[p0:p0 + n], p0)
        q, out, pos, caches = ta._orpheus_read(eng, n)
        assert pos.tolist() == list(range(p0, p0 + n))
        nz = ta._plan(n, p0 + n)
        kernel = "unsplit" if nz == 1 else ("wave" if wave else "split")
        if n == 1:
            assert nz == ta.ONE_ROW_NZ[p0]
        K, V = caches[0]
        assert _same_bits(K, K.astype(np.float16).astype(np.float32)) and _same_bits(V, V.astype(np.float16).astype(np.float32))      # fp16 numbers, widened exactly
        try:
            ta._check(f"orpheus f16 kv eager wave={wave} pos {p0}..{p0 + n - 1}", kernel, nz, q, out, [(int(p) + 1, K, V) for p in pos], ta.SCALE, ta.NKV, log)
        except AssertionError as e:      # go on: the later calls read caches this one did not write wrongly
            failures.append(str(e))
    eng.close()
    return log, failures


@pytest.mark.parametrize("wave", [1, 0])
def test_f16_cache_eager_decode_ascending_through_the_cache(wave):
    """ORPHEUS_CALLS up to position 1060.  The multi-row pieces take attn_gqa_kernel<128, false, _Float16>; the one-row, 3-row and 20-row calls take
    attn_gqa_wave_kernel<128, 4, false, _Float16> (wave=1) or attn_gqa_kernel<128, true, _Float16> (wave=0) at the nz of ONE_ROW_NZ, then attn_gqa_combine_kernel"""
    log, failures = _sequence(wave)
    assert len(log) == len(ta.ORPHEUS_CALLS)
    want = "wave" if wave else "split"
    for p0, nz in ta.ONE_ROW_NZ.items():
        e = ta._entry(log, p0, 1)
        assert (e["kernel"], e["nz"]) == (want, nz)
    assert (ta._entry(log, 641, 3)["kernel"], ta._entry(log, 641, 3)["nz"]) == (want, 5)
    assert (ta._entry(log, 644, 20)["kernel"], ta._entry(log, 644, 20)["nz"]) == (want, 3)
    assert ta._entry(log, 500, 100)["kernel"] == "unsplit" and ta._entry(log, 500, 100)["keys"] == (501, 600)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("split", [8, 3])
@pytest.mark.parametrize("n_prompt,max_new,T", [(3, 2, 4), (509, 5, 513), (600, 3, 602)])
def test_f16_cache_captured_step(n_prompt, max_new, T, split):
    """the last replay of the captured step (attn_gqa_wave_kernel<128, 4, false, _Float16> at a fixed split count), as test_orpheus_captured_step reads it"""
    model, ids = ta._orpheus_model(), ta._orpheus_ids()
    eng = _engine(model)
    eng.tune("attn_split", split)
    eng.load(model)
    toks = eng.generate_greedy(ids[:n_prompt], max_new, stop_id=ta.VOCAB + 5)
    assert len(toks) == max_new and _elem(eng) == 2
    q, out, pos, caches = ta._orpheus_read(eng, 1)
    assert int(pos[0]) == T
    K, V = caches[0]
    ta._check(f"orpheus f16 kv captured split={split} prompt {n_prompt}", "wave", split, q, out, [(int(pos[0]), K, V)], ta.SCALE, ta.NKV, [])
    eng.close()


def test_f16_cache_lockstep_rows_with_their_own_slots():
    """four utterances of 2, 70, 333 and 600 prompt ids, one lock-step step: attn_gqa_kernel<128, true, _Float16> with row_seq and the slot stride, nz = 4"""
    model = ta._orpheus_model()
    rng = np.random.default_rng(0x10C)
    lens = [2, 70, 333, 600]
    prompts = [rng.integers(0, ta.VOCAB, n).astype(np.uint32) for n in lens]
    eng = _engine(model, max_seqs=4)
    eng.load(model)
    first = eng.generate_batch(prompts, 1, stop_id=ta.VOCAB + 5)
    slots = [0, 1, 2, 3]
    eng.step_batch(slots, [int(f[0]) for f in first], lens, want_logits=False)
    q, out, pos, caches = ta._orpheus_read(eng, 4, slot_of=slots)
    assert pos.tolist() == lens and _elem(eng) == 2
    nz = ta._plan(4, max(lens) + 1)
    assert nz == 4
    ta._check("orpheus f16 kv lock-step 4 slots", "split", nz, q, out, [(int(p) + 1,) + caches[s] for p, s in zip(pos, slots)], ta.SCALE, ta.NKV, [])
    eng.close()


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------------
def test_f16_cache_prompt_and_steps_against_the_oracle():
    """the oracle keeps fp32 K/V: the bar is the one of Parler's fp16 cache (tests/test_gpu_parler.py, "F16 KV cache (extension)")"""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=gguf.F16))
    eng = _engine(model)
    eng.load(model)
    o = orc.OrpheusOracle(model, act_mode=1)
    rng = np.random.default_rng(0xE2E)
    prompt = rng.integers(0, model.cfg.vocab, 9).astype(np.uint32)
    lg, _ = eng.decode(prompt, 0)
    ref = o.decode(prompt, 0)
    errs = [float(np.abs(lg - ref).max() / np.abs(ref).max())]
    pos = len(prompt)
    for _ in range(8):
        t = int(ref.argmax())           # teacher forcing with the oracle's id
        lg, _ = eng.decode([t], pos)
        ref = o.decode([t], pos)
        errs.append(float(np.abs(lg - ref).max() / np.abs(ref).max()))
        pos += 1
    print("[kv f16] logits against the fp32-cache oracle, prompt + 8 steps: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-2, errs
    eng.close()


# ---- 4. the equalities of the API, inside fp16 mode -------------------------------------------------------------------------------------
def test_f16_cache_captured_step_equals_the_eager_step():
    """test_orpheus_greedy_through_the_captured_step's model, prompt and lengths: the captured graph against the eager loop, both on the fp16 cache"""
    import os
    model = synth.build_orpheus(synth.orpheus_tiny())
    prompt = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_orpheus.npz"))["prompt"]
    never = model.cfg.vocab + 5
    eager = ts._eager_engine(model.cfg, flags=F16)
    eager.load(model)
    captured = _engine(model)
    captured.load(model)
    for n in (6, 40):
        a, b = eager.generate_greedy(prompt, n, stop_id=never).tolist(), captured.generate_greedy(prompt, n, stop_id=never).tolist()
        assert len(a) == n and a == b, n
    eager.close(); captured.close()


SMP8 = dict(top_k=8, temperature=0.9, repetition_penalty=1.2)


def _solo(model, prompts, uni):
    """the eager one-sequence engine on the fp16 cache: greedy, greedy with a stop id that some meet early, and sampled ids per prompt"""
    cfg = model.cfg
    never = cfg.vocab + ts.NEVER
    single = ts._eager_engine(cfg, flags=F16)
    single.load(model)
    greedy = [single.generate_greedy(p, ts.MAX_NEW, stop_id=never).tolist() for p in prompts]
    stop = int(greedy[1][5])
    stopped = [single.generate_greedy(p, ts.MAX_NEW, stop_id=stop).tolist() for p in prompts]
    sampled = [single.generate_sampled(p, ts.MAX_NEW, stop_id=never, uniforms=uni[u], **SMP8).tolist() for u, p in enumerate(prompts)]
    single.close()
    return stop, greedy, stopped, sampled


@pytest.mark.parametrize("wtype", [gguf.F16, gguf.Q4_0])
def test_f16_cache_lockstep_batch_equals_single_generations(wtype):
    """test_orpheus_lockstep_batch_equals_single_sequence_generations at 3 utterances (its prompts and seed), every engine on the fp16 cache"""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=wtype))
    cfg = model.cfg
    rng = np.random.default_rng(10 * 3 + wtype)
    prompts = [rng.integers(0, cfg.vocab, 3 + 2 * (u % 4)).astype(np.uint32) for u in range(3)]
    uni = rng.random((3, ts.MAX_NEW), dtype=np.float32)
    stop, greedy, stopped, sampled = _solo(model, prompts, uni)
    never = cfg.vocab + ts.NEVER
    eng = _engine(model, max_seqs=3)
    eng.load(model)
    assert [g.tolist() for g in eng.generate_batch(prompts, ts.MAX_NEW, stop_id=never)] == greedy
    assert [g.tolist() for g in eng.generate_batch(prompts, ts.MAX_NEW, stop_id=stop)] == stopped
    assert [g.tolist() for g in eng.generate_batch(prompts, ts.MAX_NEW, stop_id=never, uniforms=uni, **SMP8)] == sampled
    assert eng.generate_greedy(prompts[0], ts.MAX_NEW, stop_id=never).tolist() == greedy[0]      # slot 0 through the one-sequence entry point
    eng.close()


@pytest.mark.parametrize("wtype", [gguf.F16, gguf.Q4_0])
def test_f16_cache_session_equals_solo_runs(wtype):
    """test_session_equals_one_sequence_generations at 3 slots (7 utterances, its prompts and schedule): utterances admitted beside others in mid-generation
    into reused slots give the ids of their solo runs, greedy and sampled"""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=wtype))
    cfg = model.cfg
    rng = np.random.default_rng(10 * 3 + wtype)
    prompts = [rng.integers(0, cfg.vocab, 3 + 2 * (u % 4)).astype(np.uint32) for u in range(7)]
    uni = rng.random((7, ts.MAX_NEW), dtype=np.float32)
    stop, greedy, stopped, sampled = _solo(model, prompts, uni)
    never = cfg.vocab + ts.NEVER
    eng = _engine(model, max_seqs=3)
    eng.load(model)
    got, facts = ts._run_session(eng, prompts, 3, 5, never)
    assert got == greedy and facts["slot_twice"] and facts["runs"] > 1, facts
    assert len({len(r) for r in stopped}) > 1      # ends in the middle of a run: new utterances meet rows in mid-generation
    got, facts = ts._run_session(eng, prompts, 3, 5, stop)
    assert got == stopped and facts["mid_flight"], facts
    got, facts = ts._run_session(eng, prompts, 3, 1, never, uniforms=uni, **SMP8)
    assert got == sampled and facts["slot_twice"], facts
    eng.close()


# ---- 5. the runner ----------------------------------------------------------------------------------------------------------------------
TEXTS = ["hello the zebra", "a zebra", "the quick hello of the zebra there"]


def test_runner_reads_the_switch_at_load(tmp_path, monkeypatch):
    """TTS_HIP_KV_F16 in the environment when the runner is loaded -> the decoder context reports 2-byte cache elements, and generate / generate_batch /
    generate_stream give every text the same audio (SNAC of the same ids, noise block off); without the variable the context reports 4"""
    from tts_cpp_amd import runner
    path = synth.SynthOrpheusFull(max_gen=28).write_gguf(str(tmp_path / "orpheus.gguf"))
    monkeypatch.setenv("TTS_SNAC_NO_NOISE", "1")
    monkeypatch.delenv("TTS_HIP_KV_F16", raising=False)
    plain = runner.Runner(path, sample=0)
    assert plain.kv_element_bytes() == 4
    plain.close()
    monkeypatch.setenv("TTS_HIP_KV_F16", "1")
    one = runner.Runner(path, sample=0)
    many = runner.Runner(path, sample=0, max_seqs=4)
    monkeypatch.delenv("TTS_HIP_KV_F16")         # read at load: the loaded runners keep their cache type
    assert (one.kv_element_bytes(), many.kv_element_bytes()) == (2, 2)
    compared = 0
    for kw in (dict(sample=0), dict(sample=1, top_k=8, seed=3)):
        try:
            singles = [one.generate(t, voice=b"zoe", **kw) for t in TEXTS]
        except runner.RunnerError as e:          # random weights may sample a text id where an audio id belongs
            assert "codebook size" in str(e)
            continue
        for got in (many.generate_batch(TEXTS, voice=b"zoe", **kw), many.generate_stream(TEXTS, voice=b"zoe", **kw)):
            assert len(got) == len(TEXTS)
            for a, b in zip(singles, got):
                assert a.size > 0 and np.array_equal(a, b), kw
        compared += 1
    assert compared >= 1
    one.close(); many.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_other_create_calls_refuse_the_flag():
    pcfg = synth.tiny(weight_type=gguf.F16)
    with pytest.raises(hip.HipError, match=r"tts_hip_create: TTS_HIP_FLAG_KV_F16"):
        hip.HipEngine(pcfg, flags=F16)
    hip.HipEngine(pcfg).close()                                        # a valid create works afterwards
    dcfg = synth.dia_tiny()
    with pytest.raises(hip.HipError, match=r"tts_hip_dia_create: TTS_HIP_FLAG_KV_F16"):
        hip.DiaEngine(dcfg, flags=F16)
    hip.DiaEngine(dcfg).close()
