"""GPU: the opt-in e4m3 K/V cache of an Orpheus context (tts_hip_orpheus_desc::kv_type = TTS_HIP_KV_F8_E4M3, include/tts_hip.h).  Section by section the
file of the fp16 cache (test_gpu_orpheus_kv_f16.py), at its shapes and with its prompts and seeds.

1. the writers: what llama_rope_kv_kernel<kv_f8> and gemv_q4_qkv_rope_kernel<4, 0 / 2, 2, kv_f8> store is e4m3_round (tests/e4m3_reference.py: clamp to
   +-448, nearest-even at 3 mantissa bits, exponent floor -6) of what their float instantiations store, bit for bit — also where K and V exceed 448;
2. the readers: attn_gqa_kernel<128, false / true, kv_f8> and attn_gqa_wave_kernel<128, 4, false, kv_f8> against the float64 softmax . V of what the launch
   itself read, with the checker, the call tables and the bar of test_gpu_llama_attention (BAR = 6.44e-6 of max|ref|; the cache rows come back widened
   exactly, so the rounding of the cache is on both sides and nothing but the attention lies between the two numbers), and one step of 66 rows;
3. the equalities the API promises, inside e4m3 mode: captured step = eager step, lock-step batch = single generations, session = solo runs;
4. prompt + eight steps against the oracle, which keeps fp32 K/V: this distance measures the format, not the implementation (1 - 3 pin that);
5. the runner's switch (TTS_HIP_KV_F8 in the environment at load); 6. what the create calls refuse, and the descriptor of the size before kv_type.

Measured on MI355X (printed under -s; DESIGN.md, "fp8 (e4m3) K/V cache of the Llama decoder"): kernel distances 0.98e-7 .. 5.0e-7 of max|ref| (bar 6.44e-6), least
boundary-key shift 1.98e-3 (bar 6.44e-5), logits against the oracle 1.6e-2 .. 2.6e-2 (bar 1.04e-1; the fp16 cache in the same test: 3.8e-4 .. 6.7e-4)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
import test_gpu_llama_attention as ta
import test_gpu_orpheus_stream as ts
from e4m3_reference import e4m3_round
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

KVH = ta.NKV * ta.HD
F8 = getattr(hip, "KV_F8_E4M3", None)      # (None: a tree without the e4m3 cache — every test below fails at its first engine)


def _tiny(wtype, **kw):
    """the tiny model of test_gpu_llama_attention with the matrices in wtype"""
    return synth.build_orpheus(synth.orpheus_tiny(hidden=512, heads=ta.NH, kv_heads=ta.NKV, layers=2, vocab=ta.VOCAB, ctx=ta.CTX, weight_type=wtype, **kw))


def _elem(eng):
    return int(eng.debug_read("l_kv_elem", 1)[0])


def _layer0(eng, slot=0):
    return tuple(eng.debug_read(f"l_{w}:0:{slot}", ta.CTX * KVH).reshape(ta.CTX, KVH) for w in "kv")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _is_e4m3(a):
    return _same_bits(a, e4m3_round(a))


def _assert_rounded(tag, e32, e8, written, slot=0, saturating=False):
    """layer 0 of slot `slot`: the e4m3 engine's rows are e4m3_round of the fp32 engine's for the written positions, every other row is zero in both"""
    for name, a, b in zip("KV", _layer0(e32, slot), _layer0(e8, slot)):
        w = np.zeros(ta.CTX, dtype=bool)
        w[list(written)] = True
        assert a[w].any(axis=1).all() and np.isfinite(a[w]).all(), tag      # every written row is there
        big = np.abs(a[w]) > 448
        if saturating:      # some magnitudes beyond the format's range, most inside it
            assert big.any() and big.mean() < 0.05, (tag, name, float(big.mean()))
            assert np.isfinite(b[w]).all() and np.array_equal(b[w][big], np.copysign(np.float32(448), a[w][big])), f"{tag}: {name} beyond 448 is not stored as +-448"
        else:
            assert not big.any(), tag
        assert _same_bits(b[w], e4m3_round(a[w])), f"{tag}: {name} rows of slot {slot} are not the fp32 rows rounded to e4m3, nearest-even"
        assert not a[~w].any() and not b[~w].any(), f"{tag}: an unwritten {name} row of slot {slot} is not zero"
        assert not _same_bits(b[w], a[w]), tag      # the rounding is live: these rows are not e4m3 numbers to begin with


def _pair(model, tune=None, **kw):
    engines = []
    for kv_type in (0, F8):
        eng = hip.OrpheusEngine(model.cfg, kv_type=kv_type, **kw)
        for k, v in (tune or {}).items():
            eng.tune(k, v)
        eng.load(model)
        engines.append(eng)
    assert (_elem(engines[0]), _elem(engines[1])) == (4, 1)
    return engines


# ---- 1. the writers ---------------------------------------------------------------------------------------------------------------------
def test_rope_kv_kernel_stores_the_fp32_rows_rounded_once():
    """F16 matrices: a 255-row piece and two one-row steps, all through llama_rope_kv_kernel<float> / <kv_f8>"""
    model, ids = _tiny(gguf.F16), ta._orpheus_ids()
    e32, e8 = _pair(model)
    for p0, n in ((0, 255), (255, 1), (256, 1)):
        for eng in (e32, e8):
            eng.decode(ids[p0:p0 + n], p0)
    _assert_rounded("rope_kv", e32, e8, range(257))
    e32.close(); e8.close()


@pytest.mark.parametrize("q4_rms", [1, 0])
def test_fused_q4_projection_stores_the_fp32_rows_rounded_once(q4_rms):
    """Q4_0 matrices, calls of 3, 1, 1 and 3 rows: gemv_q4_qkv_rope_kernel<4, 2, 2, KV> (the rms norm in its staging) and <4, 0, 2, KV> (q4_rms off), KV = float against kv_f8"""
    model, ids = _tiny(gguf.Q4_0), ta._orpheus_ids()
    e32, e8 = _pair(model, tune={"q4_rms": q4_rms})
    for p0, n in ((0, 3), (3, 1), (4, 1), (5, 3)):
        for eng in (e32, e8):
            eng.decode(ids[p0:p0 + n], p0)
    _assert_rounded(f"q4 qkv rope, q4_rms={q4_rms}", e32, e8, range(8))
    e32.close(); e8.close()


def test_lockstep_rows_append_to_their_own_slots():
    """three cache slots fed through step_batch alone, ragged (2, 5 and 9 positions): llama_rope_kv_kernel's row_seq addressing with the slot stride in elements"""
    model = _tiny(gguf.F16)
    rng = np.random.default_rng(0x516)
    lens = [2, 5, 9]
    seqs = [rng.integers(0, ta.VOCAB, n).astype(np.uint32) for n in lens]
    e32, e8 = _pair(model, max_seqs=3)
    for t in range(max(lens)):
        slots = [s for s in range(3) if lens[s] > t]
        for eng in (e32, e8):
            eng.step_batch(slots, [int(seqs[s][t]) for s in slots], [t] * len(slots), want_logits=False)
    for s in range(3):
        _assert_rounded("lock-step", e32, e8, range(lens[s]), slot=s)
    e32.close(); e8.close()


# layer 0's K and V are projections of unit-variance rows by matrices of standard deviation kv_gain / sqrt(hidden): about N(0, kv_gain^2).  150 puts 448 at
# three standard deviations: some thousandths of the elements beyond it, the rest inside
KV_GAIN = 150.0


@pytest.mark.parametrize("wtype", [gguf.F16, gguf.Q4_0])
def test_writers_saturate_at_448(wtype):
    """both writers (F16 matrices: llama_rope_kv_kernel; Q4_0: gemv_q4_qkv_rope_kernel) on a model whose layer-0 K and V partly exceed the e4m3 range: stored as
    +-448, never NaN, and e4m3_round everywhere"""
    model, ids = _tiny(wtype, kv_gain=KV_GAIN), ta._orpheus_ids()
    e32, e8 = _pair(model)
    for p0, n in ((0, 3), (3, 1), (4, 20)):
        for eng in (e32, e8):
            eng.decode(ids[p0:p0 + n], p0)
    _assert_rounded(f"saturation, wtype {wtype}", e32, e8, range(24), saturating=True)
    e32.close(); e8.close()


# ---- 2. the readers against float64 -----------------------------------------------------------------------------------------------------
def _engine(model, **kw):
    return hip.OrpheusEngine(model.cfg, kv_type=F8, **kw)


def _sequence(wave):
    """test_gpu_llama_attention._orpheus_sequence on the e4m3 cache"""
    model, ids = ta._orpheus_model(), ta._orpheus_ids()
    eng = _engine(model)
    eng.tune("attn_wave", wave)
    eng.load(model)
    assert _elem(eng) == 1
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
        assert _is_e4m3(K) and _is_e4m3(V)      # e4m3 numbers, widened exactly
        try:
            ta._check(f"orpheus f8 kv eager wave={wave} pos {p0}..{p0 + n - 1}", kernel, nz, q, out, [(int(p) + 1, K, V) for p in pos], ta.SCALE, ta.NKV, log)
        except AssertionError as e:      # go on: the later calls read caches this one did not write wrongly
            failures.append(str(e))
    eng.close()
    return log, failures


@pytest.mark.parametrize("wave", [1, 0])
def test_f8_cache_eager_decode_ascending_through_the_cache(wave):
    """ORPHEUS_CALLS up to position 1060.  The multi-row pieces take attn_gqa_kernel<128, false, kv_f8>; the one-row, 3-row and 20-row calls take
    attn_gqa_wave_kernel<128, 4, false, kv_f8> (wave=1) or attn_gqa_kernel<128, true, kv_f8> (wave=0) at the nz of ONE_ROW_NZ, then attn_gqa_combine_kernel"""
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
def test_f8_cache_captured_step(n_prompt, max_new, T, split):
    """the last replay of the captured step (attn_gqa_wave_kernel<128, 4, false, kv_f8> at a fixed split count), as test_orpheus_captured_step reads it"""
    model, ids = ta._orpheus_model(), ta._orpheus_ids()
    eng = _engine(model)
    eng.tune("attn_split", split)
    eng.load(model)
    toks = eng.generate_greedy(ids[:n_prompt], max_new, stop_id=ta.VOCAB + 5)
    assert len(toks) == max_new and _elem(eng) == 1
    q, out, pos, caches = ta._orpheus_read(eng, 1)
    assert int(pos[0]) == T
    K, V = caches[0]
    assert _is_e4m3(K) and _is_e4m3(V)
    ta._check(f"orpheus f8 kv captured split={split} prompt {n_prompt}", "wave", split, q, out, [(int(pos[0]), K, V)], ta.SCALE, ta.NKV, [])
    eng.close()


def test_f8_cache_lockstep_rows_with_their_own_slots():
    """four utterances of 2, 70, 333 and 600 prompt ids, one lock-step step: attn_gqa_kernel<128, true, kv_f8> with row_seq and the slot stride, nz = 4"""
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
    assert pos.tolist() == lens and _elem(eng) == 1
    assert all(_is_e4m3(x) for kv in caches.values() for x in kv)
    nz = ta._plan(4, max(lens) + 1)
    assert nz == 4
    ta._check("orpheus f8 kv lock-step 4 slots", "split", nz, q, out, [(int(p) + 1,) + caches[s] for p, s in zip(pos, slots)], ta.SCALE, ta.NKV, [])
    eng.close()


def test_f8_cache_step_of_66_rows():
    """a context of more than 64 slots (as test_gpu_orpheus_many_rows builds them), one lock-step step of 66 rows with ragged histories: 66 x 4 (head, row)
    pairs are more than the split form takes, so the step runs attn_gqa_kernel<128, false, kv_f8> with row_seq.  Slot 0 has read 130 ids and slot 1 has 65
    (more than one 64-key batch), slot 2 exactly 64, the others 2 .. 31; the last row sits at position 0 of a slot without history: exactly 1 key"""
    model = ta._orpheus_model()
    B = 66
    rng = np.random.default_rng(0x42F8)
    lens = [130, 65, 64] + [2 + (u * 7) % 30 for u in range(3, B - 1)]
    prompts = [rng.integers(0, ta.VOCAB, n).astype(np.uint32) for n in lens]
    eng = _engine(model, max_seqs=B)
    eng.load(model)
    first = eng.generate_batch(prompts, 1, stop_id=ta.VOCAB + 5)
    slots = list(range(B))
    ids = [int(f[0]) for f in first] + [int(rng.integers(0, ta.VOCAB))]
    eng.step_batch(slots, ids, lens + [0], want_logits=False)
    q, out, pos, caches = ta._orpheus_read(eng, B, slot_of=slots)
    assert pos.tolist() == lens + [0] and _elem(eng) == 1
    assert all(_is_e4m3(x) for kv in caches.values() for x in kv)
    assert ta._plan(B, max(lens) + 1) == 1
    keys = [int(p) + 1 for p in pos]
    assert max(keys) > 64 and keys[-1] == 1
    ta._check("orpheus f8 kv lock-step 66 slots", "unsplit", 1, q, out, [(keys[r],) + caches[s] for r, s in enumerate(slots)], ta.SCALE, ta.NKV, [])
    eng.close()


# ---- 3. the equalities of the API, inside e4m3 mode -------------------------------------------------------------------------------------
def test_f8_cache_captured_step_equals_the_eager_step():
    """test_orpheus_greedy_through_the_captured_step's model, prompt and lengths: the captured graph against the eager loop, both on the e4m3 cache"""
    model = synth.build_orpheus(synth.orpheus_tiny())
    prompt = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_orpheus.npz"))["prompt"]
    never = model.cfg.vocab + 5
    eager = ts._eager_engine(model.cfg, kv_type=F8)
    eager.load(model)
    captured = _engine(model)
    captured.load(model)
    assert (_elem(eager), _elem(captured)) == (1, 1)
    for n in (6, 40):
        a, b = eager.generate_greedy(prompt, n, stop_id=never).tolist(), captured.generate_greedy(prompt, n, stop_id=never).tolist()
        assert len(a) == n and a == b, n
    eager.close(); captured.close()


SMP8 = dict(top_k=8, temperature=0.9, repetition_penalty=1.2)


def _solo(model, prompts, uni):
    """the eager one-sequence engine on the e4m3 cache: greedy, greedy with a stop id that some meet early, and sampled ids per prompt"""
    cfg = model.cfg
    never = cfg.vocab + ts.NEVER
    single = ts._eager_engine(cfg, kv_type=F8)
    single.load(model)
    assert _elem(single) == 1
    greedy = [single.generate_greedy(p, ts.MAX_NEW, stop_id=never).tolist() for p in prompts]
    stop = int(greedy[1][5])
    stopped = [single.generate_greedy(p, ts.MAX_NEW, stop_id=stop).tolist() for p in prompts]
    sampled = [single.generate_sampled(p, ts.MAX_NEW, stop_id=never, uniforms=uni[u], **SMP8).tolist() for u, p in enumerate(prompts)]
    single.close()
    return stop, greedy, stopped, sampled


@pytest.mark.parametrize("wtype", [gguf.F16, gguf.Q4_0])
def test_f8_cache_lockstep_batch_equals_single_generations(wtype):
    """test_orpheus_lockstep_batch_equals_single_sequence_generations at 3 utterances (its prompts and seed), every engine on the e4m3 cache"""
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
def test_f8_cache_session_equals_solo_runs(wtype):
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


# ---- 4. against the fp32-cache oracle ---------------------------------------------------------------------------------------------------
F8_ORACLE_BAR = 4 * 2.61e-2      # 4 x the largest e4m3 distance measured (docstring below): the margin this project's bars take over their measured value


def test_f8_cache_prompt_and_steps_against_the_oracle():
    """The oracle keeps fp32 K/V, so this distance is the cost of the format (three mantissa bits on every cached K and V), not of the implementation.
    The fp16 engine runs beside it under its own bar (1e-2, test_gpu_orpheus_kv_f16.py): the harness of the test is sound.

    Measured on MI355X, max|logits - ref| / max|ref| for the prompt pass and the 8 steps:
      e4m3  2.03e-2 2.15e-2 2.20e-2 2.41e-2 1.67e-2 1.57e-2 2.61e-2 2.48e-2 2.31e-2   -> bar 4 x 2.61e-2 = 1.04e-1 (other ids, other positions)
      fp16  5.52e-4 4.28e-4 4.96e-4 6.65e-4 4.49e-4 3.85e-4 3.78e-4 6.74e-4 3.92e-4   (bar 1e-2)
    forty times the fp16 cache's distance: the price of the format on random weights.  No real checkpoint is at hand, so nothing is known about audible quality."""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=gguf.F16))
    e8 = _engine(model)
    e16 = hip.OrpheusEngine(model.cfg, flags=hip.FLAG_KV_F16)
    for eng in (e8, e16):
        eng.load(model)
    assert (_elem(e8), _elem(e16)) == (1, 2)
    o = orc.OrpheusOracle(model, act_mode=1)
    rng = np.random.default_rng(0xE2E)
    prompt = rng.integers(0, model.cfg.vocab, 9).astype(np.uint32)
    ref = o.decode(prompt, 0)
    errs = {8: [], 16: []}
    for bits, eng in ((8, e8), (16, e16)):
        lg, _ = eng.decode(prompt, 0)
        errs[bits].append(float(np.abs(lg - ref).max() / np.abs(ref).max()))
    pos = len(prompt)
    for _ in range(8):
        t = int(ref.argmax())           # teacher forcing with the oracle's id
        ref = o.decode([t], pos)
        for bits, eng in ((8, e8), (16, e16)):
            lg, _ = eng.decode([t], pos)
            errs[bits].append(float(np.abs(lg - ref).max() / np.abs(ref).max()))
        pos += 1
    for bits in (8, 16):
        print(f"[kv f{bits}] logits against the fp32-cache oracle, prompt + 8 steps: " + " ".join(f"{e:.2e}" for e in errs[bits]))
    assert max(errs[16]) < 1e-2, errs[16]
    assert max(errs[8]) < F8_ORACLE_BAR, errs[8]
    e8.close(); e16.close()


# ---- 5. the runner ----------------------------------------------------------------------------------------------------------------------
TEXTS = ["hello the zebra", "a zebra", "the quick hello of the zebra there"]


def test_runner_reads_the_switch_at_load(tmp_path, monkeypatch):
    """TTS_HIP_KV_F8 in the environment when the runner is loaded -> the decoder context reports 1-byte cache elements, and generate / generate_batch /
    generate_stream give every text the same audio (SNAC of the same ids, noise block off); without the variable the context reports 4; with
    TTS_HIP_KV_F16 beside it the load fails and names both"""
    from tts_cpp_amd import runner
    path = synth.SynthOrpheusFull(max_gen=28).write_gguf(str(tmp_path / "orpheus.gguf"))
    monkeypatch.setenv("TTS_SNAC_NO_NOISE", "1")
    monkeypatch.delenv("TTS_HIP_KV_F16", raising=False)
    monkeypatch.delenv("TTS_HIP_KV_F8", raising=False)
    plain = runner.Runner(path, sample=0)
    assert plain.kv_element_bytes() == 4
    plain.close()
    monkeypatch.setenv("TTS_HIP_KV_F8", "1")
    monkeypatch.setenv("TTS_HIP_KV_F16", "1")
    with pytest.raises(runner.RunnerError, match=r"(?s)TTS_HIP_KV_F16.*TTS_HIP_KV_F8|TTS_HIP_KV_F8.*TTS_HIP_KV_F16"):
        runner.Runner(path, sample=0)
    monkeypatch.delenv("TTS_HIP_KV_F16")
    one = runner.Runner(path, sample=0)
    many = runner.Runner(path, sample=0, max_seqs=4)
    monkeypatch.delenv("TTS_HIP_KV_F8")         # read at load: the loaded runners keep their cache type
    assert (one.kv_element_bytes(), many.kv_element_bytes()) == (1, 1)
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


def test_parler_and_dia_runners_refuse_the_switch_at_load(tmp_path, monkeypatch):
    """they have no fp8 cache: with TTS_HIP_KV_F8 set the load fails and names the variable instead of running on an fp32 cache; without it the same files load"""
    from tts_cpp_amd import runner
    paths = [synth.build(synth.tiny(weight_type=gguf.F16)).write_gguf(str(tmp_path / "parler.gguf")),
             synth.build_dia(synth.dia_tiny(max_gen=64), suppress_special=True).write_gguf(str(tmp_path / "dia.gguf"))]
    monkeypatch.delenv("TTS_HIP_KV_F16", raising=False)
    for path in paths:
        monkeypatch.setenv("TTS_HIP_KV_F8", "1")
        with pytest.raises(runner.RunnerError, match="TTS_HIP_KV_F8"):
            runner.Runner(path, sample=0)
        monkeypatch.delenv("TTS_HIP_KV_F8")
        runner.Runner(path, sample=0).close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
class _DescBeforeKvType(C.Structure):
    """tts_hip_orpheus_desc as callers built before kv_type was appended know it"""
    _fields_ = [f for f in hip.OrpheusDesc._fields_ if f[0] != "kv_type"]


def test_create_refuses_what_it_cannot_serve_and_takes_the_earlier_descriptor():
    cfg = synth.orpheus_tiny()
    with pytest.raises(hip.HipError, match=r"tts_hip_orpheus_create: kv_type 7 "):
        hip.OrpheusEngine(cfg, kv_type=7)
    hip.OrpheusEngine(cfg, kv_type=F8).close()                          # a valid create works afterwards
    with pytest.raises(hip.HipError, match=r"tts_hip_orpheus_create: kv_type TTS_HIP_KV_F8_E4M3 together with TTS_HIP_FLAG_KV_F16"):
        hip.OrpheusEngine(cfg, flags=hip.FLAG_KV_F16, kv_type=F8)
    model = synth.build_orpheus(cfg)
    eng = hip.OrpheusEngine(cfg, kv_type=gguf.F16)                      # TTS_HIP_F16: the same as the flag
    eng.load(model)
    assert _elem(eng) == 2
    eng.close()
    dcfg = synth.dia_tiny()
    with pytest.raises(hip.HipError, match=r"tts_hip_dia_create: kv_type 256 is neither TTS_HIP_F32 \(0\) nor TTS_HIP_F16 \(1\)"):
        hip.DiaEngine(dcfg, kv_type=F8)
    hip.DiaEngine(dcfg).close()
    # a caller built against the header before kv_type: the shorter descriptor is accepted and gives the fp32 cache
    assert C.sizeof(_DescBeforeKvType) == C.sizeof(hip.OrpheusDesc) - 4
    L = hip.load_lib()
    d = _DescBeforeKvType()
    d.struct_size = C.sizeof(d)
    d.hidden_size, d.n_layers, d.n_attn_heads, d.n_kv_heads, d.head_dim = cfg.hidden, cfg.layers, cfg.heads, cfg.kv_heads, cfg.head_dim
    d.vocab_size, d.n_ctx, d.rope_base, d.flags, d.max_seqs = cfg.vocab, cfg.ctx, 0.0, 0, 1
    buf = (C.c_uint32 * (C.sizeof(d) // 4 + 1))()                       # what follows the short descriptor in memory must not be read as kv_type
    C.memmove(buf, C.byref(d), C.sizeof(d))
    buf[C.sizeof(d) // 4] = F8
    ctx = L.tts_hip_orpheus_create(0, C.cast(buf, C.POINTER(hip.OrpheusDesc)))
    assert ctx, L.tts_hip_last_error()
    old = hip.OrpheusEngine.__new__(hip.OrpheusEngine)
    old.L, old.cfg, old.ctx, old._stream = L, cfg, ctx, (1, 0)
    old.load(model)
    assert _elem(old) == 4
    old.close()
    d.struct_size = C.sizeof(d) - 4                                     # every other size is refused as before
    C.memmove(buf, C.byref(d), C.sizeof(d))
    assert not L.tts_hip_orpheus_create(0, C.cast(buf, C.POINTER(hip.OrpheusDesc)))
    assert b"struct_size" in L.tts_hip_last_error()
