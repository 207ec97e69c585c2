"""The mixed Orpheus session (tts_hip_orpheus_stream_begin_mixed / _admit_mixed): every cache slot carries its own sampler, so requests that differ
in voice, seed and sampler settings, greedy ones among them, share one lock-step forward.  The mixed selection kernels against the one-row sampler,
the session against one-sequence generations, misuse, and the runner's and the pool's per-request configurations on top of it."""
import functools
import os

import numpy as np
import pytest

from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

V3B = 156940
TOPK_PARTS = 64          # csrc/llama_kernels.h
NEVER = 5                # stop id = vocab + NEVER: a token nobody selects


def _setting(top_k, temperature, repetition_penalty, top_p):
    return dict(top_k=top_k, temperature=temperature, repetition_penalty=repetition_penalty, top_p=top_p)


# ---- the mixed selection at the real vocabulary -------------------------------------------------------------------------------------------
ROW_SETTINGS = [_setting(50, 1.0, 1.0, 1.0), _setting(7, 0.9, 1.5, 1.0), _setting(64, 1.4, 1.0, 1.0), _setting(50, 0.8, 1.1, 0.9), None]


@functools.lru_cache(maxsize=None)
def _full_vocab_engine():
    cfg = synth.orpheus_tiny(vocab=V3B)
    eng = hip.OrpheusEngine(cfg, max_seqs=5)
    eng.load(synth.build_orpheus(cfg))
    return eng


def _selection_logits(rng, n):
    """random rows; row 0 carries a block of exactly equal maxima across a part boundary of the 64-part partition, the last row (n > 1) is constant"""
    lg = (rng.standard_normal((n, V3B)) * 3.0).astype(np.float32)
    chunk = (V3B + TOPK_PARTS - 1) // TOPK_PARTS
    b = 3 * chunk
    lg[0, b - 5:b + 5] = np.float32(lg[0].max() + 2.0)
    if n > 1:
        lg[n - 1, :] = np.float32(0.25)
    return lg


def _check_rows(eng, lg, settings, last, cnt, u):
    """sample_logits_rows_mixed against one tts_hip_orpheus_sample_logits call per row with that row's setting: token and updated state"""
    n = len(settings)
    tok, last2, cnt2 = eng.sample_logits_rows_mixed(lg, settings, u, last_id=last, rep_count=cnt)
    for r, s in enumerate(settings):
        if s is None:
            # sampler::max: the first maximum wins, which is numpy's argmax; the one-row sampler at top_k 1 selects it too
            want, state = eng.sample_logits(lg[r], 0.5, top_k=1)[0], (int(last[r]), int(cnt[r]))
            assert want == int(lg[r].argmax())
        else:
            want, l, c = eng.sample_logits(lg[r], float(u[r]), last_id=int(last[r]), rep_count=int(cnt[r]), **s)
            state = (l, c) if s["repetition_penalty"] != 1.0 else (int(last[r]), int(cnt[r]))   # no penalty: the state does not move
        assert int(tok[r]) == want, (n, r, s)
        assert (int(last2[r]), int(cnt2[r])) == state, (n, r, s)


def test_mixed_selection_equals_the_one_row_sampler_per_row():
    """The five mixed kernels (tts_hip_orpheus_sample_logits_rows_mixed) at 156 940 logits: every row with its own setting, one of them greedy,
    against tts_hip_orpheus_sample_logits with that row's setting, which test_gpu_orpheus.py pins to the reference sampler.  Equal maxima across a
    part boundary in row 0, a constant last row, uniforms 0 and 0.99999994, one row in the reset state; the settings rotate through every row
    position; 1, 3 and 5 rows.  Tokens and updated (last_id, rep_count) exactly equal."""
    eng = _full_vocab_engine()
    rng = np.random.default_rng(2024)
    cases = [(5, ROW_SETTINGS[rot:] + ROW_SETTINGS[:rot]) for rot in range(5)]
    three = [ROW_SETTINGS[1], None, ROW_SETTINGS[3]]
    cases += [(3, three[rot:] + three[:rot]) for rot in range(3)]
    cases += [(1, [s]) for s in ROW_SETTINGS]
    for n, settings in cases:
        lg = _selection_logits(rng, n)
        last = rng.integers(0, V3B, n).astype(np.int32)
        cnt = rng.integers(1, 5, n).astype(np.uint32)
        last[0] = int(np.argmax(lg[0]))       # the penalised token is the first of the equal maxima
        if n > 1:
            last[1], cnt[1] = -1, 0           # sampler::reset
        u = rng.random(n, dtype=np.float32)
        u[0] = np.float32(0.0)
        if n > 2:
            u[2] = np.float32(0.99999994)
        _check_rows(eng, lg, settings, last, cnt, u)
    lg = _selection_logits(rng, 3)
    bad = [ROW_SETTINGS[0], _setting(65, 1.0, 1.0, 1.0), None]
    with pytest.raises(hip.HipError, match="top_k"):
        eng.sample_logits_rows_mixed(lg, bad, np.zeros(3, dtype=np.float32))
    with pytest.raises(hip.HipError, match="max_seqs"):
        eng.sample_logits_rows_mixed(np.zeros((6, V3B), dtype=np.float32), [None] * 6)
    _check_rows(eng, lg, three, np.full(3, -1, dtype=np.int32), np.zeros(3, dtype=np.uint32), np.full(3, 0.5, dtype=np.float32))


# ---- the mixed session against one-sequence generations -----------------------------------------------------------------------------------
MAX_NEW = 14
GREEDY = None
S12 = dict(top_k=12, temperature=0.9, repetition_penalty=1.2)
S5 = dict(top_k=5, temperature=1.3)
S20 = dict(top_k=20, top_p=0.85, repetition_penalty=1.1)
# with three slots and utterances of equal length the slots are refilled in order: slot 0 takes utterances 0, 3, 6 (penalty 1 after 1.2), slot 1
# takes 1, 4 (greedy after sampled), slot 2 takes 2, 5 (sampled with a nucleus after greedy)
UTT_SETTINGS = [S12, S12, GREEDY, S5, GREEDY, S20, S12]
N_SLOTS = 3


def _eager_engine(cfg, **kw):
    os.environ["TTS_HIP_LLAMA_GRAPH"] = "0"
    try:
        return hip.OrpheusEngine(cfg, **kw)
    finally:
        del os.environ["TTS_HIP_LLAMA_GRAPH"]


@functools.lru_cache(maxsize=None)
def _reference(wtype):
    """prompts of 3-9 ids, uniforms, and per stop id the ids of the eager one-sequence engine with each utterance's own setting"""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=wtype))
    cfg = model.cfg
    rng = np.random.default_rng(77 + wtype)
    prompts = [rng.integers(0, cfg.vocab, 3 + u).astype(np.uint32) for u in range(len(UTT_SETTINGS))]
    uni = rng.random((len(prompts), MAX_NEW), dtype=np.float32)
    single = _eager_engine(cfg)
    single.load(model)

    def one(u, stop):
        s = UTT_SETTINGS[u]
        if s is None:
            return single.generate_greedy(prompts[u], MAX_NEW, stop_id=stop).tolist()
        return single.generate_sampled(prompts[u], MAX_NEW, stop_id=stop, uniforms=uni[u], **s).tolist()

    never = cfg.vocab + NEVER
    ref_never = [one(u, never) for u in range(len(prompts))]
    stop = int(ref_never[2][5])                                  # utterance 2 is greedy: it ends with its sixth id
    ref_stop = [one(u, stop) for u in range(len(prompts))]
    single.close()
    return model, prompts, uni, never, ref_never, stop, ref_stop


def _run_mixed_session(eng, prompts, uni, n_steps, stop_id):
    """every prompt through one mixed session, admitted into whatever slots are free after each run
    -> (ids per utterance, (setting of the previous utterance, setting of the next) for every reuse of a slot)"""
    eng.stream_begin_mixed(N_SLOTS, MAX_NEW, stop_id)
    free, slot_utt, reuse = list(range(N_SLOTS)), {}, []
    held = [None] * N_SLOTS
    out, nxt, runs = [None] * len(prompts), 0, 0
    while nxt < len(prompts) or slot_utt:
        while nxt < len(prompts) and free:
            s = free.pop(0)
            eng.stream_admit_mixed([s], [prompts[nxt]], [UTT_SETTINGS[nxt]], uni[nxt:nxt + 1])
            if held[s] is not None:
                reuse.append((held[s], nxt))
            slot_utt[s] = held[s] = nxt
            nxt += 1
        fin = eng.stream_run(n_steps)
        runs += 1
        for s, cnt in fin:
            out[slot_utt.pop(s)] = eng.stream_collect(s, cnt).tolist()
            free.append(s)
        assert runs < 1000
    assert eng.stream_run(n_steps) == []
    eng.stream_end()
    return out, reuse


@pytest.mark.parametrize("wtype", [gguf.F16, gguf.Q4_0])
def test_mixed_session_equals_one_sequence_generations(wtype):
    """Seven utterances, each with one of four settings (greedy; top_k 12 / T 0.9 / rep 1.2; top_k 5 / T 1.3; top_k 20 / top_p 0.85 / rep 1.1),
    through a mixed session of three slots against the eager one-sequence engine with that utterance's setting and uniforms: ids and counts equal,
    at look-in intervals of 1, 5 and 28 steps, with a stop id nobody meets and with one that ends a greedy utterance inside a run.  Slots are
    reused by utterances of another mode (greedy after sampled, penalty 1 after 1.2): a trace of the predecessor would change the ids."""
    model, prompts, uni, never, ref_never, stop, ref_stop = _reference(wtype)
    assert len(ref_stop[2]) == 6 and len({len(r) for r in ref_stop}) > 1
    eng = hip.OrpheusEngine(model.cfg, max_seqs=N_SLOTS)
    eng.load(model)
    seen = set()
    for n_steps in (1, 5, 28):
        got, reuse = _run_mixed_session(eng, prompts, uni, n_steps, stop)
        assert got == ref_stop, n_steps
        seen.update(reuse)
        got, reuse = _run_mixed_session(eng, prompts, uni, n_steps, never)
        assert got == ref_never, n_steps
        seen.update(reuse)
    kinds = {(UTT_SETTINGS[a] is None, UTT_SETTINGS[b] is None) for a, b in seen}
    assert (False, True) in kinds and (True, False) in kinds, seen        # greedy after sampled, sampled after greedy
    assert any(UTT_SETTINGS[a] is S12 and UTT_SETTINGS[b] is S5 for a, b in seen), seen   # penalty 1 after 1.2
    eng.close()


def test_mixed_session_misuse_is_refused_and_the_session_goes_on():
    model, prompts, uni, never, ref_never, _, _ = _reference(gguf.F16)
    cfg = model.cfg
    eng = hip.OrpheusEngine(cfg, max_seqs=N_SLOTS)
    eng.load(model)
    single = _eager_engine(cfg)
    single.load(model)
    ref_greedy0 = single.generate_greedy(prompts[0], MAX_NEW, stop_id=never).tolist()
    single.close()
    # admit_mixed on a session opened with one sampler
    eng.stream_begin(N_SLOTS, MAX_NEW, never)
    eng.stream_admit([0], [prompts[0]])
    with pytest.raises(hip.HipError, match="one sampler"):
        eng.stream_admit_mixed([1], [prompts[1]], [S12], uni[1:2])
    assert eng.stream_run(64) == [(0, MAX_NEW)]
    assert eng.stream_collect(0, MAX_NEW).tolist() == ref_greedy0
    eng.stream_end()
    # the plain admit on a mixed session; a bad sampler on one of two utterances: neither is admitted
    eng.stream_begin_mixed(N_SLOTS, MAX_NEW, never)
    eng.stream_admit_mixed([0], [prompts[0]], [UTT_SETTINGS[0]], uni[0:1])
    with pytest.raises(hip.HipError, match="per slot"):
        eng.stream_admit([1], [prompts[1]])
    with pytest.raises(hip.HipError, match="top_k"):
        eng.stream_admit_mixed([1, 2], [prompts[1], prompts[2]], [S12, dict(top_k=65)], uni[1:3])
    with pytest.raises(hip.HipError, match="temperature"):
        eng.stream_admit_mixed([1, 2], [prompts[2], prompts[1]], [GREEDY, dict(top_k=5, temperature=0.0)], uni[1:3])
    with pytest.raises(hip.HipError, match="uniforms"):
        eng.stream_admit_mixed([1], [prompts[1]], [S12])
    with pytest.raises(hip.HipError, match="busy"):
        eng.stream_admit_mixed([0], [prompts[1]], [S12], uni[1:2])
    eng.stream_admit_mixed([1, 2], [prompts[1], prompts[2]], [UTT_SETTINGS[1], UTT_SETTINGS[2]], uni[1:3])   # the slots the refusals named are free
    fin = eng.stream_run(64)
    assert fin == [(0, MAX_NEW), (1, MAX_NEW), (2, MAX_NEW)]
    assert [eng.stream_collect(s, c).tolist() for s, c in fin] == ref_never[:3]
    eng.stream_end()
    eng.close()


# ---- runner, C API and pool ---------------------------------------------------------------------------------------------------------------
TEXTS = ["hello the zebra", "a zebra", "the quick hello of the zebra there", "hello", "the zebra there hello", "a quick zebra", "of the hello",
         "zebra zebra the quick", "there a hello of zoe"]
# candidates, tried per text in this order starting at the text's index: random weights may select a text id where an audio id belongs, and then
# generate() itself fails; a text keeps the first configuration whose generate() call succeeds
CANDIDATES = [dict(voice=b"zoe", sample=0), dict(voice=b"leo", sample=1, top_k=4, temperature=0.7, seed=3), dict(voice=b"mia", sample=1, top_k=8, temperature=1.2, seed=11),
              dict(voice=b"leo", sample=0), dict(voice=b"zoe", sample=1, top_k=3, temperature=0.9, seed=5), dict(voice=b"jess", sample=1, top_k=2, temperature=0.5, seed=7)]


@pytest.fixture(scope="module")
def orpheus_gguf(tmp_path_factory):
    return synth.SynthOrpheusFull(max_gen=28).write_gguf(str(tmp_path_factory.mktemp("orpheus_stream_mixed") / "orpheus.gguf"))


@pytest.fixture(scope="module")
def no_noise():
    old = os.environ.get("TTS_SNAC_NO_NOISE")
    os.environ["TTS_SNAC_NO_NOISE"] = "1"
    yield
    if old is None:
        del os.environ["TTS_SNAC_NO_NOISE"]
    else:
        os.environ["TTS_SNAC_NO_NOISE"] = old


@pytest.fixture(scope="module")
def six(orpheus_gguf, no_noise):
    """six (text, configuration, audio of a fresh generate() call) that differ in voice, temperature, top_k, seed and sample"""
    from tts_cpp_amd import runner
    one = runner.Runner(orpheus_gguf, sample=0)
    picked = []
    for i, t in enumerate(TEXTS):
        for j in range(len(CANDIDATES)):
            kw = CANDIDATES[(i + j) % len(CANDIDATES)]
            try:
                picked.append((t, kw, one.generate(t, **kw)))
                break
            except runner.RunnerError as e:
                assert "codebook size" in str(e)
        if len(picked) == 6:
            break
    one.close()
    assert len(picked) == 6, "pick other TEXTS / CANDIDATES: fewer than six generate() calls succeed"
    cfgs = [kw for _, kw, _ in picked]
    assert {kw["sample"] for kw in cfgs} == {0, 1} and len({kw["voice"] for kw in cfgs}) >= 2, cfgs
    assert all(len({kw.get(f) for kw in cfgs if kw["sample"]}) >= 2 for f in ("temperature", "top_k", "seed")), cfgs
    return picked


def test_runner_generate_stream_with_per_text_configs_equals_single_calls(orpheus_gguf, six, no_noise):
    """tts_c_generate_stream_configs over orpheus_runner's mixed session: six texts, each with its own voice, seed and sampler, through three
    slots; every audio bit for bit that of generate(text, **config) on a fresh call.  A request the device sampler does not carry fails the
    call, and the runner works afterwards."""
    from tts_cpp_amd import runner
    many = runner.Runner(orpheus_gguf, sample=0, max_seqs=3)
    got = many.generate_stream([t for t, _, _ in six], configs=[kw for _, kw, _ in six])
    assert len(got) == 6
    for i, ((t, kw, want), audio) in enumerate(zip(six, got)):
        assert want.size > 0 and np.array_equal(want, audio), (i, t, kw)
    with pytest.raises(runner.RunnerError, match="device sampler"):
        many.generate_stream([six[0][0], six[1][0]], configs=[six[0][1], dict(voice=b"zoe", sample=1, top_k=0)])
    with pytest.raises(runner.RunnerError, match="not a valid voice"):
        many.generate_stream([six[0][0], six[1][0]], configs=[six[0][1], dict(voice=b"nobody", sample=0)])
    t, kw, want = six[1]
    assert np.array_equal(many.generate(t, **kw), want)
    assert np.array_equal(many.generate_stream([six[0][0], t], configs=[six[0][1], kw])[1], want)
    many.close()


def test_pool_continuous_mode_takes_differing_requests_into_one_session(orpheus_gguf, six, no_noise):
    """Six requests that differ in voice, seed and sampler through a continuous pool of three slots: the session's runner accepts them
    (stream_accepts), so they are answered out of ONE session, joining it in flight, with the audio of their own generate() calls; the pool
    opens no more sessions than for six requests with identical configurations."""
    from tts_cpp_amd import runner

    def serve(requests):
        pool = runner.Pool(orpheus_gguf, n_workers=1, max_batch=3, continuous=True, sample=0, voice=b"zoe")
        ids = [pool.submit(t, **kw) for t, kw in requests]
        out = [pool.wait(tid, 60000) for tid in ids]
        st = pool.stats()
        pool.close()
        return out, st

    _, st_same = serve([(t, dict(voice=b"zoe", sample=0)) for t, _, _ in six])
    mixed, st = serve([(t, kw) for t, kw, _ in six])
    for i, ((t, kw, want), (audio, bs, wk, err)) in enumerate(zip(six, mixed)):
        assert err == "" and np.array_equal(audio, want), (i, kw, err)
    assert st["tasks"] == 6 and st["largest_batch"] <= 3, st
    assert st["batches"] == 1 and st["admitted_in_flight"] > 0 and st["batches"] <= st_same["batches"], (st, st_same)
