"""The Orpheus continuous session (tts_hip_orpheus_stream_*): the row-batched selection, the device-driven lock-step loop, the runner's
stream_* interface and the device pool's continuous mode on top of it."""
import functools
import os

import numpy as np
import pytest

from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

V3B = 156940
TOPK_PARTS = 64          # csrc/llama_kernels.h
NEVER = 5                # stop id = vocab + NEVER: a token nobody selects


@functools.lru_cache(maxsize=None)
def _full_vocab_engine():
    cfg = synth.orpheus_tiny(vocab=V3B)
    eng = hip.OrpheusEngine(cfg, max_seqs=5)
    eng.load(synth.build_orpheus(cfg))
    return eng


def _selection_logits(rng, n):
    """random rows; row 0 carries a block of exactly equal maxima across a part boundary of topk_parts_kernel's partition, the last row (n > 1) is constant"""
    lg = (rng.standard_normal((n, V3B)) * 3.0).astype(np.float32)
    chunk = (V3B + TOPK_PARTS - 1) // TOPK_PARTS
    b = 3 * chunk
    lg[0, b - 5:b + 5] = np.float32(lg[0].max() + 2.0)
    if n > 1:
        lg[n - 1, :] = np.float32(0.25)
    return lg


@pytest.mark.parametrize("params", [(50, 1.0, 1.0, 1.0), (7, 0.9, 1.5, 1.0), (64, 1.4, 1.0, 1.0), (1, 1.0, 1.0, 1.0), (50, 0.8, 1.1, 0.9), None],
                         ids=["k50", "k7_t0.9_r1.5", "k64_t1.4", "k1", "k50_t0.8_r1.1_p0.9", "argmax"])
def test_row_batched_selection_equals_the_one_row_sampler(params):
    """topk_parts_rows_kernel / softmax_total_rows_kernel / topk_sample_rows_kernel and the arg-max pair with the row as a grid dimension
    (tts_hip_orpheus_sample_logits_rows) against n calls of tts_hip_orpheus_sample_logits, which test_gpu_orpheus.py pins to the reference
    sampler: 156 940 logits, 1 / 3 / 5 rows, per-row repetition state (one row in the reset state), tokens and updated state exactly equal."""
    eng = _full_vocab_engine()
    rng = np.random.default_rng(7 if params is None else int(params[0] * 31 + params[1] * 10 + params[3] * 1000))
    for n in (1, 3, 5):
        lg = _selection_logits(rng, n)
        if params is None:
            tok, _, _ = eng.sample_logits_rows(lg)
            # sampler::max: the first maximum wins, which is numpy's argmax; the one-row sampler at top_k 1 selects it too
            want = [int(lg[r].argmax()) for r in range(n)]
            one = [eng.sample_logits(lg[r], 0.5, top_k=1)[0] for r in range(n)]
            assert tok.tolist() == want == one
            continue
        top_k, temp, rep, top_p = params
        last = rng.integers(0, V3B, n).astype(np.int32)
        cnt = rng.integers(1, 5, n).astype(np.uint32)
        last[0] = int(np.argmax(lg[0]))       # the penalised token is the first of the equal maxima
        if n > 1:
            last[1], cnt[1] = -1, 0           # sampler::reset
        u = rng.random(n, dtype=np.float32)
        u[0] = np.float32(0.0)
        if n > 2:
            u[2] = np.float32(0.99999994)
        tok, last2, cnt2 = eng.sample_logits_rows(lg, u, top_k=top_k, temperature=temp, repetition_penalty=rep, top_p=top_p, last_id=last, rep_count=cnt)
        for r in range(n):
            t, l, c = eng.sample_logits(lg[r], float(u[r]), top_k=top_k, temperature=temp, repetition_penalty=rep, top_p=top_p, last_id=int(last[r]), rep_count=int(cnt[r]))
            assert int(tok[r]) == t, (n, r)
            if rep != 1.0:
                assert (int(last2[r]), int(cnt2[r])) == (l, c), (n, r)
            else:
                assert (int(last2[r]), int(cnt2[r])) == (int(last[r]), int(cnt[r])), (n, r)   # no penalty: the state does not move
    with pytest.raises(hip.HipError, match="max_seqs"):
        eng.sample_logits_rows(np.zeros((6, V3B), dtype=np.float32))
    with pytest.raises(hip.HipError, match="top_k"):
        eng.sample_logits_rows(np.zeros((2, V3B), dtype=np.float32), np.zeros(2, dtype=np.float32), top_k=65)


# ---- the session against one-sequence generations ---------------------------------------------------------------------------------------
MAX_NEW = 14
SMP = dict(top_k=12, temperature=0.9, repetition_penalty=1.2)


def _eager_engine(cfg, **kw):
    os.environ["TTS_HIP_LLAMA_GRAPH"] = "0"
    try:
        return hip.OrpheusEngine(cfg, **kw)
    finally:
        del os.environ["TTS_HIP_LLAMA_GRAPH"]


@functools.lru_cache(maxsize=None)
def _reference(n_slots, wtype):
    """prompts, uniforms and the ids of the eager one-sequence engine, as test_orpheus_lockstep_batch_equals_single_sequence_generations builds them
    (same seed formula; its first n_slots prompts are that test's)"""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=wtype))
    cfg = model.cfg
    n_utt = 2 * n_slots + 1
    rng = np.random.default_rng(10 * n_slots + wtype)
    prompts = [rng.integers(0, cfg.vocab, 3 + 2 * (u % 4)).astype(np.uint32) for u in range(n_utt)]
    uni = rng.random((n_utt, MAX_NEW), dtype=np.float32)
    single = _eager_engine(cfg)
    single.load(model)
    never = cfg.vocab + NEVER
    greedy = [single.generate_greedy(p, MAX_NEW, stop_id=never).tolist() for p in prompts]
    stop = int(greedy[1][5])
    stopped = [single.generate_greedy(p, MAX_NEW, stop_id=stop).tolist() for p in prompts]
    sampled = [single.generate_sampled(p, MAX_NEW, stop_id=never, uniforms=uni[u], **SMP).tolist() for u, p in enumerate(prompts)]
    single.close()
    return model, prompts, uni, stop, greedy, stopped, sampled


def _run_session(eng, prompts, n_slots, n_steps, stop_id, uniforms=None, max_new=MAX_NEW, **smp):
    """every prompt through one session: admit into whatever slots are free after each run -> (ids per utterance, facts about the schedule)"""
    eng.stream_begin(n_slots, max_new, stop_id, sampled=uniforms is not None, **smp)
    free, slot_utt, uses = list(range(n_slots)), {}, [0] * n_slots
    out, end_run = [None] * len(prompts), [None] * len(prompts)
    nxt, run, runs_of, mid_flight = 0, 0, {}, False
    while nxt < len(prompts) or slot_utt:
        while nxt < len(prompts) and free:
            s = free.pop(0)
            mid_flight = mid_flight or any(runs_of[o] > 0 for o in slot_utt)    # someone else has been through a run: unequal positions
            eng.stream_admit([s], [prompts[nxt]], None if uniforms is None else uniforms[nxt:nxt + 1])
            slot_utt[s], runs_of[s] = nxt, 0
            uses[s] += 1
            nxt += 1
        fin = eng.stream_run(n_steps)
        run += 1
        for s in slot_utt:
            runs_of[s] += 1
        assert [s for s, _ in fin] == sorted(s for s, _ in fin)
        for s, cnt in fin:
            u = slot_utt.pop(s)
            out[u], end_run[u] = eng.stream_collect(s, cnt).tolist(), run
            free.append(s)
        assert run < 1000
    assert eng.stream_run(n_steps) == []          # no live rows: returns at once with nothing finished
    eng.stream_end()
    return out, dict(mid_flight=mid_flight, slot_twice=max(uses) > 1, refilled=sum(u > 1 for u in uses), runs=len(set(end_run)))


@pytest.mark.parametrize("wtype", [gguf.F16, gguf.Q4_0])
@pytest.mark.parametrize("n_slots", [3, 7])
def test_session_equals_one_sequence_generations(n_slots, wtype):
    """2 n_slots + 1 utterances through a session of n_slots slots (3: the 1-4-row kernels; 7: the weight-streaming GEMM, falling to <= 4 live
    rows as utterances end), admitted into whatever slots are free after each run, against the eager one-sequence engine: greedy with a stop
    id nobody meets, greedy with stop = ref[1][5] (utterances end early and in the middle of a run), and sampled with per-utterance uniforms.
    Look-in intervals of 1 and 5 steps give the same ids; 5 does not divide the lengths, so steps past a stop are really discarded."""
    model, prompts, uni, stop, greedy, stopped, sampled = _reference(n_slots, wtype)
    cfg = model.cfg
    never = cfg.vocab + NEVER
    assert len({len(r) for r in stopped}) > 1
    eng = hip.OrpheusEngine(cfg, max_seqs=n_slots)
    eng.load(model)
    for n_steps in (1, 5):
        got, facts = _run_session(eng, prompts, n_slots, n_steps, never)
        assert got == greedy, n_steps
        assert facts["slot_twice"] and facts["runs"] > 1, facts
        got, facts = _run_session(eng, prompts, n_slots, n_steps, stop)
        assert got == stopped, n_steps
        # the lengths the reference fixes decide these: utterances admitted beside others in mid-generation, slots reused, ends in different runs
        assert facts["mid_flight"] and facts["slot_twice"] and facts["runs"] > 1, facts
        got, facts = _run_session(eng, prompts, n_slots, n_steps, never, uniforms=uni, **SMP)
        assert got == sampled, n_steps
        assert facts["slot_twice"] and facts["runs"] > 1, facts
    eng.close()


@functools.lru_cache(maxsize=None)
def _cache_end_reference():
    """a short prompt and one that leaves six positions of the cache, with the ids of the eager one-sequence engine"""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=gguf.F16))
    cfg = model.cfg
    never = cfg.vocab + NEVER
    rng = np.random.default_rng(3)
    short, long_ = rng.integers(0, cfg.vocab, 6).astype(np.uint32), rng.integers(0, cfg.vocab, cfg.ctx - 6).astype(np.uint32)
    single = _eager_engine(cfg)
    single.load(model)
    ref_short, ref_long = single.generate_greedy(short, MAX_NEW, never).tolist(), single.generate_greedy(long_, MAX_NEW, never).tolist()
    ref_one = single.generate_greedy(short, 1, never).tolist()
    single.close()
    return model, short, long_, ref_short, ref_long, ref_one


def test_session_ends_where_the_one_sequence_generation_ends():
    """max_new ids, the end of the cache (prompt + max_new > n_ctx) and max_new 0"""
    model, short, long_, ref_short, ref_long, ref_one = _cache_end_reference()
    cfg = model.cfg
    never = cfg.vocab + NEVER
    assert len(ref_short) == MAX_NEW and 0 < len(ref_long) < MAX_NEW      # the second one runs into the end of the cache
    eng = hip.OrpheusEngine(cfg, max_seqs=2)
    eng.load(model)
    for n_steps in (1, 4, 64):
        got, _ = _run_session(eng, [short, long_], 2, n_steps, never)
        assert got == [ref_short, ref_long], n_steps
    got, _ = _run_session(eng, [short], 2, 3, never, max_new=1)           # the first selection is the last: finished at admission
    assert got == [ref_one]
    eng.stream_begin(2, 0, never)
    eng.stream_admit([1], [short])
    assert eng.stream_run(7) == [(1, 0)]
    assert eng.stream_collect(1, 0).size == 0
    eng.stream_end()
    eng.close()


# ---- the fixed batch: the same loop with every slot admitted at begin ---------------------------------------------------------------------
def _batch_in_pieces(eng, prompts, max_new, stop_id, k, ref, **kw):
    """gen_begin, then launches of k steps; after the j-th launch (j = 0: the begin) an utterance whose one-sequence generation has L ids has
    handed out min(L, 1 + j k) of them and is done exactly when those are all"""
    eng.gen_begin(prompts, max_new, stop_id, **kw)
    j = 0
    while True:
        ids, done = eng.gen_wait()
        for u, r in enumerate(ref):
            want = min(len(r), 1 + j * k)
            assert ids[u].tolist() == r[:want], (k, j, u)
            assert bool(done[u]) == (want == len(r)), (k, j, u)
        if done.all():
            return j
        eng.gen_launch(k)
        j += 1
        assert j < 100


def test_fixed_batch_rows_that_end_inside_a_launch():
    """tts_hip_orpheus_gen_* at three utterances, launches of 1, 3 and 64 steps (64: more than is left of max_new 14), with the stopping id of
    test_orpheus_lockstep_batch_equals_single_sequence_generations (some utterances meet it early, others never): the ids are the eager
    one-sequence ids, nothing is counted after the stopping id, and an utterance is done at the wait of the launch in which it ended."""
    model, prompts, uni, stop, greedy, stopped, sampled = _reference(3, gguf.F16)
    cfg = model.cfg
    never = cfg.vocab + NEVER
    assert len({len(r) for r in stopped[:3]}) > 1 and max(len(r) for r in stopped[:3]) == MAX_NEW
    eng = hip.OrpheusEngine(cfg, max_seqs=3)
    eng.load(model)
    for k in (1, 3, 64):
        launches = _batch_in_pieces(eng, prompts[:3], MAX_NEW, stop, k, stopped[:3])
        assert launches == -(-(MAX_NEW - 1) // k)
        _batch_in_pieces(eng, prompts[:3], MAX_NEW, never, k, greedy[:3])
        _batch_in_pieces(eng, prompts[:3], MAX_NEW, never, k, sampled[:3], uniforms=uni[:3], **SMP)
    assert [g.tolist() for g in eng.generate_batch(prompts[:3], MAX_NEW, stop)] == stopped[:3]
    eng.close()


def test_fixed_batch_ends_where_the_one_sequence_generation_ends():
    """the end of the cache inside a launch (prompt + max_new > n_ctx), max_new 1 and max_new 0 in a fixed batch"""
    model, short, long_, ref_short, ref_long, ref_one = _cache_end_reference()
    cfg = model.cfg
    never = cfg.vocab + NEVER
    assert len(ref_short) == MAX_NEW and 0 < len(ref_long) < MAX_NEW
    eng = hip.OrpheusEngine(cfg, max_seqs=2)
    eng.load(model)
    assert [g.tolist() for g in eng.generate_batch([short, long_], MAX_NEW, never)] == [ref_short, ref_long]
    for k in (1, 4, 64):
        _batch_in_pieces(eng, [short, long_], MAX_NEW, never, k, [ref_short, ref_long])
    assert [g.tolist() for g in eng.generate_batch([short, short], 1, never)] == [ref_one, ref_one]
    assert [g.size for g in eng.generate_batch([short, long_], 0, never)] == [0, 0]
    eng.gen_begin([short, long_], 0, never)
    ids, done = eng.gen_wait()
    assert [i.size for i in ids] == [0, 0] and done.all()
    eng.close()


def test_the_loops_buffers_are_reused_without_a_trace_of_the_last_loop():
    """One context of seven slots: a sampled fixed batch of 3, a uniform greedy session over all 7 slots (15 utterances: slots are refilled), a
    mixed session (every other utterance sampled), a greedy fixed batch of 7 with another max_new, and the first call again.  The loop's device
    buffers stay on the context between them, so every admission has to overwrite what the slot's predecessor left — state, sampler state,
    record, penalty table, uniforms, ids: every result equals its eager one-sequence reference, and the last equals the first."""
    model, prompts, uni, stop, greedy, stopped, sampled = _reference(7, gguf.F16)
    cfg = model.cfg
    never = cfg.vocab + NEVER
    eng = hip.OrpheusEngine(cfg, max_seqs=7)
    eng.load(model)
    first = [g.tolist() for g in eng.generate_batch(prompts[:3], MAX_NEW, never, uniforms=uni[:3], **SMP)]
    assert first == sampled[:3]
    got, facts = _run_session(eng, prompts, 7, 5, stop)
    assert got == stopped and facts["refilled"] >= 2, facts
    settings = [SMP if u % 2 == 0 else None for u in range(len(prompts))]
    eng.stream_begin_mixed(7, MAX_NEW, never)
    eng.stream_admit_mixed(list(range(7)), prompts[:7], settings[:7], uni[:7])
    fin = eng.stream_run(64)
    assert [s for s, _ in fin] == list(range(7))
    assert [eng.stream_collect(s, c).tolist() for s, c in fin] == [sampled[u] if u % 2 == 0 else greedy[u] for u in range(7)]
    eng.stream_admit_mixed([0, 1], prompts[7:9], settings[7:9], uni[7:9])      # utterance 7 is greedy in slot 0 after a sampled one, 8 the reverse
    fin = eng.stream_run(64)
    assert [eng.stream_collect(s, c).tolist() for s, c in fin] == [greedy[7], sampled[8]]
    eng.stream_end()
    assert [g.tolist() for g in eng.generate_batch(prompts[:7], 5, never)] == [r[:5] for r in greedy[:7]]   # greedy: max_new 5 gives the first 5 ids
    again = [g.tolist() for g in eng.generate_batch(prompts[:3], MAX_NEW, never, uniforms=uni[:3], **SMP)]
    assert again == first == sampled[:3]
    eng.close()


def test_session_misuse_is_refused_and_the_context_works_afterwards():
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=gguf.F16))
    cfg = model.cfg
    never = cfg.vocab + NEVER
    rng = np.random.default_rng(11)
    prompts = [rng.integers(0, cfg.vocab, 4 + u).astype(np.uint32) for u in range(3)]
    single = _eager_engine(cfg)
    single.load(model)
    ref = [single.generate_greedy(p, MAX_NEW, never).tolist() for p in prompts]
    single.close()
    eng = hip.OrpheusEngine(cfg, max_seqs=3)
    eng.load(model)
    with pytest.raises(hip.HipError, match="no session"):
        eng.stream_run(1)
    with pytest.raises(hip.HipError, match="max_seqs"):
        eng.stream_begin(4, MAX_NEW, never)
    with pytest.raises(hip.HipError, match="top_k"):
        eng.stream_begin(2, MAX_NEW, never, sampled=True, top_k=0)
    eng.gen_begin(prompts[:2], MAX_NEW, never)
    with pytest.raises(hip.HipError, match="under way"):
        eng.stream_begin(2, MAX_NEW, never)                       # a gen_* generation with unfinished utterances
    eng.gen_launch(64)
    assert all(eng.gen_wait()[1])
    eng.stream_begin(2, MAX_NEW, never)
    eng.stream_admit([0], [prompts[0]])
    with pytest.raises(hip.HipError, match="busy"):
        eng.stream_admit([0], [prompts[1]])
    with pytest.raises(hip.HipError, match="n_slots"):
        eng.stream_admit([2], [prompts[1]])                       # max_seqs is 3, the session has 2 slots
    with pytest.raises(hip.HipError, match="twice"):
        eng.stream_admit([1, 1], [prompts[1], prompts[2]])
    with pytest.raises(hip.HipError, match="does not fit"):
        eng.stream_admit([1], [np.zeros(cfg.ctx, dtype=np.uint32)])
    with pytest.raises(hip.HipError, match="vocabulary"):
        eng.stream_admit([1], [np.array([cfg.vocab], dtype=np.uint32)])
    with pytest.raises(hip.HipError, match="not finished"):
        eng.stream_collect(0, 1)
    with pytest.raises(hip.HipError, match="n_slots"):
        eng.stream_collect(2, 1)
    for call in (lambda: eng.generate_greedy(prompts[0], 2, never), lambda: eng.generate_batch(prompts[:2], 2, never), lambda: eng.decode(prompts[0], 0),
                 lambda: eng.step_batch([0], [1], [0]), lambda: eng.gen_begin(prompts[:1], 2, never), lambda: eng.stream_begin(2, MAX_NEW, never),
                 lambda: eng.sample_logits(np.zeros(cfg.vocab, dtype=np.float32), 0.5, top_k=4),
                 lambda: eng.sample_logits_rows(np.zeros((1, cfg.vocab), dtype=np.float32))):
        with pytest.raises(hip.HipError, match="session is open"):
            call()
    eng.stream_admit([1], [prompts[1]])                           # the refused calls left the session as it was
    fin = eng.stream_run(64)
    assert fin == [(0, MAX_NEW), (1, MAX_NEW)]
    with pytest.raises(hip.HipError, match="produced"):
        eng.stream_collect(0, MAX_NEW + 1)
    assert [eng.stream_collect(s, c).tolist() for s, c in fin] == ref[:2]
    eng.stream_admit([0], [prompts[2]])                           # a collected slot is free again
    with pytest.raises(hip.HipError, match="not finished"):
        eng.stream_collect(0, 1)
    assert eng.stream_run(64) == [(0, MAX_NEW)]
    assert eng.stream_collect(0, MAX_NEW).tolist() == ref[2]
    eng.stream_end()
    eng.stream_end()                                              # idempotent
    assert eng.generate_greedy(prompts[0], MAX_NEW, never).tolist() == ref[0]
    assert [g.tolist() for g in eng.generate_batch(prompts, MAX_NEW, never)] == ref
    eng.close()


# ---- runner, C ABI and pool ---------------------------------------------------------------------------------------------------------------
TEXTS = ["hello the zebra", "a zebra", "the quick hello of the zebra there", "hello", "the zebra there hello", "a quick zebra", "of the hello",
         "zebra zebra the quick", "there a hello of zoe"]
CONFIGS = (dict(sample=0), dict(sample=1, top_k=8, seed=3))


@pytest.fixture(scope="module")
def orpheus_gguf(tmp_path_factory):
    return synth.SynthOrpheusFull(max_gen=28).write_gguf(str(tmp_path_factory.mktemp("orpheus_stream") / "orpheus.gguf"))


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
def singles(orpheus_gguf, no_noise):
    """per configuration: the audio of a generate() call per text, or None where a call fails on an id the codec refuses"""
    from tts_cpp_amd import runner
    one = runner.Runner(orpheus_gguf, sample=0)
    out = []
    for kw in CONFIGS:
        audio = []
        for t in TEXTS:
            try:
                audio.append(one.generate(t, voice=b"zoe", **kw))
            except runner.RunnerError as e:     # random weights may select a text id where an audio id belongs
                assert "codebook size" in str(e)
                audio = None
                break
        out.append(audio)
    one.close()
    return out


def test_runner_generate_stream_equals_single_calls(orpheus_gguf, singles, no_noise):
    """orpheus_runner::stream_* under tts_c_generate_stream: nine texts through a session of four slots, every audio bit for bit that of a
    generate() call of its own, greedy and with the seeded device sampler; a sampler the device does not carry is refused by stream_begin."""
    from tts_cpp_amd import runner
    many = runner.Runner(orpheus_gguf, sample=0, max_seqs=4)
    compared = 0
    for kw, want in zip(CONFIGS, singles):
        if want is None:
            continue
        got = many.generate_stream(TEXTS, voice=b"zoe", **kw)
        assert len(got) == len(TEXTS)
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.size > 0 and np.array_equal(a, b), (kw, i)
        compared += 1
    assert compared >= 1
    with pytest.raises(runner.RunnerError, match="stream_begin"):
        many.generate_stream(TEXTS[:2], voice=b"zoe", sample=1, top_k=0)
    if singles[0] is not None:     # the runner is usable after the refusal, in both modes
        assert np.array_equal(many.generate(TEXTS[1], voice=b"zoe", sample=0), singles[0][1])
        assert np.array_equal(many.generate_stream(TEXTS[:2], voice=b"zoe", sample=0)[1], singles[0][1])
    many.close()


def test_pool_continuous_mode_runs_orpheus_through_one_session(orpheus_gguf, singles, no_noise):
    """pool_options::continuous reaches Orpheus through the virtual interface: two waves of requests, answered out of one session"""
    from tts_cpp_amd import runner
    want = singles[0]
    assert want is not None, "the greedy configuration must be comparable: pick other TEXTS"
    pool = runner.Pool(orpheus_gguf, n_workers=1, max_batch=4, continuous=True, sample=0, voice=b"zoe")
    ids = [pool.submit(t) for t in TEXTS[:5]]            # the pool's configuration: greedy, voice zoe
    ids += [pool.submit(t) for t in TEXTS[5:]]           # the second wave arrives while the session is running or just over; either way it joins one
    for i, tid in enumerate(ids):
        audio, bs, wk, err = pool.wait(tid, 60000)
        assert err == "" and np.array_equal(audio, want[i]), (i, err)
    st = pool.stats()
    assert st["tasks"] == len(TEXTS) and st["admitted_in_flight"] > 0 and st["largest_batch"] <= 4, st
    pool.close()
