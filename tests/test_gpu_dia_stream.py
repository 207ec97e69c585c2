"""The Dia continuous session (tts_hip_dia_stream_*): utterances enter and leave the slots of one fixed lock-step loop while the others keep
going.  An utterance's ids and step count must be exactly those of tts_hip_dia_generate on a fresh context with n_utt = n_slots, the utterance
in the same slot, its budget as max_gen and its uniforms in that slot's column: the same forward at the same row count, so no tolerance."""
import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

# <= 24 bytes (tiny max_ctx); a sixth sentence so that three slots are all used twice
TEXTS = ["[S1] first one.", "[S2] the second is long.", "[S1] hi.", "[S1] a [S2] b [S1] c.", "[S2] number five.", "[S1] and a sixth."]
FILLER = "[S1] somebody else."
EXTRA = (2, 9, 5, 18, 6, 11)      # budgets max_delay + these: 16, 23, 19, 32, 20 and 25 steps after their admissions
RUN = 4                           # steps per run: budgets 24 and 20 park on the last replay of a run, the others inside one
SAMPLING = dict(top_k=8, repetition_penalty=1.3)   # slot reuse must reset d_last / d_repc


def _args(cfg):
    return dict(delay_pattern=[0, 8, 9, 10, 11, 12, 13, 14, 15], bos=cfg.bos, eos=cfg.eos, pad=cfg.pad, max_delay=cfg.max_delay)


def _engine(model, n):
    eng = hip.DiaEngine(model.cfg, max_utterances=n)
    eng.load(model)
    return eng


def _session(eng, n_slots, utts, budgets, uniforms=None, run=RUN, **sampling):
    """utts [(tokens, len)] through one session: the first n_slots at once, the rest as slots free up (one admit call per look-in)
    -> (ids per utterance, slot per utterance, admissions made while other slots were live)"""
    cfg = eng.cfg
    eng.stream_begin(n_slots, cfg.max_gen, sampled=uniforms is not None, **sampling, **_args(cfg))
    out, slot_of, in_slot = [None] * len(utts), [None] * len(utts), {}
    free, nxt, refills = list(range(n_slots)), 0, 0

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
    assert not in_slot and nxt == len(utts)
    assert eng.stream_run(run) == []            # no live slot: nothing to launch, nothing to report
    eng.stream_end()
    return out, slot_of, refills


def _reference(model, n_slots, slot, utt, budget, filler, uniforms=None, **sampling):
    """tts_hip_dia_generate on a fresh context with n_utt = n_slots: the utterance in `slot`, any encoded sentence in the others"""
    cfg = model.cfg
    eng = _engine(model, n_slots)
    for s in range(n_slots):
        eng.encode_slot(s, *(utt if s == slot else filler))
    outs = [eng.generate(n_slots, budget, **_args(cfg))[slot]]
    if uniforms is not None:
        u = np.random.default_rng(99).random((budget, n_slots, cfg.n_out), dtype=np.float32)
        u[:, slot, :] = uniforms[:budget]
        outs.append(eng.generate(n_slots, budget, uniforms=u, **sampling, **_args(cfg))[slot])
    eng.close()
    return outs


@pytest.mark.parametrize("wtype", [gguf.F32, gguf.F16])
@pytest.mark.parametrize("n_slots", [2, 3])
def test_session_equals_lockstep_generation(n_slots, wtype):
    model = synth.build_dia(synth.dia_tiny(weight_type=wtype), suppress_special=True)
    cfg = model.cfg
    utts = [orc.dia_tokenize(t, cfg.max_ctx) for t in TEXTS]
    filler = orc.dia_tokenize(FILLER, cfg.max_ctx)
    budgets = [cfg.max_delay + e for e in EXTRA]
    assert all(cfg.max_delay < b <= cfg.max_gen for b in budgets)
    uni = np.random.default_rng(5).random((len(utts), cfg.max_gen, cfg.n_out), dtype=np.float32)
    eng = _engine(model, n_slots)
    greedy, slots, refills = _session(eng, n_slots, utts, budgets)
    assert refills >= 1 and sorted(set(slots)) == list(range(n_slots))
    assert all(slots.count(s) >= 2 for s in range(n_slots))                      # every slot is reused at least once
    sampled, slots_s, _ = _session(eng, n_slots, utts, budgets, uniforms=uni, **SAMPLING)   # the same context, the session's graph dropped and rebuilt
    assert slots_s == slots
    eng.close()
    one = _engine(model, 1)
    for u in range(len(utts)):
        ref_g, ref_s = _reference(model, n_slots, slots[u], utts[u], budgets[u], filler, uniforms=uni[u], **SAMPLING)
        assert len(ref_g) == budgets[u] - 1 == len(ref_s)                          # no EOS in this model: the countdown starts at budget - max_delay
        assert greedy[u].shape == ref_g.shape and np.array_equal(greedy[u], ref_g), (u, slots[u])
        assert sampled[u].shape == ref_s.shape and np.array_equal(sampled[u], ref_s), (u, slots[u])
        one.encode(*utts[u])
        assert np.array_equal(greedy[u], one.generate(1, budgets[u], **_args(cfg))[0]), u      # and the one-utterance generation, greedy
    one.close()
    assert not np.array_equal(sampled[0], greedy[0])


def test_parked_slots_do_not_disturb_live_ones():
    """three slots, only slot 1 ever admitted; slots 0 and 2 were never encoded and stay parked over the one cleared cross position"""
    model = synth.build_dia(synth.dia_tiny(), suppress_special=True)
    cfg = model.cfg
    utt, filler = orc.dia_tokenize(TEXTS[1], cfg.max_ctx), orc.dia_tokenize(FILLER, cfg.max_ctx)
    budget = cfg.max_delay + 12
    eng = _engine(model, 3)
    eng.stream_begin(3, cfg.max_gen, **_args(cfg))
    eng.stream_admit([1], [utt[0]], [utt[1]], budgets=[budget])
    fin = []
    for _ in range(20):
        fin += eng.stream_run(RUN)
        if fin:
            break
    assert fin == [(1, budget - 1)]
    got = eng.stream_collect(1, budget - 1)
    eng.stream_end()
    eng.close()
    ref = _reference(model, 3, 1, utt, budget, filler)[0]
    assert np.array_equal(got, ref)
    assert got.max() < cfg.audio_vocab           # ids out of finite logits: a NaN row would select id 0 everywhere, a garbage row a special id
    assert len(np.unique(got)) > 8


EOS_SEED, EOS_TOP_K, EOS_BUDGET, EOS_STEPS = 14, 16, 40, 18
# found on the CPU: orc.DiaOracle(build_dia(dia_tiny(), suppress_special=False)).generate("[S1] stop early.", max_tokens=40, pick=orc_sampler_sample with
# top_k 16 and np.random.default_rng(seed).random((max_gen, n_out), float32)[call]) for seeds 0..199: seed 14 draws EOS on head 0 at step 3 and
# stops after 3 + max_delay = 18 steps (12 -> 30, 18 -> 20, 31 -> 24, 38 -> 19 stop early too; most seeds run the 39 steps of the budget)


def test_session_finishing_at_admission_and_on_eos():
    """The two other ways to finish.  budget = max_delay + 1, the shortest there is: check_stopping starts the countdown at position
    budget - max_delay = 1, so max_delay sampler calls follow the admission (no budget ends AT the admission); the next run reports the slot with
    the step count tts_hip_dia_generate gives for that max_gen.  And EOS on head 0: a sampled utterance on a model that keeps its special-id head
    rows, with a seed found on the CPU oracle, stops before its budget."""
    model = synth.build_dia(synth.dia_tiny(), suppress_special=False)
    cfg = model.cfg
    filler = orc.dia_tokenize(FILLER, cfg.max_ctx)
    short, early = orc.dia_tokenize(TEXTS[0], cfg.max_ctx), orc.dia_tokenize("[S1] stop early.", cfg.max_ctx)
    uni = np.random.default_rng(EOS_SEED).random((cfg.max_gen, cfg.n_out), dtype=np.float32)
    eng = _engine(model, 2)
    # the shortest budget there is: the countdown starts at position 1, the next run reports the slot with tts_hip_dia_generate's step count
    eng.stream_begin(2, cfg.max_gen, **_args(cfg))
    eng.stream_admit([0], [short[0]], [short[1]], budgets=[cfg.max_delay + 1])
    fin = eng.stream_run(cfg.max_gen)
    ref = _reference(model, 2, 0, short, cfg.max_delay + 1, filler)[0]
    assert fin == [(0, len(ref))] and len(ref) == cfg.max_delay
    assert np.array_equal(eng.stream_collect(0, len(ref)), ref)
    eng.stream_end()
    # EOS on head 0 starts the countdown before the budget does
    eng.stream_begin(2, cfg.max_gen, sampled=True, top_k=EOS_TOP_K, **_args(cfg))
    eng.stream_admit([1], [early[0]], [early[1]], budgets=[EOS_BUDGET], uniforms=uni[None])
    fin = []
    for _ in range(EOS_BUDGET // RUN + 1):
        fin += eng.stream_run(RUN)
    got = eng.stream_collect(1, fin[0][1])
    eng.stream_end()
    eng.close()
    ref = _reference(model, 2, 1, early, EOS_BUDGET, filler, uniforms=uni, top_k=EOS_TOP_K)[1]
    assert fin == [(1, len(ref))] and np.array_equal(got, ref)
    assert len(ref) == EOS_STEPS < EOS_BUDGET - 1 and ref[EOS_STEPS - cfg.max_delay, 0] == cfg.eos


def test_session_misuse_is_refused_and_the_context_works_afterwards():
    model = synth.build_dia(synth.dia_tiny(), suppress_special=True)
    cfg = model.cfg
    a = _args(cfg)
    utts = [orc.dia_tokenize(t, cfg.max_ctx) for t in TEXTS[:3]]
    fresh = _engine(model, 3)
    for s in range(3):
        fresh.encode_slot(s, *utts[s])
    want = fresh.generate(3, 24, **a)
    fresh.close()
    eng = _engine(model, 3)
    with pytest.raises(hip.HipError, match="no session"):
        eng.stream_run(1)
    with pytest.raises(hip.HipError, match="max_utterances"):
        eng.stream_begin(4, cfg.max_gen, **a)
    with pytest.raises(hip.HipError, match="max_gen"):
        eng.stream_begin(2, cfg.max_gen + 1, **a)
    with pytest.raises(hip.HipError, match="temperature"):
        eng.stream_begin(2, cfg.max_gen, sampled=True, temperature=0.0, **a)
    eng.encode_slot(0, *utts[0])
    eng.gen_begin(1, 24, **a)
    eng.gen_launch(4)                                    # an unfinished gen_* loop: begin waits for it and drops it
    eng.stream_begin(2, cfg.max_gen, **a)
    eng.stream_admit([0], [utts[0][0]], [utts[0][1]], budgets=[24])
    with pytest.raises(hip.HipError, match="busy"):
        eng.stream_admit([0], [utts[1][0]], [utts[1][1]])
    with pytest.raises(hip.HipError, match="n_slots"):
        eng.stream_admit([2], [utts[1][0]], [utts[1][1]])            # max_utterances is 3, the session has 2 slots
    with pytest.raises(hip.HipError, match="twice"):
        eng.stream_admit([1, 1], [utts[1][0], utts[2][0]], [utts[1][1], utts[2][1]])
    for bad in (cfg.max_delay, cfg.max_gen + 1):
        with pytest.raises(hip.HipError, match="budget"):
            eng.stream_admit([1], [utts[1][0]], [utts[1][1]], budgets=[bad])
    for bad in (0, cfg.max_ctx + 1):
        with pytest.raises(hip.HipError, match="sentence length"):
            eng.stream_admit([1], [utts[1][0]], [bad])
    with pytest.raises(hip.HipError, match="not finished"):
        eng.stream_collect(0, 1)
    with pytest.raises(hip.HipError, match="not finished"):
        eng.stream_collect(1, 0)                                     # never admitted
    with pytest.raises(hip.HipError, match="n_slots"):
        eng.stream_collect(2, 1)
    ids = np.full((1, cfg.n_out), cfg.bos, dtype=np.uint32)
    for call in (lambda: eng.encode_slot(1, *utts[1]), lambda: eng.encode(*utts[1]), lambda: eng.step_batch(ids, [0]), lambda: eng.step(ids[0], 0),
                 lambda: eng.generate(1, 24, **a), lambda: eng.gen_begin(1, 24, **a), lambda: eng.gen_launch(1), lambda: eng.gen_wait(),
                 lambda: eng.stream_begin(2, cfg.max_gen, **a)):
        with pytest.raises(hip.HipError, match="session is open"):
            call()
    eng.stream_admit([1], [utts[1][0]], [utts[1][1]], budgets=[24])   # the refused calls left the session as it was
    fin = eng.stream_run(64)
    assert fin == [(0, 23), (1, 23)]
    with pytest.raises(hip.HipError, match="asked for"):
        eng.stream_collect(0, 24)
    got = [eng.stream_collect(s, n) for s, n in fin]
    eng.stream_admit([0], [utts[2][0]], [utts[2][1]], budgets=[24])   # a collected slot is free again
    with pytest.raises(hip.HipError, match="not finished"):
        eng.stream_collect(0, 1)
    assert eng.stream_run(64) == [(0, 23)]
    eng.stream_end()
    eng.stream_end()                                                  # idempotent
    sampled = _engine(model, 2)
    sampled.stream_begin(2, cfg.max_gen, sampled=True, top_k=8, **a)
    with pytest.raises(hip.HipError, match="uniforms"):
        sampled.stream_admit([0], [utts[0][0]], [utts[0][1]])
    sampled.stream_end()
    sampled.close()
    for s in range(3):                                                # after the session a plain generate works and equals a fresh context's
        eng.encode_slot(s, *utts[s])
    after = eng.generate(3, 24, **a)
    assert all(np.array_equal(x, y) for x, y in zip(after, want))
    assert np.array_equal(got[0], _reference(model, 2, 0, utts[0], 24, utts[1])[0])
    eng.close()


# ---- runner, C ABI and pool ---------------------------------------------------------------------------------------------------------------
RTEXTS = [" Hi there [S2] ok", "[S1] another one.", "[S2] short", "[S1] the fourth one.", "[S2] five [S1] and six", "[S1] last."]
CONFIGS = (dict(sample=0, max_tokens=30), dict(sample=1, top_k=8, seed=5, max_tokens=36))


@pytest.fixture(scope="module")
def dia_gguf(tmp_path_factory):
    # the special-id head rows stay: an EOS ends an utterance early where the sampler draws one (ragged lengths as such are the device tests' business)
    return synth.build_dia(synth.dia_tiny(), suppress_special=False).write_gguf(str(tmp_path_factory.mktemp("dia_stream") / "dia.gguf"))


@pytest.fixture(scope="module")
def singles(dia_gguf):
    """per configuration: (audio, still-delayed ids) of a generate() call per text"""
    from tts_cpp_amd import runner
    one = runner.Runner(dia_gguf, sample=0)
    out = []
    for kw in CONFIGS:
        res = []
        for t in RTEXTS:
            audio = one.generate(t, **kw)
            res.append((audio, one.last_tokens(1).copy()))
        out.append(res)
    one.close()
    return out


def test_runner_generate_stream_equals_single_calls(dia_gguf, singles):
    """dia_runner::stream_* under tts_c_generate_stream: six texts through a session of three slots.  Token streams identical to a generate()
    call of each text's own; audio within the 1e-5 of the batch test (the codec pass groups the utterances that finish together)."""
    from tts_cpp_amd import runner
    many = runner.Runner(dia_gguf, sample=0, max_seqs=3)
    for kw, want in zip(CONFIGS, singles):
        got = many.generate_stream(RTEXTS, **kw)
        assert len(got) == len(RTEXTS)
        for i, ((audio, toks), g) in enumerate(zip(want, got)):
            assert np.array_equal(many.last_tokens(16 + i), toks) and toks.size > 0, (kw, i)
            assert g.shape == audio.shape and (g.size == 0 or np.abs(g - audio).max() < 1e-5), (kw, i)
        assert sum(g.size > 0 for g in got) >= 3, kw
    assert np.array_equal(many.generate(RTEXTS[1], **CONFIGS[0]), singles[0][1][0])      # the runner generates as before after a session
    many.close()


def test_pool_continuous_mode_runs_dia_through_one_session(dia_gguf, singles):
    """pool_options::continuous reaches Dia through the virtual interface: two waves of requests, answered out of one session"""
    from tts_cpp_amd import runner
    want = singles[0]
    pool = runner.Pool(dia_gguf, n_workers=1, max_batch=3, continuous=True, **CONFIGS[0])
    ids = [pool.submit(t) for t in RTEXTS[:4]]
    ids += [pool.submit(t) for t in RTEXTS[4:]]          # the second wave arrives while the session is running or just over; either way it joins one
    for i, tid in enumerate(ids):
        audio, bs, wk, err = pool.wait(tid, 60000)
        assert err == "" and audio.shape == want[i][0].shape and (audio.size == 0 or np.abs(audio - want[i][0]).max() < 1e-5), (i, err)
    st = pool.stats()
    assert st["tasks"] == len(RTEXTS) and st["admitted_in_flight"] > 0 and st["largest_batch"] <= 3, st
    pool.close()
