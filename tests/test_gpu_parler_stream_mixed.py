"""The Parler mixed session (tts_hip_parler_stream_begin_mixed / _admit_mixed): requests that differ in sample, seed, top_k, top_p, temperature
or repetition penalty share one lock-step forward.
  engine      a session of 12 slots serving 40 utterances with four settings equals, utterance by utterance, the lock-step generation of all
              40 with that utterance's setting (tts_hip_parler_generate_greedy / _sampled: code the session does not go through); an all-greedy
              mixed session equals the uniform greedy session, also around a sampled guest; every misuse is refused and the session goes on
  runner      generate_stream(texts, configs=[...]) and the continuous pool: the audio of generate_batch(texts, **config) per configuration
The GEMM tile shape is pinned as in tests/test_gpu_parler.py::test_utterance_admitted_mid_flight_gets_the_tokens_of_its_own_run (a forward of 64
rows otherwise sums in another order than one of 40 x 60 prompt rows)."""
import numpy as np
import pytest

from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

PINS = {"TTS_HIP_TILE_FORCE": "3", "TTS_HIP_TILE_KS": "1", "TTS_HIP_ATTN_NSPLIT": "1", "TTS_HIP_ATTN_ROWS": "0"}
# None: sampler::max.  top_k, top_p, temperature, repetition penalty otherwise
SETTINGS = [None,
            dict(top_k=20, top_p=1.0, temperature=0.9, repetition_penalty=1.1),
            dict(top_k=0, top_p=0.8, temperature=1.2, repetition_penalty=1.0),
            dict(top_k=8, top_p=1.0, temperature=1.0, repetition_penalty=1.4)]
N, CAP, SLOTS = 40, 80, 12
MAX_STEPS = CAP - 1


def _penalised(s):
    return s is not None and s["repetition_penalty"] != 1.0


@pytest.fixture(scope="module")
def pins():
    with pytest.MonkeyPatch.context() as mp:
        for k, v in PINS.items():
            mp.setenv(k, v)
        yield


@pytest.fixture(scope="module")
def world(pins):
    """model, prompts, uniforms [step][utterance][head], and per setting the lock-step generation of all 40: (tokens [step][utt][head], steps [utt])"""
    cfg = synth.small(weight_type=gguf.F16, ctx=CAP, max_gen=CAP)
    model = synth.build(cfg)
    rng = np.random.default_rng(29)
    lens = rng.integers(4, 61, N)
    prompts = [rng.integers(3, cfg.prompt_vocab, int(l)).astype(np.uint32) for l in lens]
    n_steps = int(CAP - lens.min())
    uni = rng.random((n_steps, N, cfg.n_out), dtype=np.float32)
    refs = []
    for s in SETTINGS:
        ref = hip.HipEngine(cfg, max_seqs=N, kv_positions=CAP, flags=hip.FLAG_NO_DAC)
        ref.load(model)
        ref.prefill_batch(prompts)
        if s is None:
            rt, rd = ref.generate_greedy(lens, n_steps)
        else:
            rt, rd = ref.generate_sampled(lens, n_steps, uni, **s)
        ref.close()
        steps = np.where(rd > 0, rd, n_steps).astype(int)
        assert (steps <= CAP - lens).all()
        refs.append((rt.copy(), steps))
    assert not np.array_equal(refs[0][0], refs[1][0]) and not np.array_equal(refs[1][0], refs[3][0]), "the settings must matter"
    return dict(cfg=cfg, model=model, lens=lens, prompts=prompts, n_steps=n_steps, uni=uni, refs=refs)


def _engine(w, slots=SLOTS):
    eng = hip.HipEngine(w["cfg"], max_seqs=slots + 1, kv_positions=CAP, flags=hip.FLAG_NO_DAC)
    eng.load(w["model"])
    return eng


def _draws(w, us):
    u = np.zeros((len(us), MAX_STEPS, w["cfg"].n_out), dtype=np.float32)
    for i, k in enumerate(us):
        u[i, :w["n_steps"]] = w["uni"][:, k]
    return u


def _want(w, k, setting_index):
    rt, steps = w["refs"][setting_index]
    return int(steps[k]), rt[:int(steps[k]), k]


def _admit_mixed(eng, w, slots, us, settings):
    sampled = any(s is not None for s in settings)
    eng.stream_admit_mixed(slots, [w["prompts"][k] for k in us], settings, _draws(w, us) if sampled else None)


def _serve(eng, w, order, admit, slots=SLOTS, log=None):
    """the waiting list `order` through `slots` slots, look-ins every 32 steps, freed slots refilled -> {utterance: (steps, tokens)}"""
    waiting, slot_utt, free, got, rounds = list(order), {}, list(range(slots)), {}, 0
    while waiting or slot_utt:
        take = waiting[:len(free)]
        if take:
            waiting = waiting[len(take):]
            sl = [free.pop(0) for _ in take]
            if log is not None:
                log.append(("admit", list(zip(sl, take)), bool(slot_utt)))
            admit(sl, take)
            slot_utt.update(dict(zip(sl, take)))
        if log is not None:
            log.append(("run", sorted(slot_utt.values())))
        for slot, steps in eng.stream_run(32):
            k = slot_utt.pop(slot)
            got[k] = (steps, eng.stream_collect(slot, steps))
            free.append(slot)
        rounds += 1
        assert rounds < 100
    return got


def test_mixed_session_equals_each_utterances_own_lock_step_generation(world):
    """40 utterances, prompts of 4 ... 60 ids, the four settings dealt round-robin, through 12 slots (every forward is padded to 64 rows with rows
    of the padding slot 12).  Utterance u must get exactly the tokens and the step count of the lock-step generation of all 40 with u's setting."""
    w = world
    setting_of = [u % len(SETTINGS) for u in range(N)]
    eng = _engine(w)
    eng.stream_begin_mixed(SLOTS, MAX_STEPS)
    log = []
    got = _serve(eng, w, range(N), lambda sl, us: _admit_mixed(eng, w, sl, us, [SETTINGS[setting_of[k]] for k in us]), log=log)
    eng.stream_end()
    eng.close()
    assert len(got) == N
    for u in range(N):
        steps, toks = _want(w, u, setting_of[u])
        assert got[u][0] == steps, (u, SETTINGS[setting_of[u]], got[u][0], steps)
        assert np.array_equal(got[u][1], toks), f"utterance {u} ({w['lens'][u]} prompt ids, {SETTINGS[setting_of[u]]})"
    # the schedule must have exercised what the test is about
    runs = [e[1] for e in log if e[0] == "run"]
    assert any(len({setting_of[u] for u in live}) >= 3 for live in runs), "three distinct settings live in one run"
    assert any({setting_of[u] == 0 for u in live} == {True, False} for live in runs), "a greedy and a sampled row share a run"
    occupants = {}
    for e in log:
        if e[0] == "admit":
            for slot, u in e[1]:
                occupants.setdefault(slot, []).append(u)
    pairs = [(SETTINGS[setting_of[a]], SETTINGS[setting_of[b]]) for occ in occupants.values() for a, b in zip(occ, occ[1:])]
    assert any((a is None) != (b is None) for a, b in pairs), "a slot reused by an occupant of the other mode"
    assert any(not _penalised(a) and _penalised(b) for a, b in pairs), "a slot reused with a penalty after an occupant without one"
    assert any(_penalised(a) and not _penalised(b) for a, b in pairs), "a slot reused without a penalty after an occupant with one"
    assert sum(len(e[1]) for e in log if e[0] == "admit" and e[2]) >= N - SLOTS, "utterances joined mid-flight"


def test_all_greedy_mixed_session_equals_the_uniform_greedy_session(world):
    """The all-greedy mixed session replays the uniform session's arg-max step: same ids.  A sampled guest switches the runs it is live in to
    the mixed step and back; the greedy utterances around it keep their ids, and the guest gets its own."""
    w = world
    uni_eng = _engine(w)
    uni_eng.stream_begin(SLOTS, MAX_STEPS, sampling=None)
    want = _serve(uni_eng, w, range(N), lambda sl, us: uni_eng.stream_admit(sl, [w["prompts"][k] for k in us]))
    uni_eng.stream_end()
    uni_eng.close()
    eng = _engine(w)
    eng.stream_begin_mixed(SLOTS, MAX_STEPS)
    got = _serve(eng, w, range(N), lambda sl, us: _admit_mixed(eng, w, sl, us, [None] * len(us)))
    assert len(got) == len(want) == N
    for u in range(N):
        assert got[u][0] == want[u][0] and np.array_equal(got[u][1], want[u][1]), f"utterance {u}"
    # the same session goes on: greedy 0..5, one look-in later the sampled guest (utterance 6 with setting 1), then greedy 7..10 once it has left
    guest, done, live = 6, {}, {}

    def run():
        for slot, steps in eng.stream_run(32):
            done[live.pop(slot)] = (steps, eng.stream_collect(slot, steps))

    first = list(range(6))
    _admit_mixed(eng, w, list(range(6)), first, [None] * 6)
    live.update(dict(zip(range(6), first)))
    run()                                                     # all greedy
    assert len(live) >= 1, "greedy utterances must still be running when the guest arrives"
    _admit_mixed(eng, w, [6], [guest], [SETTINGS[1]])
    live[6] = guest
    rounds = 0
    while guest not in done:                                  # greedy and sampled rows in one step
        run()
        rounds += 1
        assert rounds < 10
    late = [7, 8, 9, 10]
    free = [s for s in range(SLOTS) if s not in live][:len(late)]
    _admit_mixed(eng, w, free, late, [None] * len(late))
    live.update(dict(zip(free, late)))
    while live:                                               # all greedy again
        run()
        rounds += 1
        assert rounds < 20
    eng.stream_end()
    eng.close()
    for u in first + late:
        assert done[u][0] == want[u][0] and np.array_equal(done[u][1], want[u][1]), f"greedy utterance {u} around the guest"
    steps, toks = _want(w, guest, 1)
    assert done[guest][0] == steps and np.array_equal(done[guest][1], toks), "the sampled guest"


def test_mixed_session_misuse_is_refused_and_the_session_goes_on(world):
    w = world
    slots = 6
    # a uniform session refuses the mixed admission and goes on
    eng = _engine(w, slots)
    eng.stream_begin(slots, MAX_STEPS, sampling=None)
    with pytest.raises(hip.HipError, match=r"opened by tts_hip_parler_stream_begin \(tts_hip_parler_stream_admit\)"):
        _admit_mixed(eng, w, [0], [0], [None])
    eng.stream_admit([0], [w["prompts"][0]])
    fin = []
    while not fin:
        fin = eng.stream_run(32)
    assert fin == [(0, _want(w, 0, 0)[0])] and np.array_equal(eng.stream_collect(0, fin[0][1]), _want(w, 0, 0)[1])
    eng.stream_end()
    eng.close()

    eng = _engine(w, slots)
    eng.stream_begin_mixed(slots, MAX_STEPS)
    live = {}   # slot -> (utterance, setting index)

    def valid(slot, u, si):
        _admit_mixed(eng, w, [slot], [u], [SETTINGS[si]])
        live[slot] = (u, si)

    with pytest.raises(hip.HipError, match=r"opened by tts_hip_parler_stream_begin_mixed \(tts_hip_parler_stream_admit_mixed\)"):   # the uniform admission
        eng.stream_admit([0], [w["prompts"][1]])
    valid(0, 1, 1)
    with pytest.raises(hip.HipError, match="uniforms"):                                 # a sampled setting without uniforms
        eng.stream_admit_mixed([1], [w["prompts"][2]], [SETTINGS[2]], None)
    valid(1, 2, 2)
    with pytest.raises(hip.HipError, match="temperature"):                              # the second of two is out of the sampler's limits
        eng.stream_admit_mixed([2, 3], [w["prompts"][3], w["prompts"][4]], [None, dict(SETTINGS[3], temperature=0.0)], _draws(w, [3, 4]))
    valid(2, 3, 3)                                                                      # ... and the first one's slot is still free
    with pytest.raises(hip.HipError, match="still generating"):                         # a busy slot
        _admit_mixed(eng, w, [0], [5], [None])
    valid(3, 4, 0)
    with pytest.raises(hip.HipError, match="named twice"):
        _admit_mixed(eng, w, [4, 4], [5, 6], [None, SETTINGS[1]])
    valid(4, 5, 1)
    with pytest.raises(hip.HipError, match="slot %d >= %d" % (slots, slots)):
        _admit_mixed(eng, w, [slots], [6], [None])
    valid(5, 6, 2)
    rounds = 0
    while live:
        for slot, steps in eng.stream_run(32):
            u, si = live.pop(slot)
            want_steps, want = _want(w, u, si)
            assert steps == want_steps and np.array_equal(eng.stream_collect(slot, steps), want), (u, SETTINGS[si])
        rounds += 1
        assert rounds < 10
    eng.stream_end()
    eng.close()


# ---- runner and pool ---------------------------------------------------------------------------------------------------------------------
# sample, seed, top_k, temperature and repetition_penalty differ
RCONFIGS = [dict(sample=0),
            dict(sample=1, seed=5, top_k=20, temperature=0.9, repetition_penalty=1.1),
            dict(sample=1, seed=11, top_k=8, temperature=1.2, repetition_penalty=1.0),
            dict(sample=1, seed=7, top_k=50, temperature=1.0, repetition_penalty=1.4)]
N_TEXTS = 24


@pytest.fixture(scope="module")
def served(pins, tmp_path_factory):
    """the GGUF, 24 texts, and per configuration the lock-step generate_batch of all 24 (the path the session does not go through).
    The yardstick batch holds the 24 texts twice, 48 rows: a lock-step forward of fewer than 33 rows (tile_min_rows) takes the 16-feature GEMM
    kernel, whose fp32 summation order the pins do not reach, while every forward of a session is padded to 64 rows and takes the pinned
    tiles.  With 24 rows the uniform generate_stream of the parent commit already differs from generate_batch in the ids themselves (greedy:
    14 of 24 utterances bit-equal, PCM apart by up to 0.67; sampled top_k 20 and top_k 50: 0 of 24, up to 0.78); with 48 rows they are bit for bit
    equal on the parent, so equality here is np.array_equal.  Rows 24 ... 47 repeat rows 0 ... 23 and must equal them (rows do not mix)."""
    from tts_cpp_amd import runner
    cfg = synth.small(weight_type=gguf.F16, ctx=96, max_gen=96)
    path = synth.build(cfg).write_gguf(str(tmp_path_factory.mktemp("parler_stream_mixed") / "small.gguf"))
    rng = np.random.default_rng(5)
    texts = [" ".join("w%d" % rng.integers(0, 50) for _ in range(int(rng.integers(1, 9)))) for _ in range(N_TEXTS)]
    yard = []
    for kw in RCONFIGS:
        r = runner.Runner(path, max_seqs=2 * N_TEXTS + 1, **kw)
        both = r.generate_batch(texts + texts)
        r.close()
        assert all(np.array_equal(a, b) for a, b in zip(both[:N_TEXTS], both[N_TEXTS:])), kw
        yard.append(both[:N_TEXTS])
    assert all(a.size > 0 for a in yard[0]) and len({a.size for a in yard[0]}) > 3, "a ragged set of utterances"
    assert all(sum(a.size > 0 for a in y) >= N_TEXTS // 2 for y in yard), "most sampled utterances must have audio"
    assert not np.array_equal(yard[1][0], yard[0][0]) and not np.array_equal(yard[1][0], yard[3][0]), "the configurations must matter"
    return dict(path=path, texts=texts, yard=yard, configs=[RCONFIGS[i % len(RCONFIGS)] for i in range(N_TEXTS)])


def test_runner_generate_stream_with_per_text_configs_equals_the_lock_step_batches(served):
    """parler_runner's mixed session under tts_c_generate_stream_configs: 24 texts, the four configurations in turn, through 8 rows.  The
    session's audio is bit for bit that of generate_batch: the decoder's ids are equal, and the codec works utterance by utterance."""
    from tts_cpp_amd import runner
    s = served
    many = runner.Runner(s["path"], max_seqs=9, sample=0)
    got = many.generate_stream(s["texts"], configs=s["configs"])
    assert len(got) == N_TEXTS
    for i, g in enumerate(got):
        assert np.array_equal(g, s["yard"][i % len(RCONFIGS)][i]), (i, s["configs"][i])
    # the runner generates as before after a session
    one = runner.Runner(s["path"], sample=0)
    for i in (2, 4):
        alone = one.generate(s["texts"][i], **s["configs"][i])
        assert alone.size > 0 and np.array_equal(many.generate(s["texts"][i], **s["configs"][i]), alone), i
    one.close()
    many.close()


def test_pool_continuous_mode_takes_differing_parler_requests_into_one_session(served):
    """the 24 requests through a continuous pool of 8 rows: parler_runner::stream_accepts takes them, so they join the open session in flight; the
    pool opens no more sessions than for 24 requests with identical configurations"""
    from tts_cpp_amd import runner
    s = served

    def serve(configs):
        pool = runner.Pool(s["path"], n_workers=1, max_batch=8, continuous=True, **RCONFIGS[0])
        ids = [pool.submit(t, **kw) for t, kw in zip(s["texts"], configs)]
        out = [pool.wait(tid, 60000) for tid in ids]
        st = pool.stats()
        pool.close()
        return out, st

    _, st_same = serve([RCONFIGS[0]] * N_TEXTS)
    mixed, st = serve(s["configs"])
    for i, (audio, bs, wk, err) in enumerate(mixed):
        assert err == "" and np.array_equal(audio, s["yard"][i % len(RCONFIGS)][i]), (i, s["configs"][i], err)
    assert st["tasks"] == N_TEXTS and st["batches"] <= st_same["batches"] and st["admitted_in_flight"] > 0, (st, st_same)
