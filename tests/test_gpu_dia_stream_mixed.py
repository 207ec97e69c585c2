"""The Dia mixed session (tts_hip_dia_stream_begin_mixed / _admit_mixed): every slot of the one device loop carries its own sampler record,
penalty table, uniforms and step budget, so requests that differ in sampler, seed or length share one captured graph.

Bars, all exact (the same kernels on the same device, so no tolerance and no CDF-boundary allowance):
  selection   tts_hip_sample_logits_rows_mixed == tts_hip_sample_logits called once per row with that row's settings, id for id and state
              for state; greedy rows == argmax (first maximum wins) with their state untouched
  session     an utterance's ids and step count == tts_hip_dia_generate on a fresh context with n_utt = n_slots, the utterance in the same
              slot, max_gen = its budget, its own sampler (NULL for greedy) and its uniforms in that slot's column
  runner      generate_stream(texts, configs=[...]) and the continuous pool: the ids of generate(text, **config); audio within the 1e-5 of
              test_gpu_dia_stream.py (the finished utterances of an interval share one batched codec pass)"""
import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

MARK = 0xFFFFFFFF


# ---- 1. the selection, per row ---------------------------------------------------------------------------------------------------------------
def _s(top_k, top_p, temperature, rep):
    return dict(top_k=top_k, top_p=top_p, temperature=temperature, repetition_penalty=rep)


ROWS = [_s(50, 1.0, 1.0, 1.0), _s(8, 1.0, 0.9, 1.5), _s(0, 0.8, 1.3, 1.0),      # [2]: nucleus only, the full-vocabulary sort
        _s(20, 0.95, 0.9, 1.2), _s(2000, 1.0, 1.5, 1.0), None, _s(1, 1.0, 1.0, 1.0), None]   # [4]: top_k >= vocabulary, disabled


def test_mixed_selection_equals_the_one_setting_sampler_per_row():
    cfg = synth.small(weight_type=gguf.F32)
    model = synth.build(cfg)
    eng = hip.HipEngine(cfg, max_seqs=8, flags=hip.FLAG_NO_DAC)
    eng.load(model)
    nh, v = cfg.n_out, cfg.out_vocab
    assert (nh, v) == (9, 1088)                                  # not a power of two: the sort pads
    rng = np.random.default_rng(2024)
    rows = len(ROWS)
    greedy = [r for r in range(rows) if ROWS[r] is None]
    last = rng.integers(-1, v, (rows, nh)).astype(np.int32)      # non-trivial state
    counts = rng.integers(1, 6, (rows, nh)).astype(np.uint32)
    last0, counts0 = last.copy(), counts.copy()
    last_ref, counts_ref = last.copy(), counts.copy()
    for call in range(3):
        lg = (rng.standard_normal((rows, nh, v)) * 3.0).astype(np.float32)
        if call == 1:   # the last token is the arg-max: its penalised value decides the maximum
            for r in range(rows):
                for h in range(nh):
                    if last[r, h] >= 0:
                        lg[r, h, last[r, h]] = 9.0
        for r in greedy:   # an exact tie at the top: the lower index wins
            for h in range(nh):
                lo, hi = sorted(rng.choice(v, 2, replace=False))
                lg[r, h, lo] = lg[r, h, hi] = 20.0
        u = rng.random((rows, nh)).astype(np.float32)
        got = eng.sample_logits_rows_mixed(lg, ROWS, uniforms=u, last_ids=last, rep_counts=counts)
        ref = np.zeros_like(got)
        for r in range(rows):
            if ROWS[r] is None:
                ref[r] = lg[r].argmax(-1)                        # numpy: the first maximum
            else:
                ref[r] = eng.sample_logits(lg[r:r + 1], u[r:r + 1], last_ids=last_ref[r:r + 1], rep_counts=counts_ref[r:r + 1], **ROWS[r])[0]
        assert np.array_equal(got, ref), (call, np.argwhere(got != ref))
        assert np.array_equal(last, last_ref) and np.array_equal(counts, counts_ref), call
        assert np.array_equal(last[greedy], last0[greedy]) and np.array_equal(counts[greedy], counts0[greedy])   # greedy rows: state untouched
        for r in range(rows):
            if ROWS[r] is not None and ROWS[r]["repetition_penalty"] != 1.0:
                assert np.array_equal(last[r], got[r].astype(np.int32)), (call, r)                                # penalised rows: state moved
    assert np.array_equal(got[6], lg[6].argmax(-1))              # top_k 1 is the arg-max too
    # all rows greedy: no uniforms, no state
    lg = (rng.standard_normal((3, nh, v)) * 3.0).astype(np.float32)
    assert np.array_equal(eng.sample_logits_rows_mixed(lg, [None] * 3), lg.argmax(-1))
    with pytest.raises(hip.HipError, match="uniforms"):
        eng.sample_logits_rows_mixed(lg, [None, _s(8, 1.0, 1.0, 1.0), None])
    with pytest.raises(hip.HipError, match="temperature"):
        eng.sample_logits_rows_mixed(lg, [None, _s(8, 1.0, 0.0, 1.0), None], uniforms=np.zeros((3, nh), dtype=np.float32))
    eng.close()


# ---- 2. the session --------------------------------------------------------------------------------------------------------------------------
TEXTS = ["[S1] first one.", "[S2] the second is long.", "[S1] hi.", "[S1] a [S2] b [S1] c.", "[S2] number five.", "[S1] and a sixth.", "[S2] seven."]
FILLER = "[S1] somebody else."
EXTRA = (2, 9, 5, 18, 6, 11, 7)        # budgets max_delay + these
A = dict(top_k=8, repetition_penalty=1.3)
B = dict(top_k=20, top_p=0.9, temperature=0.8, repetition_penalty=1.1)
Cs = dict(top_k=0, temperature=1.4)
SETTINGS = [A, A, None, B, None, Cs, A]   # in admission order
# The slot each utterance waits for.  Utterances 0 and 2 park inside the same look-in interval (16 and 19 sampler calls), so slots 0 and 2 come
# free together; B takes slot 0 (A -> B) and the greedy utterance 4 waits for slot 1 (A -> greedy), which leaves slot 2 parked and free for a
# few steps beside two live slots; the last A follows that greedy one (greedy -> A).  A stale record, table or state shows in one of them.
PLAN = [0, 1, 2, 0, 1, 2, 1]
N_SLOTS = 3


def _args(cfg):
    return dict(delay_pattern=[0, 8, 9, 10, 11, 12, 13, 14, 15], bos=cfg.bos, eos=cfg.eos, pad=cfg.pad, max_delay=cfg.max_delay)


def _engine(model, n):
    eng = hip.DiaEngine(model.cfg, max_utterances=n)
    eng.load(model)
    return eng


def _penalised(s):
    return s is not None and s.get("repetition_penalty", 1.0) != 1.0


def _reference(model, n_slots, slot, utt, budget, filler, uniforms, setting):
    """tts_hip_dia_generate on a fresh context with n_utt = n_slots: the utterance in `slot`, any encoded sentence in the others, its budget as
    max_gen, its own sampler (greedy: none) and its uniforms in that slot's column"""
    cfg = model.cfg
    eng = _engine(model, n_slots)
    for s in range(n_slots):
        eng.encode_slot(s, *(utt if s == slot else filler))
    if setting is None:
        out = eng.generate(n_slots, budget, **_args(cfg))[slot]
    else:
        u = np.random.default_rng(99).random((budget, n_slots, cfg.n_out), dtype=np.float32)
        u[:, slot, :] = uniforms[:budget]
        out = eng.generate(n_slots, budget, uniforms=u, **setting, **_args(cfg))[slot]
    eng.close()
    return out


def _admit(eng, take, utts, budgets, settings, uni):
    eng.stream_admit_mixed([s for s, _ in take], [utts[u][0] for _, u in take], [utts[u][1] for _, u in take], [settings[u] for _, u in take],
                           budgets=[budgets[u] for _, u in take],
                           uniforms=None if all(settings[u] is None for _, u in take) else np.stack([uni[u] for _, u in take]))


def _mixed_session(eng, utts, budgets, settings, uni, plan, launch):
    """the utterances in order, each into the slot `plan` names as soon as that slot is free (one admission per look-in).  launch == 0: run(4) and
    collect; else launch(launch) / wait taking rows, which must tile each occupant's history -> (ids per utterance, occupants per slot)"""
    cfg = eng.cfg
    eng.stream_begin_mixed(N_SLOTS, cfg.max_gen, **_args(cfg))
    out, in_slot, nxt = [None] * len(utts), {}, 0
    occupants = [[] for _ in range(N_SLOTS)]
    have, pieces = [0] * N_SLOTS, {}
    buf = eng._stream_out[0]

    def admit():
        nonlocal nxt
        take = []
        while nxt < len(utts) and plan[nxt] not in in_slot:
            take.append((plan[nxt], nxt))
            in_slot[plan[nxt]] = nxt
            nxt += 1
        if take:
            _admit(eng, take, utts, budgets, settings, uni)
            for s, u in take:
                occupants[s].append(u)
                have[s], pieces[u] = 0, []
                buf[s] = MARK

    admit()
    for _ in range(200):
        if not in_slot:
            break
        if launch == 0:
            fin = eng.stream_run(4)
        else:
            eng.stream_launch(launch)
            _, steps, done, fin = eng.stream_wait()
            for s, u in in_slot.items():
                n = int(steps[s])
                assert n >= have[s] and not (buf[s, :n] == MARK).any() and (buf[s, n:] == MARK).all(), (s, u, n)
                pieces[u].append(buf[s, have[s]:n].copy())
                have[s] = n
        for s, steps_s in fin:
            u = in_slot.pop(s)
            out[u] = eng.stream_collect(s, steps_s)
            if launch:
                assert np.array_equal(np.concatenate(pieces[u]), out[u]), u      # the rows the waits handed out tile the history
        admit()
    assert not in_slot and nxt == len(utts)
    eng.stream_end()
    return out, occupants


def _uniform_session(eng, utts, uni, budget, **sampling):
    """three utterances through a session opened by stream_begin with one sampler"""
    cfg = eng.cfg
    eng.stream_begin(N_SLOTS, cfg.max_gen, sampled=True, **sampling, **_args(cfg))
    eng.stream_admit(list(range(N_SLOTS)), [utts[u][0] for u in range(N_SLOTS)], [utts[u][1] for u in range(N_SLOTS)], budgets=[budget] * N_SLOTS,
                     uniforms=np.stack([uni[u] for u in range(N_SLOTS)]))
    fin = eng.stream_run(cfg.max_gen)
    assert [s for s, _ in fin] == list(range(N_SLOTS))
    out = [eng.stream_collect(s, n) for s, n in fin]
    eng.stream_end()
    return out


@pytest.mark.parametrize("wtype", [gguf.F32, gguf.F16])
def test_mixed_session_equals_each_utterances_own_generation(wtype):
    model = synth.build_dia(synth.dia_tiny(weight_type=wtype), suppress_special=True)
    cfg = model.cfg
    utts = [orc.dia_tokenize(t, cfg.max_ctx) for t in TEXTS]
    filler = orc.dia_tokenize(FILLER, cfg.max_ctx)
    budgets = [cfg.max_delay + e for e in EXTRA]
    assert all(cfg.max_delay < b <= cfg.max_gen for b in budgets)
    uni = np.random.default_rng(5).random((len(utts), cfg.max_gen, cfg.n_out), dtype=np.float32)
    eng = _engine(model, N_SLOTS)
    # the other two loops of this context first: their graphs exist before the mixed session's does
    for s in range(N_SLOTS):
        eng.encode_slot(s, *utts[s])
    u3 = np.ascontiguousarray(uni[:N_SLOTS, :24].transpose(1, 0, 2))
    gen_before = eng.generate(N_SLOTS, 24, uniforms=u3, **B, **_args(cfg))
    sess_before = _uniform_session(eng, utts, uni, 24, **A)

    by_run, occ = _mixed_session(eng, utts, budgets, SETTINGS, uni, PLAN, 0)
    by_wait, occ_w = _mixed_session(eng, utts, budgets, SETTINGS, uni, PLAN, 5)
    assert occ == occ_w == [[0, 3], [1, 4, 6], [2, 5]]
    assert all(len(o) >= 2 for o in occ)                                                          # every slot is reused
    pairs = [(SETTINGS[a], SETTINGS[b]) for o in occ for a, b in zip(o, o[1:])]
    assert any(_penalised(a) and b is None for a, b in pairs)                                     # sampled with penalty -> greedy
    assert any(a is None and _penalised(b) for a, b in pairs)                                     # greedy -> sampled with penalty
    assert any(a is A and b is B for a, b in pairs)                                               # one sampler -> another
    for u in range(len(utts)):
        ref = _reference(model, N_SLOTS, PLAN[u], utts[u], budgets[u], filler, uni[u], SETTINGS[u])
        assert len(ref) == budgets[u] - 1                                                         # no EOS in this model
        assert by_run[u].shape == ref.shape and np.array_equal(by_run[u], ref), (u, PLAN[u], SETTINGS[u])
        assert by_wait[u].shape == ref.shape and np.array_equal(by_wait[u], ref), (u, PLAN[u], SETTINGS[u])
    assert not np.array_equal(by_run[0][:16], by_run[3][:16])                                     # slot 0: the second occupant is not the first again

    # the uniform session and the fixed batch afterwards, on the same context: their graphs hold their own arguments still
    sess_after = _uniform_session(eng, utts, uni, 24, **A)
    for s in range(N_SLOTS):
        eng.encode_slot(s, *utts[s])
    gen_after = eng.generate(N_SLOTS, 24, uniforms=u3, **B, **_args(cfg))
    assert all(np.array_equal(x, y) for x, y in zip(sess_before, sess_after))
    assert all(np.array_equal(x, y) for x, y in zip(gen_before, gen_after))
    for s in range(N_SLOTS):   # ... and those are what a fresh context gives
        assert np.array_equal(sess_after[s], _reference(model, N_SLOTS, s, utts[s], 24, filler, uni[s], A)), s
    eng.close()
    fresh = _engine(model, N_SLOTS)
    for s in range(N_SLOTS):
        fresh.encode_slot(s, *utts[s])
    want = fresh.generate(N_SLOTS, 24, uniforms=u3, **B, **_args(cfg))
    fresh.close()
    assert all(np.array_equal(x, y) for x, y in zip(gen_after, want))


# ---- 3. misuse -------------------------------------------------------------------------------------------------------------------------------
def test_mixed_session_misuse_is_refused_and_the_session_goes_on():
    model = synth.build_dia(synth.dia_tiny(), suppress_special=True)
    cfg = model.cfg
    a = _args(cfg)
    utts = [orc.dia_tokenize(t, cfg.max_ctx) for t in TEXTS[:3]]
    filler = orc.dia_tokenize(FILLER, cfg.max_ctx)
    uni = np.random.default_rng(8).random((3, cfg.max_gen, cfg.n_out), dtype=np.float32)
    eng = _engine(model, 2)
    with pytest.raises(hip.HipError, match="no session"):
        _admit(eng, [(0, 0)], utts, [24] * 3, [A] * 3, uni)
    with pytest.raises(hip.HipError, match="max_utterances"):
        eng.stream_begin_mixed(3, cfg.max_gen, **a)
    eng.stream_begin_mixed(2, cfg.max_gen, **a)
    with pytest.raises(hip.HipError, match="utterance 1: temperature"):                     # all n are checked before anything is launched
        _admit(eng, [(0, 0), (1, 1)], utts, [24] * 3, [A, dict(top_k=8, temperature=0.0), None], uni)
    with pytest.raises(hip.HipError, match="uniforms"):                                     # a sampled utterance without uniforms
        eng.stream_admit_mixed([0], [utts[0][0]], [utts[0][1]], [A], budgets=[24])
    with pytest.raises(hip.HipError, match="begin_mixed"):                                  # admit on a mixed session
        eng.stream_admit([0], [utts[0][0]], [utts[0][1]], budgets=[24])
    assert eng.stream_run(4) == []                                                          # nobody was admitted: nothing to launch
    _admit(eng, [(0, 2)], utts, [24] * 3, [A, B, None], uni)                                # slot 0: greedy
    with pytest.raises(hip.HipError, match="busy"):
        _admit(eng, [(0, 1)], utts, [24] * 3, [A, B, None], uni)
    with pytest.raises(hip.HipError, match="busy"):                                         # ... also as the second of two: slot 1 stays free
        _admit(eng, [(1, 1), (0, 0)], utts, [24] * 3, [A, B, None], uni)
    _admit(eng, [(1, 1)], utts, [24] * 3, [A, B, None], uni)                                # slot 1: B
    fin = eng.stream_run(64)
    assert fin == [(0, 23), (1, 23)]
    assert np.array_equal(eng.stream_collect(0, 23), _reference(model, 2, 0, utts[2], 24, filler, uni[2], None))
    assert np.array_equal(eng.stream_collect(1, 23), _reference(model, 2, 1, utts[1], 24, filler, uni[1], B))
    eng.stream_end()
    # admit_mixed on a session opened by begin
    eng.stream_begin(2, cfg.max_gen, **a)
    with pytest.raises(hip.HipError, match="opened by tts_hip_dia_stream_begin "):
        _admit(eng, [(0, 0)], utts, [24] * 3, [None] * 3, uni)
    eng.stream_admit([0], [utts[2][0]], [utts[2][1]], budgets=[24])
    assert eng.stream_run(64) == [(0, 23)]
    assert np.array_equal(eng.stream_collect(0, 23), _reference(model, 2, 0, utts[2], 24, filler, uni[2], None))
    eng.stream_end()
    eng.close()


# ---- 4, 5. runner, C API and pool ------------------------------------------------------------------------------------------------------------
RTEXTS = [" Hi there [S2] ok", "[S1] another one.", "[S2] short", "[S1] the fourth one.", "[S2] five [S1] and six", "[S1] last."]
# sample, seed, top_k, temperature, repetition_penalty and max_tokens all differ; no max_tokens exceeds the first one's, which sizes the session
RCONFIGS = [dict(sample=1, top_k=8, seed=5, max_tokens=36), dict(sample=0, max_tokens=30),
            dict(sample=1, top_k=20, temperature=0.8, repetition_penalty=1.1, seed=11, max_tokens=30), dict(sample=0, max_tokens=24),
            dict(sample=1, top_k=8, temperature=1.2, repetition_penalty=1.3, seed=7, max_tokens=36), dict(sample=1, top_k=4, seed=5, max_tokens=24)]


@pytest.fixture(scope="module")
def dia_gguf(tmp_path_factory):
    # the special-id head rows stay: an EOS ends an utterance early where the sampler draws one
    return synth.build_dia(synth.dia_tiny(), suppress_special=False).write_gguf(str(tmp_path_factory.mktemp("dia_stream_mixed") / "dia.gguf"))


@pytest.fixture(scope="module")
def singles(dia_gguf):
    """(audio, still-delayed ids) of a fresh generate(text, **config) per request"""
    from tts_cpp_amd import runner
    one = runner.Runner(dia_gguf, sample=0)
    out = []
    for t, kw in zip(RTEXTS, RCONFIGS):
        audio = one.generate(t, **kw)
        out.append((audio, one.last_tokens(1).copy()))
    one.close()
    assert sum(a.size > 0 for a, _ in out) >= 3, "pick other RTEXTS / seeds: fewer than three utterances have audio"
    return out


def test_runner_generate_stream_with_per_text_configs_equals_single_calls(dia_gguf, singles):
    """dia_runner's mixed session under tts_c_generate_stream_configs: six texts, each with its own sampler, seed and length, through three slots"""
    from tts_cpp_amd import runner
    many = runner.Runner(dia_gguf, sample=0, max_seqs=3)
    got = many.generate_stream(RTEXTS, configs=RCONFIGS)
    assert len(got) == len(RTEXTS)
    for i, ((audio, toks), g) in enumerate(zip(singles, got)):
        assert np.array_equal(many.last_tokens(16 + i), toks) and toks.size > 0, (i, RCONFIGS[i])
        assert g.shape == audio.shape and (g.size == 0 or np.abs(g - audio).max() < 1e-5), (i, RCONFIGS[i])
    assert sum(g.size > 0 for g in got) >= 3
    # a request longer than the session was opened for is not accepted: the session drains and reopens for it, the outputs stay the same
    order = [1, 0, 3]
    got = many.generate_stream([RTEXTS[i] for i in order], configs=[RCONFIGS[i] for i in order])
    for i, g in zip(order, got):
        assert g.shape == singles[i][0].shape and (g.size == 0 or np.abs(g - singles[i][0]).max() < 1e-5), i
    assert np.array_equal(many.generate(RTEXTS[2], **RCONFIGS[2]), singles[2][0])        # the runner generates as before after a session
    assert np.array_equal(many.last_tokens(1), singles[2][1])
    many.close()


def test_pool_continuous_mode_takes_differing_dia_requests_into_one_session(dia_gguf, singles):
    """the six requests through a continuous pool of three slots: dia_runner::stream_accepts takes them, so they are answered out of ONE session,
    joining it in flight; the pool opens no more sessions than for six requests with identical configurations"""
    from tts_cpp_amd import runner

    def serve(requests):
        pool = runner.Pool(dia_gguf, n_workers=1, max_batch=3, continuous=True, **RCONFIGS[0])
        ids = [pool.submit(t, **kw) for t, kw in requests]
        out = [pool.wait(tid, 60000) for tid in ids]
        st = pool.stats()
        pool.close()
        return out, st

    _, st_same = serve([(t, RCONFIGS[0]) for t in RTEXTS])
    mixed, st = serve(list(zip(RTEXTS, RCONFIGS)))
    for i, ((want, _), (audio, bs, wk, err)) in enumerate(zip(singles, mixed)):
        assert err == "" and audio.shape == want.shape and (audio.size == 0 or np.abs(audio - want).max() < 1e-5), (i, RCONFIGS[i], err)
    assert st["tasks"] == 6 and st["largest_batch"] <= 3, st
    assert st["batches"] == 1 and st["admitted_in_flight"] > 0 and st["batches"] <= st_same["batches"], (st, st_same)
