"""Per-request voice descriptions in one lock-step forward (tts_hip_parler_voice_bank / _voice_set / _seq_voices, attn_short_voices_kernel).
  forward     rows spread over the context's own description (voice 0) and five bank voices of 8, 9, 16, 17 and 32 positions: the logits of every
              row with voice v are bit for bit those of a context whose own description is v's encoding, run unfolded (tune cross_fold = 0) over
              the same rows; the oracle and the folded one-description forward within the project's tolerances
  no bank     a bank nobody uses changes nothing: same logits, same tokens, the fold still taken
  loops       generate_greedy / _sampled and a mixed session whose slots change voice from one occupant to the next
  refusals    every misuse returns an error that names the call, and the context goes on
The GEMM tile shape is pinned where a forward has 33 rows or more, as in tests/test_gpu_parler.py / test_gpu_parler_stream_mixed.py."""
import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

TOL = {gguf.F32: 2e-4, gguf.F16: 2e-3, gguf.Q8_0: 3e-2}   # the project's bars: fp32, fp16, the integer path (one flipped Q8_0 activation code)
VOICE_LENS = [8, 9, 16, 17, 32]                            # both sides of every TN boundary of attn_short_body<8 | 16 | 32>
PINS = {"TTS_HIP_TILE_FORCE": "3", "TTS_HIP_TILE_KS": "1", "TTS_HIP_ATTN_NSPLIT": "1", "TTS_HIP_ATTN_ROWS": "0"}


def relerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / (np.abs(b).max() + 1e-30))


_models = {}


def wide_model(wtype, enc=8):
    key = (wtype, enc)
    if key not in _models:
        _models[key] = synth.build(synth.tiny(hidden=1024, heads=16, ffn=4096, layers=1, enc_len=enc, weight_type=wtype))
    return _models[key]


def encodings(hidden, lens, seed=41):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((n, hidden)) * 0.5).astype(np.float32) for n in lens]


def _flat_rows(prompts):
    """the rows of prefill_batch's forward: (sequence, position) in order"""
    return [s for s, p in enumerate(prompts) for _ in p]


@pytest.mark.parametrize("rows,wtype,enc", [
    (3, gguf.F16, 8), (12, gguf.F16, 8), (40, gguf.F16, 8), (100, gguf.F16, 8), (40, gguf.F16, 27),
    (3, gguf.F32, 8), (12, gguf.F32, 8), (40, gguf.F32, 8), (100, gguf.F32, 8),
    (100, gguf.Q8_0, 8),
])
def test_mixed_forward_equals_each_voices_own_unfolded_forward(rows, wtype, enc, monkeypatch):
    """3 rows: the <= 4-row chain; 12: the few-row GEMMs; 40 and 100: the tiled GEMMs (64 x 64 tiles forced, the shape the fold needs).  One
    prefill_batch (its hidden rows, debug_read "x") and one step (its logits)."""
    if rows >= 33:
        monkeypatch.setenv("TTS_HIP_TILE_FORCE", "3")
    model = wide_model(wtype, enc)
    cfg = model.cfg
    H = cfg.hidden
    encs = [None] + encodings(H, VOICE_LENS)
    rng = np.random.default_rng(rows * 3 + enc)
    prompts = [rng.integers(3, cfg.prompt_vocab, 2 + (i % 3)).astype(np.uint32) for i in range(rows)]
    pos = [len(p) for p in prompts]
    ids = rng.integers(0, cfg.audio_vocab, (rows, cfg.n_out)).astype(np.uint32)
    voice_of = np.array([(r * 5 + r // 6) % 6 for r in range(rows)])
    assert 0 in voice_of and len(set(voice_of.tolist())) == min(rows, 6)
    flat = np.array(_flat_rows(prompts))
    n_flat = len(flat)

    def forward(eng):
        eng.prefill_batch(prompts)
        x = eng.debug_read("x", n_flat * H).reshape(-1, H)    # the rows of the call's last forward (a forward carries up to 256 or 1024 rows)
        return x, eng.step(ids, pos)

    mixed = hip.HipEngine(cfg, max_seqs=rows, kv_positions=16)
    mixed.load(model)
    mixed.voice_bank(len(VOICE_LENS))
    for v in range(1, 6):
        mixed.voice_set(v, encs[v])
    mixed.seq_voices(np.arange(rows), voice_of)
    xm, lm = forward(mixed)
    assert np.isfinite(lm).all()
    lm2 = mixed.step(ids, pos)           # the captured step replayed
    assert np.array_equal(lm, lm2)

    for v in sorted(set(voice_of.tolist())):
        sel = voice_of == v
        out = {}
        for fold in (0, 1):
            one = hip.HipEngine(cfg, max_seqs=rows, kv_positions=16, tune={"cross_fold": fold})
            one.load(model)
            if v:
                one.set_text_encoding(encs[v])
            out[fold] = forward(one)
            if fold == 0 and v:
                n = VOICE_LENS[v - 1]
                for kv in (0, 1):
                    assert np.array_equal(mixed.debug_read(f"voice:{v}:0:{kv}", n * H), one.debug_read(f"cross:0:{kv}", n * H)), (v, kv)
            one.close()
        x0, l0 = out[0]
        assert np.array_equal(lm[sel], l0[sel]), f"rows of voice {v}: logits differ from the unfolded one-description forward"
        fs = sel[flat[n_flat - len(xm):]]
        assert len(x0) == len(xm) and fs.any() and np.array_equal(xm[fs], x0[fs]), f"rows of voice {v}: prefill hidden rows differ"
        # the folded forward sums the scores in another order
        assert relerr(lm[sel], out[1][1][sel]) < TOL[wtype], (v, relerr(lm[sel], out[1][1][sel]))
        # the oracle on a model whose description is this voice's
        r = int(np.flatnonzero(sel)[-1])
        o = orc.ParlerOracle(model, act_mode=1, gelu_mode=1)
        if v:
            o.set_text_encoding(encs[v])
        o.decode(prompts[r], 0, audio=False, want_logits=False)
        ref, _ = o.decode(ids[r], pos[r], audio=True)
        assert relerr(lm[r], ref[:, 0, :]) < TOL[wtype], (rows, v, r, relerr(lm[r], ref[:, 0, :]))
    mixed.close()


def test_mixed_forward_launches_one_attention_per_layer_and_voices_matter(monkeypatch):
    """the same prompt and ids in every row: rows differ exactly where their voices do; the profile shows the new launch in the ATTN_CROSS class"""
    monkeypatch.setenv("TTS_HIP_TILE_FORCE", "3")
    model = wide_model(gguf.F16)
    cfg = model.cfg
    rows = 40
    encs = [None] + encodings(cfg.hidden, VOICE_LENS)
    eng = hip.HipEngine(cfg, max_seqs=rows, kv_positions=16)
    eng.load(model)
    eng.voice_bank(5)
    for v in range(1, 6):
        eng.voice_set(v, encs[v])
    voice_of = np.arange(rows) % 6
    eng.seq_voices(np.arange(rows), voice_of)
    prompt = np.array([5, 9, 33], dtype=np.uint32)
    eng.prefill_batch([prompt] * rows)
    ids = np.full((rows, cfg.n_out), cfg.bos, dtype=np.uint32)
    eng.profile(True)
    lg = eng.step(ids, [3] * rows)
    st = eng.profile_get()
    eng.profile(False)
    assert st["attn_cross"]["launches"] == cfg.layers
    for v in range(6):
        same = lg[voice_of == v]
        assert all(np.array_equal(same[0], s) for s in same), v
    firsts = [lg[v] for v in range(6)]
    assert all(not np.array_equal(firsts[a], firsts[b]) for a in range(6) for b in range(a)), "six voices, six different rows"
    eng.close()


def test_a_bank_nobody_uses_changes_nothing(monkeypatch):
    """voice_bank + voice_set with every slot left at voice 0: step at 3 and 100 rows and generate_greedy are bit-equal to a context that never
    made a bank, and at 100 rows no ATTN_CROSS launch appears (the fold is still taken)"""
    monkeypatch.setenv("TTS_HIP_TILE_FORCE", "3")
    model = wide_model(gguf.F16)
    cfg = model.cfg
    enc = encodings(cfg.hidden, [12])[0]
    rng = np.random.default_rng(8)
    res = []
    for bank in (False, True):
        eng = hip.HipEngine(cfg, max_seqs=100, kv_positions=24)
        eng.load(model)
        if bank:
            eng.voice_bank(3)
            eng.voice_set(2, enc)
            eng.seq_voices([0, 1, 2], [0, 0, 0])
        got = []
        for rows in (3, 100):
            rng = np.random.default_rng(rows)
            prompts = [rng.integers(3, cfg.prompt_vocab, 2 + (i % 3)).astype(np.uint32) for i in range(rows)]
            eng.prefill_batch(prompts)
            ids = rng.integers(0, cfg.audio_vocab, (rows, cfg.n_out)).astype(np.uint32)
            got.append(eng.step(ids, [len(p) for p in prompts]))
            if rows == 100:
                eng.profile(True)
                eng.step(ids, [len(p) for p in prompts])
                st = eng.profile_get()
                eng.profile(False)
                assert st["attn_cross"]["launches"] == 0 and st["gemm_cross_q"]["launches"] == cfg.layers, st["attn_cross"]
                toks, done = eng.generate_greedy([len(p) for p in prompts], 6)
                got += [toks, done]
        res.append(got)
        eng.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ---- loops ---------------------------------------------------------------------------------------------------------------------------------
SAMPLED = dict(top_k=20, top_p=1.0, temperature=0.9, repetition_penalty=1.1)
LOOP_VOICES = [10, 27]      # positions of voices 1 and 2 (the model's own description: 6)


@pytest.fixture(scope="module")
def pins():
    with pytest.MonkeyPatch.context() as mp:
        for k, v in PINS.items():
            mp.setenv(k, v)
        yield


@pytest.fixture(scope="module")
def loop_world():
    cfg = synth.tiny(weight_type=gguf.F16)     # 2 layers: the second layer's self-attention sees the first one's cross-attention
    model = synth.build(cfg)
    encs = [None] + encodings(cfg.hidden, LOOP_VOICES, seed=77)
    return dict(cfg=cfg, model=model, encs=encs)


def _voice_engine(w, max_seqs, kv_positions, fold=None):
    eng = hip.HipEngine(w["cfg"], max_seqs=max_seqs, kv_positions=kv_positions, flags=hip.FLAG_NO_DAC, tune=None if fold is None else {"cross_fold": fold})
    eng.load(w["model"])
    return eng


def _with_bank(eng, w):
    eng.voice_bank(4)
    for v in (1, 2):
        eng.voice_set(v, w["encs"][v])
    return eng


def _own_engine(w, v, max_seqs, kv_positions):
    """the yardstick: a context whose own description is voice v, the cross-attention a launch of its own"""
    eng = _voice_engine(w, max_seqs, kv_positions, fold=0)
    if v:
        eng.set_text_encoding(w["encs"][v])
    return eng


@pytest.mark.parametrize("sampled", [False, True])
def test_generation_loops_with_a_voice_per_utterance(loop_world, sampled):
    """6 utterances with voices [0, 1, 2, 1, 0, 2]: each one's tokens and step count are those of the unfolded engine of its voice at the same n_seqs"""
    w = loop_world
    cfg = w["cfg"]
    voices = [0, 1, 2, 1, 0, 2]
    n, n_steps = len(voices), 24
    rng = np.random.default_rng(3)
    prompts = [rng.integers(3, cfg.prompt_vocab, 3 + i).astype(np.uint32) for i in range(n)]
    lens = [len(p) for p in prompts]
    uni = rng.random((n_steps, n, cfg.n_out), dtype=np.float32)

    def generate(eng):
        eng.prefill_batch(prompts)
        return eng.generate_sampled(lens, n_steps, uni, **SAMPLED) if sampled else eng.generate_greedy(lens, n_steps)

    eng = _with_bank(_voice_engine(w, n, 64), w)
    eng.seq_voices(range(n), voices)
    toks, done = generate(eng)
    toks2, done2 = generate(eng)     # the captured mixed steps replayed
    assert np.array_equal(toks, toks2) and np.array_equal(done, done2)
    eng.close()
    refs = {}
    for v in (0, 1, 2):
        one = _own_engine(w, v, n, 64)
        refs[v] = generate(one)
        one.close()
    for u, v in enumerate(voices):
        rt, rd = refs[v]
        assert done[u] == rd[u] and np.array_equal(toks[:, u], rt[:, u]), (u, v)
    assert not np.array_equal(refs[0][0], refs[1][0]) and not np.array_equal(refs[1][0], refs[2][0]), "the voices must matter"


N_UTT, SLOTS, CAP, REP = 8, 3, 48, 5
MAX_STEPS = CAP - 1
UTT_VOICE = [0, 0, 0, 1, 2, 1, 0, 2]            # the first occupants share the context's own description, the second ones bring another voice
UTT_SETTING = [None, SAMPLED, None, SAMPLED, SAMPLED, None, None, SAMPLED]


@pytest.fixture(scope="module")
def session_world(pins, loop_world):
    """per voice and setting the lock-step generation of the 8 utterances, five times over (40 rows: the tiled GEMMs a session's 64-row forwards
    take, as tests/test_gpu_parler_stream_mixed.py builds its yardstick): (tokens [step][utt][head], steps [utt])"""
    w = dict(loop_world)
    cfg = w["cfg"]
    rng = np.random.default_rng(19)
    lens = rng.integers(3, 12, N_UTT)
    prompts = [rng.integers(3, cfg.prompt_vocab, int(l)).astype(np.uint32) for l in lens]
    n_steps = int(CAP - lens.min())
    uni = rng.random((n_steps, N_UTT, cfg.n_out), dtype=np.float32)
    refs = {}
    for v in (0, 1, 2):
        for si, s in enumerate((None, SAMPLED)):
            one = _own_engine(w, v, N_UTT * REP, CAP)
            one.prefill_batch(prompts * REP)
            if s is None:
                rt, rd = one.generate_greedy(np.tile(lens, REP), n_steps)
            else:
                rt, rd = one.generate_sampled(np.tile(lens, REP), n_steps, np.tile(uni, (1, REP, 1)), **s)
            one.close()
            assert np.array_equal(rt[:, :N_UTT], rt[:, N_UTT:2 * N_UTT]), "rows do not mix"
            steps = np.where(rd > 0, rd, n_steps).astype(int)
            refs[(v, si)] = (rt[:, :N_UTT].copy(), steps[:N_UTT])
    w.update(lens=lens, prompts=prompts, n_steps=n_steps, uni=uni, refs=refs)
    return w


def _graphs(eng):
    return int(eng.debug_read("graphs", 1)[0])


def test_mixed_session_whose_slots_change_voice(session_world):
    """3 slots, 8 utterances that differ in voice and sampler, stream_run sizes cycled over 1 / 5 / 16; every slot gets a second occupant with
    another voice.  Tokens and step counts are those of the unfolded engine of the utterance's voice; after the first one-voice run and the first
    mixed run of each row count and sampler mode nothing is captured again."""
    w = session_world
    cfg = w["cfg"]
    eng = _with_bank(_voice_engine(w, SLOTS + 1, CAP), w)
    eng.stream_begin_mixed(SLOTS, MAX_STEPS)
    waiting, slot_utt, free, got = list(range(N_UTT)) + [0, 1], {}, list(range(SLOTS)), {}   # 0 and 1 once more at the end: one-voice runs after mixed ones
    again = {}
    occupants = {s: [] for s in range(SLOTS)}
    sizes, rounds = [1, 5, 16], 0
    seen_modes, modes_in_order, grew_without_new_mode = set(), [], []
    while waiting or slot_utt:
        take = waiting[:len(free)]
        if take:
            waiting = waiting[len(take):]
            sl = [free.pop(0) for _ in take]
            eng.seq_voices(sl, [UTT_VOICE[u] for u in take])            # before the admission: its prefill already attends
            settings = [UTT_SETTING[u] for u in take]
            u_in = np.zeros((len(take), MAX_STEPS, cfg.n_out), dtype=np.float32)
            for i, u in enumerate(take):
                u_in[i, :w["n_steps"]] = w["uni"][:, u]
            eng.stream_admit_mixed(sl, [w["prompts"][u] for u in take], settings, u_in if any(s is not None for s in settings) else None)
            for s, u in zip(sl, take):
                slot_utt[s] = u
                occupants[s].append(u)
        mode = (any(UTT_VOICE[u] for u in slot_utt.values()), any(UTT_SETTING[u] is not None for u in slot_utt.values()))
        before = _graphs(eng)
        for slot, steps in eng.stream_run(sizes[rounds % 3]):
            u = slot_utt.pop(slot)
            (again if u in got else got)[u] = (steps, eng.stream_collect(slot, steps))
            free.append(slot)
        after = _graphs(eng)
        if mode in seen_modes and after != before:
            grew_without_new_mode.append((rounds, mode, before, after))
        seen_modes.add(mode)
        modes_in_order.append(mode)
        rounds += 1
        assert rounds < 400
    assert not grew_without_new_mode, grew_without_new_mode
    assert any(m[0] for m in seen_modes) and any(not m[0] for m in seen_modes), "one-voice runs and mixed runs"
    assert modes_in_order[0][0] is False and modes_in_order[-1][0] is False and any(m[0] for m in modes_in_order), "one-voice, mixed, one-voice again"
    print("steps per utterance:", [got[u][0] for u in range(N_UTT)], "runs:", rounds, "graphs:", after)
    eng.stream_end()
    eng.close()
    for occ in occupants.values():
        assert len(occ) >= 2 and UTT_VOICE[occ[0]] != UTT_VOICE[occ[1]], occ
    assert sorted(again) == [0, 1]
    for u in again:
        assert again[u][0] == got[u][0] and np.array_equal(again[u][1], got[u][1]), u
    for u in range(N_UTT):
        rt, steps = w["refs"][(UTT_VOICE[u], 0 if UTT_SETTING[u] is None else 1)]
        assert got[u][0] == steps[u], (u, got[u][0], steps[u])
        assert np.array_equal(got[u][1], rt[:steps[u], u]), f"utterance {u} (voice {UTT_VOICE[u]}, {UTT_SETTING[u]})"


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_by_name_and_the_context_goes_on(loop_world):
    w = loop_world
    cfg = w["cfg"]
    H = cfg.hidden
    n, n_steps = 3, 12
    rng = np.random.default_rng(23)
    prompts = [rng.integers(3, cfg.prompt_vocab, 4 + i).astype(np.uint32) for i in range(n)]
    lens = [len(p) for p in prompts]
    voices = [1, 0, 2]
    refs = {}
    for v in (0, 1, 2):
        one = _own_engine(w, v, n, 64)
        one.prefill_batch(prompts)
        refs[v] = one.generate_greedy(lens, n_steps)
        one.close()
    eng = _voice_engine(w, n + 1, 64)

    def still_equal():
        eng.seq_voices(range(n), voices)
        eng.prefill_batch(prompts)
        toks, done = eng.generate_greedy(lens, n_steps)
        for u, v in enumerate(voices):
            assert done[u] == refs[v][1][u] and np.array_equal(toks[:, u], refs[v][0][:, u]), (u, v)

    with pytest.raises(hip.HipError, match="tts_hip_parler_seq_voices.*no voice bank"):
        eng.seq_voices([0], [1])
    eng.seq_voices([0, 1], [0, 0])                                     # all at the context's own description: nothing to hold
    for bad in (0, 257):
        with pytest.raises(hip.HipError, match="tts_hip_parler_voice_bank"):
            eng.voice_bank(bad)
    _with_bank(eng, w)
    with pytest.raises(hip.HipError, match="tts_hip_parler_voice_bank.*already"):
        eng.voice_bank(4)
    still_equal()
    big = encodings(H, [33])[0]
    with pytest.raises(hip.HipError, match="tts_hip_parler_voice_set.*33 tokens"):
        eng.voice_set(3, big)
    for bad in (0, 5):
        with pytest.raises(hip.HipError, match="tts_hip_parler_voice_set"):
            eng.voice_set(bad, w["encs"][1])
    with pytest.raises(hip.HipError, match="tts_hip_parler_seq_voices.*never set"):
        eng.seq_voices([0], [3])
    with pytest.raises(hip.HipError, match="tts_hip_parler_seq_voices.*beyond the bank"):
        eng.seq_voices([0], [5])
    with pytest.raises(hip.HipError, match="tts_hip_parler_seq_voices.*max_seqs"):
        eng.seq_voices([n + 1], [1])
    still_equal()
    # a session: slot 0 live with voice 1
    eng.stream_begin_mixed(n, 40)
    eng.seq_voices([0], [1])
    eng.stream_admit_mixed([0], [prompts[0]], [None], None)
    with pytest.raises(hip.HipError, match="tts_hip_parler_seq_voices.*live"):
        eng.seq_voices([0], [2])
    with pytest.raises(hip.HipError, match="tts_hip_parler_voice_set.*in use"):
        eng.voice_set(1, w["encs"][2])
    with pytest.raises(hip.HipError, match="tts_hip_parler_seq_voices.*pads"):
        eng.seq_voices([n], [1])
    eng.voice_set(3, w["encs"][2])                                     # a voice nobody uses may be set while the session runs
    eng.seq_voices([1], [3])                                           # ... and a free slot may take it
    fin = []
    while not fin:
        fin = eng.stream_run(16)
    eng.stream_end()
    # between a launch and its wait
    eng.seq_voices(range(n), voices)
    eng.prefill_batch(prompts)
    L = eng.L
    import ctypes as C
    start = np.asarray(lens, dtype=np.uint32)
    eng._chk(L.tts_hip_parler_gen_begin(eng.ctx, n, start.ctypes.data_as(C.POINTER(C.c_uint32)), n_steps, cfg.bos, cfg.eos, None, None))
    with pytest.raises(hip.HipError, match="tts_hip_parler_seq_voices.*live"):
        eng.seq_voices([0], [0])
    eng._chk(L.tts_hip_parler_gen_launch(eng.ctx, 4))
    with pytest.raises(hip.HipError, match="tts_hip_parler_voice_set.*in flight"):
        eng.voice_set(4, w["encs"][1])
    with pytest.raises(hip.HipError, match="tts_hip_parler_seq_voices.*in flight"):
        eng.seq_voices([n], [1])
    ran = C.c_uint32()
    eng._chk(L.tts_hip_parler_gen_wait(eng.ctx, None, None, C.byref(ran)))
    assert ran.value == 4
    eng.reset()
    still_equal()
    eng.close()

    # a context whose own description has 40 positions cannot take part in a mixed forward
    long_model = synth.build(synth.tiny(weight_type=gguf.F16, enc_len=40))
    e2 = hip.HipEngine(long_model.cfg, max_seqs=2, kv_positions=32, flags=hip.FLAG_NO_DAC)
    e2.load(long_model)
    e2.voice_bank(2)
    e2.voice_set(1, w["encs"][1])
    with pytest.raises(hip.HipError, match="tts_hip_parler_seq_voices.*40 positions"):
        e2.seq_voices([0], [1])
    e2.seq_voices([0], [0])
    p = np.array([5, 6, 7], dtype=np.uint32)
    e2.prefill_batch([p, p])
    ids = np.full((2, long_model.cfg.n_out), long_model.cfg.bos, dtype=np.uint32)
    a = e2.step(ids, [3, 3])
    e3 = hip.HipEngine(long_model.cfg, max_seqs=2, kv_positions=32, flags=hip.FLAG_NO_DAC)
    e3.load(long_model)
    e3.prefill_batch([p, p])
    assert np.array_equal(a, e3.step(ids, [3, 3]))
    e3.close()
    # ... and the other order: a slot with a voice, then a long description for the context
    e4 = hip.HipEngine(cfg, max_seqs=2, kv_positions=32, flags=hip.FLAG_NO_DAC)
    e4.load(w["model"])
    _with_bank(e4, w)
    e4.seq_voices([1], [1])
    with pytest.raises(hip.HipError, match="set_text_encoding.*non-zero voice"):
        e4.set_text_encoding(encodings(H, [40])[0])
    e4.close()
    e2.close()
