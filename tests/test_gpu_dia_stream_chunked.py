"""Chunked audio out of the Dia continuous session.  Device: tts_hip_dia_stream_launch / _wait hand a live slot's history rows out in pieces
that tile what tts_hip_dia_stream_collect returns and what a session driven by tts_hip_dia_stream_run returns (exact: the same forward at the
same row count), tts_hip_dia_stream_drop parks one slot without touching the others.  Runner: generate_stream_chunked delivers every
utterance's audio in chunks while the slots keep running; concatenated it is generate()'s audio within the 1e-5 of test_gpu_dia_stream.py (the
codec sees windows of several utterances in one pass), with identical ids."""
import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

MAX_GEN = 160
MARK = 0xFFFFFFFF
# the six texts and budgets of test_gpu_dia_stream.py, and two long budgets whose rows are taken many times; in this order every slot of a
# two- or three-slot session gets a second occupant
TEXTS = ["[S1] first one.", "[S2] the second is long.", "[S1] hi.", "[S1] a [S2] b [S1] c.", "[S1] somebody else.", "[S2] number five.", "[S1] and a sixth.",
         "[S2] the last, long."]
EXTRA = (2, 9, 5, 18, 90, 6, 11, 115)   # budgets max_delay + these
SIZES = (1, 5, 16, 37)                  # launch sizes, cycled
SAMPLING = dict(top_k=8, repetition_penalty=1.3)
FILLER = "[S1] somebody else."


def _args(cfg):
    return dict(delay_pattern=[0, 8, 9, 10, 11, 12, 13, 14, 15], bos=cfg.bos, eos=cfg.eos, pad=cfg.pad, max_delay=cfg.max_delay)


def _engine(model, n):
    eng = hip.DiaEngine(model.cfg, max_utterances=n)
    eng.load(model)
    return eng


def _admit(eng, take, utts, budgets, uniforms):
    """take: [(slot, utterance)]"""
    eng.stream_admit([s for s, _ in take], [utts[u][0] for _, u in take], [utts[u][1] for _, u in take], budgets=[budgets[u] for _, u in take],
                     uniforms=None if uniforms is None else np.stack([uniforms[u] for _, u in take]))


def _pieces_session(eng, n_slots, utts, budgets, uniforms=None, **sampling):
    """the utterances through one session on launch / wait, rows taken at every wait but one -> (ids per utterance, the utterances each slot
    held in order, waits that handed rows of a live slot out)"""
    cfg = eng.cfg
    eng.stream_begin(n_slots, cfg.max_gen, sampled=uniforms is not None, **sampling, **_args(cfg))
    out, queue, in_slot = [None] * len(utts), [[] for _ in range(n_slots)], {}
    free, nxt, waits, partial = list(range(n_slots)), 0, 0, 0
    snap = np.full((n_slots, cfg.max_gen, cfg.n_out), MARK, dtype=np.uint32)
    have = [0] * n_slots                     # rows of the slot's occupant handed out so far

    def admit():
        nonlocal nxt
        take = []
        while free and nxt < len(utts):
            take.append((free.pop(0), nxt))
            nxt += 1
        if take:
            _admit(eng, take, utts, budgets, uniforms)
            for s, u in take:
                in_slot[s] = u
                queue[s].append(u)
                eng._stream_out[0][s] = MARK     # a new occupant: its rows start at 0 again
                snap[s] = MARK
                have[s] = 0

    admit()
    for _ in range(400):
        if not in_slot:
            break
        eng.stream_launch(SIZES[waits % len(SIZES)])
        waits += 1
        if waits == 3:                       # a look-in that takes nothing: the rows stay and arrive with the next wait
            buf, steps0, _, fin = eng.stream_wait(take=False)
            assert np.array_equal(buf, snap)
            assert any(steps0[s] > have[s] for s in in_slot)
            buf, steps, done, fin2 = eng.stream_wait()           # nothing launched: a pure look-in
            assert np.array_equal(steps, steps0) and fin2 == []
        else:
            buf, steps, done, fin = eng.stream_wait()
        for s in in_slot:
            n = int(steps[s])
            assert n >= have[s] and not (buf[s, :n] == MARK).any(), (s, n)          # no marker below steps_done
            assert (buf[s, n:] == MARK).all(), (s, n)                                # only marker above it
            assert np.array_equal(buf[s, :have[s]], snap[s, :have[s]]), (s, n)       # earlier rows not rewritten
            partial += 0 < have[s] < n and not done[s]
            have[s] = n
        snap = buf.copy()
        for s, n in fin:
            assert done[s] and n == steps[s] == have[s]
            out[in_slot.pop(s)] = buf[s, :n].copy()
            assert np.array_equal(out[queue[s][-1]], eng.stream_collect(s, n))       # collect keeps working after waits that took rows
            free.append(s)
        free.sort()
        admit()
    assert not in_slot and nxt == len(utts)
    eng.stream_end()
    return out, queue, partial


def _run_session(eng, n_slots, utts, budgets, queue, uniforms=None, **sampling):
    """the same utterances in the same slots through stream_run(4) / stream_collect"""
    cfg = eng.cfg
    eng.stream_begin(n_slots, cfg.max_gen, sampled=uniforms is not None, **sampling, **_args(cfg))
    out, todo, in_slot = [None] * len(utts), [list(q) for q in queue], {}

    def admit():
        take = [(s, todo[s].pop(0)) for s in range(n_slots) if s not in in_slot and todo[s]]
        if take:
            _admit(eng, take, utts, budgets, uniforms)
            in_slot.update(take)

    admit()
    for _ in range(400):
        if not in_slot:
            break
        for s, steps in eng.stream_run(4):
            out[in_slot.pop(s)] = eng.stream_collect(s, steps)
        admit()
    assert not in_slot and not any(todo)
    eng.stream_end()
    return out


@pytest.mark.parametrize("wtype", [gguf.F32, gguf.F16])
@pytest.mark.parametrize("n_slots", [2, 3])
def test_rows_in_pieces_equal_the_session(n_slots, wtype):
    model = synth.build_dia(synth.dia_tiny(max_gen=MAX_GEN, weight_type=wtype), suppress_special=True)
    cfg = model.cfg
    utts = [orc.dia_tokenize(t, cfg.max_ctx) for t in TEXTS]
    budgets = [cfg.max_delay + e for e in EXTRA]
    assert all(cfg.max_delay < b <= cfg.max_gen for b in budgets) and sum(b >= 100 for b in budgets) == 2
    uni = np.random.default_rng(5).random((len(utts), cfg.max_gen, cfg.n_out), dtype=np.float32)
    eng = _engine(model, n_slots)
    for kw in (dict(), dict(uniforms=uni, **SAMPLING)):
        got, queue, partial = _pieces_session(eng, n_slots, utts, budgets, **kw)
        assert all(len(q) >= 2 for q in queue), queue                       # every slot is reused at least once
        assert partial >= 8                                                  # rows of running utterances were handed out, many times
        other = _engine(model, n_slots)                                      # a fresh context, driven by stream_run
        want = _run_session(other, n_slots, utts, budgets, queue, **kw)
        other.close()
        for u in range(len(utts)):
            assert len(got[u]) == budgets[u] - 1                             # no EOS in this model
            assert got[u].shape == want[u].shape and np.array_equal(got[u], want[u]), (u, kw.keys())
    eng.close()


def _reference(model, n_slots, slot, utt, budget, filler):
    """tts_hip_dia_generate on a fresh context with n_utt = n_slots: the utterance in `slot`, any encoded sentence in the others"""
    eng = _engine(model, n_slots)
    for s in range(n_slots):
        eng.encode_slot(s, *(utt if s == slot else filler))
    out = eng.generate(n_slots, budget, **_args(model.cfg))[slot]
    eng.close()
    return out


def test_drop_parks_one_slot_and_leaves_the_others():
    model = synth.build_dia(synth.dia_tiny(max_gen=MAX_GEN), suppress_special=True)
    cfg = model.cfg
    utts = [orc.dia_tokenize(t, cfg.max_ctx) for t in TEXTS[:4]]
    filler = orc.dia_tokenize(FILLER, cfg.max_ctx)
    budgets = [70, 60, 80, 40]

    def session(drop):
        eng = _engine(model, 3)
        eng.stream_begin(3, cfg.max_gen, **_args(cfg))
        _admit(eng, [(0, 0), (1, 1), (2, 2)], utts, budgets, None)
        out, reported, new = {}, [], None
        for i in range(40):
            eng.stream_launch(5)
            buf, steps, done, fin = eng.stream_wait()
            reported += fin
            for s, n in fin:
                out[s] = out.get(s, []) + [buf[s, :n].copy()]
            if drop and i == 1:                                   # after 2 waits
                assert not done[1] and steps[1] == 10
                eng.stream_drop([1])
                _, steps2, done2, fin2 = eng.stream_wait()        # a pure look-in: parked with its step count, not reported
                assert done2[1] and steps2[1] == 10 and fin2 == [] and not done2[0] and not done2[2]
            if drop and i == 3:                                   # the dropped slot is free: a new occupant beside the two live ones
                assert not done[0] and not done[2]
                _admit(eng, [(1, 3)], utts, budgets, None)
                eng._stream_out[0][1] = MARK
            if len(reported) == 3:
                break
        eng.stream_end()
        eng.close()
        return out, reported

    kept, rep_kept = session(False)
    got, rep = session(True)
    assert sorted(rep_kept) == [(0, 69), (1, 59), (2, 79)]
    assert sorted(rep) == [(0, 69), (1, 39), (2, 79)]             # slot 1 is reported once, for its second occupant
    for s in (0, 2):
        assert len(got[s]) == 1 and np.array_equal(got[s][0], kept[s][0]), s
    assert len(got[1]) == 1 and np.array_equal(got[1][0], _reference(model, 3, 1, utts[3], 40, filler))


def test_misuse_is_refused_and_the_session_goes_on():
    model = synth.build_dia(synth.dia_tiny(max_gen=MAX_GEN), suppress_special=True)
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
        eng.stream_launch(1)
    eng.stream_begin(3, cfg.max_gen, **a)
    _admit(eng, [(0, 0), (1, 1)], utts, [40, 40, 40], None)
    eng.stream_launch(4)
    for call in (lambda: _admit(eng, [(2, 2)], utts, [40, 40, 40], None), lambda: eng.stream_collect(0, 1), lambda: eng.stream_drop([0]),
                 lambda: eng.stream_launch(1), lambda: eng.stream_run(1)):
        with pytest.raises(hip.HipError, match="in flight"):
            call()
    buf, steps, done, fin = eng.stream_wait()
    assert list(steps[:2]) == [4, 4] and fin == [] and not (buf[:2, :4] == MARK).any()
    with pytest.raises(hip.HipError, match="not live"):
        eng.stream_drop([2])                                          # parked since begin
    with pytest.raises(hip.HipError, match="n_slots"):
        eng.stream_drop([3])
    with pytest.raises(hip.HipError, match="twice"):
        eng.stream_drop([0, 0])
    eng.stream_launch(4)                                              # the refused calls left the session as it was
    buf, steps, done, fin = eng.stream_wait()
    assert list(steps[:2]) == [8, 8] and not done[0] and not (buf[:2, :8] == MARK).any()
    eng.stream_drop([0])
    with pytest.raises(hip.HipError, match="not live"):
        eng.stream_drop([0])                                          # parked by the drop
    eng.stream_launch(3)
    eng.stream_end()                                                  # waits for the steps in flight and drops them
    for s in range(3):                                                # after the session a plain generate equals a fresh context's
        eng.encode_slot(s, *utts[s])
    after = eng.generate(3, 24, **a)
    assert all(np.array_equal(x, y) for x, y in zip(after, want))
    eng.close()


# ---- runner and C ABI -----------------------------------------------------------------------------------------------------------------------
RTEXTS = [" Hi there [S2] ok", "[S1] another one.", "[S2] short", "[S1] the fourth one.", "[S2] five [S1] and six", "[S1] last."]
FIXED = dict(sample=0, max_tokens=120)                                # suppress_special: every utterance makes 119 steps, 104 kept frames
RAGGED = dict(sample=1, top_k=8, seed=5, max_tokens=36)               # the session test's configuration: dropped frames, EOS endings


@pytest.fixture(scope="module")
def ggufs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dia_stream_chunked")
    return {sup: synth.build_dia(synth.dia_tiny(max_gen=MAX_GEN), suppress_special=sup).write_gguf(str(d / f"dia{int(sup)}.gguf")) for sup in (True, False)}


@pytest.fixture(scope="module")
def singles(ggufs):
    """per model: (audio, still-delayed ids) of a generate() call per text"""
    from tts_cpp_amd import runner
    out = {}
    for sup, kw in ((True, FIXED), (False, RAGGED)):
        one = runner.Runner(ggufs[sup], sample=0)
        out[sup] = []
        for t in RTEXTS:
            audio = one.generate(t, **kw)
            out[sup].append((audio, one.last_tokens(1).copy()))
        one.close()
    return out


def _check_against_singles(many, got, want, chunk, tag):
    """got [(utterance, pcm, t)] -> chunks per utterance; sizes, concatenation and ids against the single calls"""
    per = [[a for u, a, _ in got if u == i] for i in range(len(want))]
    worst, equal = 0.0, True
    for i, (audio, toks) in enumerate(want):
        assert all(c.size == chunk for c in per[i][:-1]), (tag, i)                     # every chunk but the last is exactly chunk_frames * hop
        assert all(0 < c.size <= chunk for c in per[i][-1:]), (tag, i)
        cat = np.concatenate(per[i]) if per[i] else np.zeros(0, dtype=np.float32)
        assert cat.shape == audio.shape, (tag, i, cat.shape, audio.shape)
        if cat.size:
            worst = max(worst, float(np.abs(cat - audio).max()))
            equal = equal and np.array_equal(cat, audio)
        assert np.array_equal(many.last_tokens(16 + i), toks) and toks.size > 0, (tag, i)
    print(f"{tag}: max |chunked session - generate()| = {worst:.3e}, bit-equal: {equal}")
    assert worst < 1e-5, (tag, worst)
    return per


@pytest.mark.parametrize("chunk_frames", [8, 10000])
def test_runner_fixed_lengths(ggufs, singles, chunk_frames):
    from tts_cpp_amd import runner
    want = singles[True]
    hop = synth.dia_tiny().hop
    assert all(a.size > 100 * hop for a, _ in want)
    many = runner.Runner(ggufs[True], sample=0, max_seqs=3)
    got = many.generate_stream_chunked(RTEXTS, chunk_frames=chunk_frames, **FIXED)
    assert many.stopped is False
    per = _check_against_singles(many, got, want, chunk_frames * hop, f"fixed/{chunk_frames}")
    order = [u for u, _, _ in got]
    if chunk_frames == 8:
        assert all(len(p) >= 3 for p in per)
        for group in ((0, 1, 2), (3, 4, 5)):                                           # admitted together: nobody's first chunk waits for another's last
            first = {u: order.index(u) for u in group}
            last = {u: len(order) - 1 - order[::-1].index(u) for u in group}
            assert all(first[u] < last[v] for u in group for v in group), (first, last)
    else:
        assert all(len(p) == 1 for p in per)
    many.close()


def test_runner_dropped_frames_and_eos(ggufs, singles):
    from tts_cpp_amd import runner
    want = singles[False]
    hop = synth.dia_tiny().hop
    many = runner.Runner(ggufs[False], sample=0, max_seqs=3)
    got = many.generate_stream_chunked(RTEXTS, chunk_frames=8, **RAGGED)
    _check_against_singles(many, got, want, 8 * hop, "ragged/8")
    assert sum(a.size > 0 for a, _ in want) >= 3
    many.close()


def test_runner_cancel_drops_one_utterance_only(ggufs, singles):
    from tts_cpp_amd import runner
    want = singles[True]
    hop = synth.dia_tiny().hop
    many = runner.Runner(ggufs[True], sample=0, max_seqs=3)
    got = many.generate_stream_chunked(RTEXTS, chunk_frames=8, on_chunk=lambda u, a, t: u != 1, **FIXED)
    assert many.stopped is True                                                        # tts_c_generate_stream_chunked returned 1
    per = [[a for u, a, _ in got if u == i] for i in range(len(RTEXTS))]
    assert len(per[1]) == 1 and per[1][0].size == 8 * hop
    assert np.abs(per[1][0] - want[1][0][:8 * hop]).max() < 1e-5
    for i in (0, 2, 3, 4, 5):
        cat = np.concatenate(per[i])
        assert cat.shape == want[i][0].shape and np.abs(cat - want[i][0]).max() < 1e-5, i
    assert np.array_equal(many.generate(RTEXTS[1], **FIXED), want[1][0])               # the runner generates as before
    many.close()


def test_sessions_that_do_not_chunk_hand_out_whole_utterances(tmp_path):
    from tts_cpp_amd import runner
    path = synth.build(synth.tiny()).write_gguf(str(tmp_path / "parler.gguf"))
    texts = ["the quick brown fox", "hello there", "one two three", "and a fourth"]
    r = runner.Runner(path, sample=0, max_seqs=3, max_tokens=24)
    want = r.generate_stream(texts, sample=0, max_tokens=24)
    got = r.generate_stream_chunked(texts, chunk_frames=4, sample=0, max_tokens=24)
    assert sorted(u for u, _, _ in got) == [i for i, w in enumerate(want) if w.size] and len(got) >= 3
    for u, a, _ in got:
        assert np.array_equal(a, want[u]), u
    with pytest.raises(runner.RunnerError, match="chunk_frames"):
        r.generate_stream_chunked(texts, chunk_frames=0, sample=0, max_tokens=24)
    r.close()
