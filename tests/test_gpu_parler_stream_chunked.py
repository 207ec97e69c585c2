"""Chunked audio out of the Parler continuous session.
  engine   tts_hip_parler_stream_launch / _wait hand a live slot's token rows out in pieces that tile its history (they equal stream_collect and
           the same utterances in the same slots through stream_run / stream_collect, whatever the launch sizes), tts_hip_parler_stream_drop
           takes one slot out without touching the others, and everything that would touch the rows while steps are in flight is refused
  runner   generate_stream_chunked delivers every utterance's audio in pieces of at most chunk_frames frames that concatenate to generate()'s
           audio of that text, with the same tokens; on_chunk returning False drops that utterance only.  The runner's hook is an opt-in
           (TTS_PARLER_STREAM_CHUNKS=1); without it every utterance still arrives as one chunk
The GEMM tile shape is pinned as in tests/test_gpu_parler_stream_mixed.py: a session's forward is padded to 64 rows, a lone generate() is one row."""
import numpy as np
import pytest

from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

PINS = {"TTS_HIP_TILE_FORCE": "3", "TTS_HIP_TILE_KS": "1", "TTS_HIP_ATTN_NSPLIT": "1", "TTS_HIP_ATTN_ROWS": "0"}
CAP, SLOTS = 160, 3
MAX_STEPS = CAP - 1
LENS = [100, 30, 60, 120, 45, 90, 20, 75]          # prompt ids; random weights never end early: utterance u makes CAP - LENS[u] steps (40 ... 140)
QUEUES = [[0, 3, 6], [1, 4, 7], [2, 5]]            # slot -> its occupants in turn: both runs put an utterance into the same slot
# None: sampler::max.  The mixed session: per-slot top_k and repetition penalty, and one greedy slot
SETTINGS = [dict(top_k=20, top_p=1.0, temperature=0.9, repetition_penalty=1.1), None,
            dict(top_k=8, top_p=1.0, temperature=1.0, repetition_penalty=1.4)]
MARK = np.uint32(0xFFFFFFFF)
SIZES = (1, 5, 32, 37)


@pytest.fixture(scope="module")
def pins():
    with pytest.MonkeyPatch.context() as mp:
        for k, v in PINS.items():
            mp.setenv(k, v)
        yield


@pytest.fixture(scope="module")
def world(pins):
    cfg = synth.small(weight_type=gguf.F16, ctx=CAP, max_gen=CAP)
    model = synth.build(cfg)
    rng = np.random.default_rng(41)
    prompts = [rng.integers(3, cfg.prompt_vocab, l).astype(np.uint32) for l in LENS]
    uni = rng.random((len(LENS), MAX_STEPS, cfg.n_out), dtype=np.float32)
    w = dict(cfg=cfg, model=model, prompts=prompts, uni=uni)
    # the reference, once per kind: the same utterances in the same slots through stream_run(32) / stream_collect
    w["want"] = {kind: _serve_run(w, kind) for kind in ("greedy", "mixed")}
    for kind in ("greedy", "mixed"):
        assert [w["want"][kind][u][0] for u in range(len(LENS))] == [CAP - l for l in LENS], "every utterance ends at max_generation"
    assert not np.array_equal(w["want"]["greedy"][0][1], w["want"]["mixed"][0][1]), "the settings must matter"
    return w


def _engine(w):
    eng = hip.HipEngine(w["cfg"], max_seqs=SLOTS + 1, kv_positions=CAP, flags=hip.FLAG_NO_DAC)
    eng.load(w["model"])
    return eng


def _begin(eng, kind):
    if kind == "greedy":
        eng.stream_begin(SLOTS, MAX_STEPS, sampling=None)
    else:
        eng.stream_begin_mixed(SLOTS, MAX_STEPS)


def _admit(eng, w, kind, slots, us):
    if kind == "greedy":
        eng.stream_admit(slots, [w["prompts"][u] for u in us])
    else:
        eng.stream_admit_mixed(slots, [w["prompts"][u] for u in us], [SETTINGS[u % len(SETTINGS)] for u in us], w["uni"][us])


def _refill(eng, w, kind, queues, live):
    sl = [s for s in range(SLOTS) if s not in live and queues[s]]
    if sl:
        us = [queues[s].pop(0) for s in sl]
        _admit(eng, w, kind, sl, us)
        live.update(dict(zip(sl, us)))


def _serve_run(w, kind):
    """-> {utterance: (steps, tokens)} through stream_run(32) / stream_collect"""
    eng = _engine(w)
    _begin(eng, kind)
    queues, live, got, rounds = [list(q) for q in QUEUES], {}, {}, 0
    while live or any(queues):
        _refill(eng, w, kind, queues, live)
        for slot, steps in eng.stream_run(32):
            got[live.pop(slot)] = (steps, eng.stream_collect(slot, steps))
        rounds += 1
        assert rounds < 40
    eng.stream_end()
    eng.close()
    return got


class _Pieces:
    """the checks of one chunked session: the view stream_wait returns, marked where nothing has been handed out"""

    def __init__(self, eng):
        self.eng = eng
        self.out = eng._stream_out[0]
        self.out[:] = MARK
        self.have = np.zeros(SLOTS, dtype=int)      # rows handed out per slot
        self.live_pieces = 0                        # waits that handed rows of a live, unfinished slot out

    def wait(self, live, take=True):
        """live: the occupied slots.  A slot whose occupant has left reports that occupant's count until it is admitted again; nothing is written there."""
        before = self.out.copy()
        out, steps, done, fin = self.eng.stream_wait(take=take)
        assert out is self.out
        for s in range(SLOTS):
            if s not in live:
                assert (out[s] == MARK).all(), f"slot {s} has no occupant"
                continue
            assert np.array_equal(out[s, :self.have[s]], before[s, :self.have[s]]), "earlier rows are not rewritten"
            upto = int(steps[s]) if take else self.have[s]
            assert upto >= self.have[s]
            assert not (out[s, :upto] == MARK).any(), f"slot {s}: a marker below row {upto}"
            assert (out[s, upto:] == MARK).all(), f"slot {s}: a row above {upto} was written"
            if take and upto > self.have[s] and not done[s]:
                self.live_pieces += 1
            self.have[s] = upto
        return steps, done, fin

    def leave(self, slot):
        """the slot's occupant is gone: its rows start at 0 again"""
        self.out[slot] = MARK
        self.have[slot] = 0


@pytest.mark.parametrize("kind", ["greedy", "mixed"])
def test_pieces_tile_the_history_and_equal_run_and_collect(world, kind):
    w = world
    eng = _engine(w)
    _begin(eng, kind)
    p = _Pieces(eng)
    queues, live, got, waits = [list(q) for q in QUEUES], {}, {}, 0
    while live or any(queues):
        _refill(eng, w, kind, queues, live)
        eng.stream_launch(SIZES[waits % len(SIZES)])
        if waits == 6:                              # a look-in that takes nothing: the rows stay and arrive with the pure look-in after it
            steps0, done0, fin = p.wait(live, take=False)
            steps, done, fin2 = p.wait(live, take=True)
            assert fin2 == [] and np.array_equal(steps, steps0) and np.array_equal(done, done0)
            assert (steps > 0).any()
        else:
            steps, done, fin = p.wait(live)
        waits += 1
        for slot, n in fin:
            assert done[slot] and steps[slot] == n
            toks = p.out[slot, :n].copy()
            assert np.array_equal(toks, eng.stream_collect(slot, n)), "the pieces are what collect returns"
            got[live.pop(slot)] = (n, toks)
            p.leave(slot)
        assert waits < 400
    eng.stream_end()
    eng.close()
    assert waits > 6 and p.live_pieces > 0, "rows of a live, unfinished slot must have been handed out"
    assert len(got) == len(LENS)
    for u in range(len(LENS)):
        assert got[u][0] == w["want"][kind][u][0], u
        assert np.array_equal(got[u][1], w["want"][kind][u][1]), f"utterance {u}: launch / wait against run(32) / collect"


@pytest.mark.parametrize("kind", ["greedy", "mixed"])
def test_drop_and_ordering(world, kind):
    w = world
    want = w["want"][kind]
    eng = _engine(w)
    _begin(eng, kind)
    p = _Pieces(eng)
    queues, live, got = [list(q) for q in QUEUES], {}, {}
    _refill(eng, w, kind, queues, live)             # 0, 1, 2 into slots 0, 1, 2

    def look(fin, steps):
        for slot, n in fin:
            got[live.pop(slot)] = (n, p.out[slot, :n].copy())
            p.leave(slot)

    eng.stream_launch(32)
    # everything that would touch the rows is refused while the steps are in flight, before anything is launched
    with pytest.raises(hip.HipError, match="in flight"):
        _admit(eng, w, kind, [0], [3])
    with pytest.raises(hip.HipError, match="in flight"):
        eng.stream_collect(0, 4)
    with pytest.raises(hip.HipError, match="in flight"):
        eng.stream_drop([1])
    with pytest.raises(hip.HipError, match="in flight"):
        eng.stream_run(8)
    with pytest.raises(hip.HipError, match="in flight"):
        eng.stream_launch(8)
    steps, done, fin = p.wait(live)
    assert list(steps) == [32, 32, 32] and not done.any() and fin == []
    # 70 steps between two waits that take rows: more than the 64 the look-in's staging holds per slot, so the second wait goes round twice;
    # utterances 0 (60 steps) and 2 (100) end inside it and step on to its end
    eng.stream_launch(20)
    steps, done, fin = p.wait(live, take=False)
    assert list(steps) == [52, 52, 52] and fin == []
    eng.stream_launch(50)
    steps, done, fin = p.wait(live)
    assert sorted(fin) == [(0, 60), (2, 100)] and list(steps) == [60, 102, 100] and list(done) == [True, False, True]
    look(fin, steps)
    # slot 1 (utterance 1, 130 steps) leaves mid-utterance; its next occupant takes the slot at once
    with pytest.raises(hip.HipError, match="not live"):
        eng.stream_drop([1, 0])                     # slot 0 has finished: a free slot; slot 1 stays
    with pytest.raises(hip.HipError, match="twice"):
        eng.stream_drop([1, 1])
    with pytest.raises(hip.HipError, match=">= %d" % SLOTS):
        eng.stream_drop([1, SLOTS])
    eng.stream_drop([1])
    dropped = live.pop(1)
    p.leave(1)
    with pytest.raises(hip.HipError, match="not live"):
        eng.stream_drop([1])                        # dropped already
    rounds = 0
    while live or any(queues):
        _refill(eng, w, kind, queues, live)
        eng.stream_launch(32)
        steps, done, fin = p.wait(live)
        look(fin, steps)
        rounds += 1
        assert rounds < 40
    with pytest.raises(hip.HipError, match="not live"):
        eng.stream_drop([2])                        # nobody is live any more
    eng.stream_end()
    eng.close()
    assert dropped == 1 and sorted(got) == [0, 2, 3, 4, 5, 6, 7]
    for u in got:                                   # 4 and 7 are the dropped slot's later occupants
        assert got[u][0] == want[u][0] and np.array_equal(got[u][1], want[u][1]), f"utterance {u} beside / after the drop"


# ---- runner ---------------------------------------------------------------------------------------------------------------------------------
# The tiny fp32 model of tests/test_gpu_parler_voices_runner.py, where a session's utterance is bit for bit its own generate() call, with
# max_generation 160: a short prompt makes about 150 steps, five look-ins.
# The sampled configuration's seed: a session's forward has 64 rows and a generate() call one, other GEMM kernels and another fp32 summation
# order, and with some seeds a draw falls so close to a boundary of the sampler's cumulative sum that the two disagree from that step on.  That is
# the unchunked session's behaviour too (measured on these 8 texts: seed 5 with penalty 1.1 parts from generate() at step 7 of utterance 7, seed
# 11 in utterance 5; seeds 1234, 17 agree everywhere, with and without the pins), so the fixture checks that the unchunked session equals
# generate() here: what the tests below then compare is the chunking.
N_TEXTS = 8
CONFIGS = [dict(sample=0),
           dict(sample=1, seed=1234, top_k=20, temperature=0.9, repetition_penalty=1.1)]
WORDS = (2, 14, 5, 9, 1, 18, 7, 3)


@pytest.fixture(scope="module")
def opt_in():
    """the runner's chunk hook is an opt-in, read when the hook is asked for"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TTS_PARLER_STREAM_CHUNKS", "1")
        yield


@pytest.fixture(scope="module")
def served(pins, opt_in, tmp_path_factory):
    """the GGUFs, 8 texts of ragged length (more than the 3 slots), and per configuration a generate() call per text: (audio, still-delayed tokens)"""
    from tts_cpp_amd import runner
    d = tmp_path_factory.mktemp("parler_stream_chunked")
    cfg = synth.tiny(weight_type=gguf.F32, ctx=256, max_gen=CAP)
    path = synth.build(cfg).write_gguf(str(d / "tiny.gguf"))
    t5_path = synth.build_t5(synth.t5_tiny(vocab=cfg.prompt_vocab, output_size=cfg.hidden)).write_gguf(str(d / "t5.gguf"))
    rng = np.random.default_rng(5)
    texts = [" ".join("w%d" % rng.integers(0, 50) for _ in range(n)) for n in WORDS]
    one = runner.Runner(path, sample=0)
    singles = []
    for kw in CONFIGS:
        singles.append([])
        for t in texts:
            audio = one.generate(t, **kw)
            singles[-1].append((audio, one.last_tokens(1).copy()))
    one.close()
    many = runner.Runner(path, sample=0, max_seqs=SLOTS + 1)
    for kw, want in zip(CONFIGS, singles):
        whole = many.generate_stream(texts, **kw)
        assert all(np.array_equal(a, b) for a, (b, _) in zip(whole, want)), ("the unchunked session must equal generate() for these texts", kw)
    many.close()
    frames = [a.size // cfg.hop for a, _ in singles[0]]
    print("frames per utterance:", frames)
    assert len(set(frames)) > 3 and max(frames) >= 96, frames
    return dict(path=path, t5_path=t5_path, texts=texts, singles=singles, hop=cfg.hop, n_out=cfg.n_out)


def _per_utterance(got, n):
    return [[a for u, a, _ in got if u == i] for i in range(n)]


def _check(many, got, want, cf, hop, tag):
    """sizes, concatenation and tokens of every utterance against its generate() call; the bar of tests/test_gpu_chunked.py: equal, or within 1e-6"""
    per = _per_utterance(got, len(want))
    worst = 0.0
    for i, (audio, toks) in enumerate(want):
        assert all(0 < c.size <= cf * hop and c.size % hop == 0 for c in per[i]), (tag, i)
        cat = np.concatenate(per[i]) if per[i] else np.zeros(0, dtype=np.float32)
        assert toks.size > 0 and np.array_equal(many.last_tokens(16 + i), toks), (tag, i)
        assert cat.shape == audio.shape, (tag, i, cat.shape, audio.shape)
        if cat.size:
            worst = max(worst, float(np.abs(cat - audio).max()))
    print(f"{tag}: max |chunked session - generate()| = {worst:.3e}")
    assert worst <= 1e-6, (tag, worst)
    return per


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cf", [1, 8, 32, 40])
def test_runner_chunks_equal_generate(served, cf, mode):
    """chunk_frames below, at and above the look-in of 32; 8 plus the halo of 10 crosses a look-in.  8 utterances through 3 slots."""
    from tts_cpp_amd import runner
    s = served
    want = s["singles"][mode]
    many = runner.Runner(s["path"], sample=0, max_seqs=SLOTS + 1)
    # the call's record of an utterance's tokens is written when the utterance has ended: what it holds when a chunk arrives tells whether
    # audio left before the end
    record_at_first_chunk = {}

    def on_chunk(u, a, t):
        record_at_first_chunk.setdefault(u, many.last_tokens(16 + u).size)

    got = many.generate_stream_chunked(s["texts"], chunk_frames=cf, on_chunk=on_chunk, **CONFIGS[mode])
    assert many.stopped is False
    _check(many, got, want, cf, s["hop"], f"mode {mode} / {cf}")
    long = [i for i, (audio, _) in enumerate(want) if audio.size // s["hop"] >= 96]
    assert long
    for i in long:
        assert record_at_first_chunk[i] == 0, f"utterance {i}: its first chunk came only after it had ended"
    many.close()


def test_runner_cancel_drops_one_utterance_only(served):
    from tts_cpp_amd import runner
    s = served
    want = s["singles"][0]
    many = runner.Runner(s["path"], sample=0, max_seqs=SLOTS + 1)
    got = many.generate_stream_chunked(s["texts"], chunk_frames=8, sample=0, on_chunk=lambda u, a, t: u != 1)
    assert many.stopped is True                                                        # tts_c_generate_stream_chunked returned 1
    per = _per_utterance(got, N_TEXTS)
    assert len(per[1]) == 1 and per[1][0].size == 8 * s["hop"]
    assert np.abs(per[1][0] - want[1][0][:8 * s["hop"]]).max() <= 1e-6
    short = many.last_tokens(16 + 1)
    assert 0 < short.size < want[1][1].size and np.array_equal(short, want[1][1][:short.size])
    for i in range(N_TEXTS):
        if i == 1:
            continue
        cat = np.concatenate(per[i])
        assert cat.shape == want[i][0].shape and np.abs(cat - want[i][0]).max() <= 1e-6, i
        assert np.array_equal(many.last_tokens(16 + i), want[i][1]), i
    with pytest.raises(runner.RunnerError, match="chunk_frames"):
        many.generate_stream_chunked(s["texts"], chunk_frames=0, sample=0)
    assert np.array_equal(many.generate(s["texts"][1], sample=0), want[1][0])          # the runner generates as before
    with pytest.MonkeyPatch.context() as mp:                                          # without the switch: every utterance as one chunk, as before
        mp.delenv("TTS_PARLER_STREAM_CHUNKS")
        whole = many.generate_stream_chunked(s["texts"], chunk_frames=8, sample=0)
    assert sorted(u for u, _, _ in whole) == list(range(N_TEXTS))
    assert all(np.array_equal(a, want[u][0]) for u, a, _ in whole)
    many.close()


def test_runner_per_text_configs_and_a_bank_voice(served):
    """the mixed session under the hook: greedy and sampled texts in turn, one of them with a voice of the bank; the audio of
    generate_stream(texts, configs=...) and the tokens of each text's own generate() call"""
    from tts_cpp_amd import runner
    s = served
    many = runner.Runner(s["path"], sample=0, max_seqs=SLOTS + 1)
    many.add_voice("a", s["t5_path"], "calm low")
    configs = [dict(CONFIGS[i % 2]) for i in range(N_TEXTS)]
    configs[1]["voice"] = "a"
    configs[4]["voice"] = "a"
    want = many.generate_stream(s["texts"], configs=configs)
    got = many.generate_stream_chunked(s["texts"], chunk_frames=8, configs=configs)
    assert many.stopped is False
    per = _per_utterance(got, N_TEXTS)
    toks = [many.last_tokens(16 + i).copy() for i in range(N_TEXTS)]
    for i in range(N_TEXTS):
        assert all(0 < c.size <= 8 * s["hop"] for c in per[i]), i
        cat = np.concatenate(per[i]) if per[i] else np.zeros(0, dtype=np.float32)
        assert cat.shape == want[i].shape and want[i].size > 0, i
        assert np.array_equal(cat, want[i]) or np.abs(cat - want[i]).max() <= 1e-6, i
        many.generate(s["texts"][i], **configs[i])
        assert toks[i].size > 0 and np.array_equal(toks[i], many.last_tokens(1)), (i, configs[i])
    assert not np.array_equal(toks[1], s["singles"][1][1][1]), "the voice must matter"
    many.close()
