"""GPU: chunked audio out of the Orpheus continuous session.  The device calls (tts_hip_orpheus_stream_launch / _wait / _drop) against the
session that only runs (stream_run / stream_collect) and against each utterance's own one-sequence generation, and the runner's
generate_stream_chunked against generate()."""
import functools
import os
import time

import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import gguf, hip, runner, synth

pytestmark = pytest.mark.gpu

MAX_NEW = 45
NEVER = 5                # stop id = vocab + NEVER: a token nobody selects
SMP = dict(top_k=12, temperature=0.9, repetition_penalty=1.2)
SIZES = ([1], [5], [28], [37], [1, 5, 28, 37])
HOLE = 0xFFFFFFFF        # no id: what the test writes where a wait must write nothing
# A lock-step step of 5 or more rows goes through other kernels than the one-row step: their matrix products take fp16 inputs (2^-11 relative,
# on logits within +-4: 2^-9 absolute; measured on orpheus_tiny: up to 9.5e-4), so two logits can move against each other by 2^-8.  The tiny
# model's 200 logits lie close together, and a sampled id whose logit is within that distance of a neighbour's is another id at 7 rows (measured:
# candidates 5.6e-5 and 2.7e-4 apart swapped places under the draw).  The sampled reference therefore keeps only draws whose selection is steady:
# the same id when the selected logit moves by +-LOGIT_MARGIN against all others and the draw by +-DRAW_MARGIN (a shift of 2^-7 in a logit moves
# a candidate's share of the CDF by less than 2^-7 / temperature of itself).  A draw that is not steady is drawn again.  Decided on the eager
# one-sequence engine alone, with twice the headroom the format asks for.  With Q4_0 matrices both paths multiply Q8_0 activation blocks and differ
# by an ulp of the sums (measured 2.4e-7), which can flip a Q8_0 code of the next row: the same margin covers it.
LOGIT_MARGIN = np.float32(2.0 ** -7)
DRAW_MARGIN = np.float32(2.0 ** -6)
BELOW_ONE = np.float32(1.0) - np.float32(2.0 ** -24)


def _eager_engine(cfg, **kw):
    os.environ["TTS_HIP_LLAMA_GRAPH"] = "0"
    try:
        return hip.OrpheusEngine(cfg, **kw)
    finally:
        del os.environ["TTS_HIP_LLAMA_GRAPH"]


def _steady_sampled(single, prompt, u, rng):
    """the one-sequence sampled generation step by step (logits back, the device sampler on them, its repetition state carried), every draw
    redrawn until its selection is steady (above); u is updated in place -> ids"""
    lg, _ = single.decode(prompt, 0)
    pos, last, count, ids = len(prompt), -1, 0, []
    for k in range(MAX_NEW):
        for _ in range(200):
            tok, last2, count2 = single.sample_logits(lg, float(u[k]), last_id=last, rep_count=count, **SMP)
            steady = True
            for dl in (LOGIT_MARGIN, -LOGIT_MARGIN):
                for du in (DRAW_MARGIN, -DRAW_MARGIN):
                    moved = lg.copy()
                    moved[tok] += dl
                    steady = steady and single.sample_logits(moved, float(np.clip(u[k] + du, 0.0, BELOW_ONE)), last_id=last, rep_count=count, **SMP)[0] == tok
            if steady:
                break
            u[k] = rng.random(dtype=np.float32)
        assert steady, "no steady draw found"
        ids.append(int(tok))
        last, count = last2, count2
        if k + 1 < MAX_NEW:
            lg, _ = single.decode([tok], pos)
            pos += 1
    return ids


@functools.lru_cache(maxsize=None)
def _reference(n_slots, wtype):
    """2 n_slots + 1 prompts of ragged lengths, per-utterance uniforms, and per mode the ids of each utterance's own one-sequence generation on
    the eager engine.  The stop id is ref[20] of utterance 0's greedy run, so rows end inside a launch.  Computed once, shared, never changed."""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=wtype))
    cfg = model.cfg
    n_utt = 2 * n_slots + 1
    rng = np.random.default_rng(100 * n_slots + wtype)
    prompts = [rng.integers(0, cfg.vocab, 3 + 2 * (u % 4)).astype(np.uint32) for u in range(n_utt)]
    uni = rng.random((n_utt, MAX_NEW), dtype=np.float32)
    never = cfg.vocab + NEVER
    single = _eager_engine(cfg)
    single.load(model)
    greedy = [single.generate_greedy(p, MAX_NEW, stop_id=never).tolist() for p in prompts]
    stop = int(greedy[0][20])
    stopped = [single.generate_greedy(p, MAX_NEW, stop_id=stop).tolist() for p in prompts]
    steady = [_steady_sampled(single, p, uni[u], rng) for u, p in enumerate(prompts)]
    sampled = [single.generate_sampled(p, MAX_NEW, stop_id=never, uniforms=uni[u], **SMP).tolist() for u, p in enumerate(prompts)]
    assert sampled == steady, "the one-sequence loop and its step-by-step restatement disagree"
    single.close()
    mixed = [sampled[u] if u % 2 else greedy[u] for u in range(n_utt)]       # greedy and sampled slots side by side
    assert 0 < len(stopped[0]) <= 21 and len({len(r) for r in stopped}) > 1
    return model, prompts, uni, dict(greedy=(never, greedy), stopped=(stop, stopped), sampled=(never, sampled), mixed=(never, mixed))


def _begin(eng, mode, n_slots, stop):
    if mode == "mixed":
        eng.stream_begin_mixed(n_slots, MAX_NEW, stop)
    else:
        eng.stream_begin(n_slots, MAX_NEW, stop, sampled=mode == "sampled", **(SMP if mode == "sampled" else {}))


def _admit(eng, mode, slot, u, prompts, uni):
    if mode == "mixed":
        eng.stream_admit_mixed([slot], [prompts[u]], [SMP if u % 2 else None], uni[u:u + 1])
    else:
        eng.stream_admit([slot], [prompts[u]], uni[u:u + 1] if mode == "sampled" else None)


def _launch_session(eng, mode, prompts, uni, n_slots, stop, sizes, drop_utt=None, look_every=0):
    """Every prompt through one session on launch / wait, freed slots refilled between a wait and the next launch.  Before each taking wait the
    engine's token view holds HOLE everywhere: the wait must write exactly [ids handed so far, count) of every occupant and nothing else.
    look_every: every that many launches a wait with take=False comes first.  drop_utt: that utterance is dropped after its first wait.
    -> (ids per utterance as the waits tiled them, ids per utterance as stream_collect returns them, the utterances reported)"""
    _begin(eng, mode, n_slots, stop)
    free, slot_utt = list(range(n_slots)), {}
    view = np.full((n_slots, MAX_NEW), HOLE, dtype=np.uint32)          # the buffer the waits write into
    tiled, collected, reported = [[] for _ in prompts], [None] * len(prompts), []
    nxt, i = 0, 0
    while nxt < len(prompts) or slot_utt:
        while nxt < len(prompts) and free:
            s = free.pop(0)
            _admit(eng, mode, s, nxt, prompts, uni)
            slot_utt[s] = nxt
            nxt += 1
        eng.stream_launch(sizes[i % len(sizes)])
        i += 1
        fin, looked = [], look_every and i % look_every == 0
        if looked:
            _, cnt0, _, fin = eng.stream_wait(take=False, out=view)      # headers only: nothing is written, nothing is marked handed out
            assert (view == HOLE).all()
        out, cnt, done, fin2 = eng.stream_wait(out=view)                 # (the view holds HOLE everywhere: above, and this loop below)
        assert out is view
        if looked:
            assert np.array_equal(cnt, cnt0) and fin2 == []
        fin = fin + fin2
        for s in range(n_slots):
            if s not in slot_utt:
                continue
            u, had = slot_utt[s], len(tiled[slot_utt[s]])
            assert cnt[s] >= had
            assert (out[s, :had] == HOLE).all() and (out[s, cnt[s]:] == HOLE).all(), "a wait writes only what no earlier wait handed out"
            assert (out[s, had:cnt[s]] != HOLE).all(), "no gap"
            tiled[u] += out[s, had:cnt[s]].tolist()
            assert bool(done[s]) == (s in [f for f, _ in fin])
        out[:] = HOLE
        assert [s for s, _ in fin] == sorted(s for s, _ in fin)
        for s, c in fin:
            u = slot_utt.pop(s)
            assert c == len(tiled[u])
            collected[u] = eng.stream_collect(s, c).tolist()
            reported.append(u)
            free.append(s)
        if drop_utt is not None and drop_utt in slot_utt.values():
            s = [k for k, v in slot_utt.items() if v == drop_utt][0]
            eng.stream_drop([s])
            del slot_utt[s]
            free.insert(0, s)                                             # admissible at once: the next admission takes it
        assert i < 2000
    eng.stream_launch(5)                                                  # no live rows: nothing is launched, the wait is a pure look-in
    assert eng.stream_wait(out=view)[3] == [] and (view == HOLE).all()
    eng.stream_end()
    return tiled, collected, reported


def _run_session(eng, mode, prompts, uni, n_slots, stop, sizes):
    """the same schedule on stream_run / stream_collect: run sizes in the same turn, slots refilled in the same order"""
    _begin(eng, mode, n_slots, stop)
    free, slot_utt, out, nxt, i = list(range(n_slots)), {}, [None] * len(prompts), 0, 0
    while nxt < len(prompts) or slot_utt:
        while nxt < len(prompts) and free:
            s = free.pop(0)
            _admit(eng, mode, s, nxt, prompts, uni)
            slot_utt[s] = nxt
            nxt += 1
        for s, c in eng.stream_run(sizes[i % len(sizes)]):
            out[slot_utt.pop(s)] = eng.stream_collect(s, c).tolist()
            free.append(s)
        i += 1
    eng.stream_end()
    return out


PARAMS = [pytest.mark.parametrize("mode", ["greedy", "stopped", "sampled", "mixed"]), pytest.mark.parametrize("wtype", [gguf.F16, gguf.Q4_0], ids=["f16", "q4_0"]),
          pytest.mark.parametrize("n_slots", [3, 7])]


def _all(marks):
    def wrap(f):
        for m in marks:
            f = m(f)
        return f
    return wrap


@_all(PARAMS)
def test_waits_tile_every_occupants_ids(n_slots, wtype, mode):
    """launch sizes 1 / 5 / 28 / 37 and their rotation: the ids the waits hand out tile each occupant's sequence (every wait writes exactly the
    cells no earlier wait wrote), equal stream_collect, and equal a stream_run session on a fresh context that runs the same sizes in the same
    turn (3 slots: the 1-4-row kernels; 7: the weight-streaming GEMM, falling to <= 4 live rows as utterances end)"""
    model, prompts, uni, refs = _reference(n_slots, wtype)
    stop, _ = refs[mode]
    eng = hip.OrpheusEngine(model.cfg, max_seqs=n_slots)
    eng.load(model)
    fresh = hip.OrpheusEngine(model.cfg, max_seqs=n_slots)
    fresh.load(model)
    for k, sizes in enumerate(SIZES):
        tiled, collected, reported = _launch_session(eng, mode, prompts, uni, n_slots, stop, sizes, look_every=3 if k % 2 else 0)
        assert collected == tiled, sizes
        assert sorted(reported) == list(range(len(prompts)))
        assert _run_session(fresh, mode, prompts, uni, n_slots, stop, sizes) == tiled, sizes
        if mode == "stopped":
            assert len({len(t) for t in tiled}) > 1 and min(len(t) for t in tiled) < MAX_NEW, "rows end inside a launch"
    eng.close()
    fresh.close()


@_all(PARAMS)
def test_waits_hand_out_each_utterances_one_sequence_ids(n_slots, wtype, mode):
    """the ids the waits hand out equal each utterance's own one-sequence generation (the eager engine), launch sizes 1 / 5 / 28 / 37 in rotation;
    the sampled draws are steady ones (LOGIT_MARGIN above), because 5 or more rows and one row go through kernels that round differently"""
    model, prompts, uni, refs = _reference(n_slots, wtype)
    stop, ref = refs[mode]
    eng = hip.OrpheusEngine(model.cfg, max_seqs=n_slots)
    eng.load(model)
    tiled, _, _ = _launch_session(eng, mode, prompts, uni, n_slots, stop, SIZES[-1])
    eng.close()
    for u, (a, b) in enumerate(zip(tiled, ref)):
        if a != b:
            print("utterance", u, "first differing id at", next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b))))
    assert tiled == ref


@pytest.mark.parametrize("mode", ["stopped", "mixed"])
def test_a_drop_changes_no_other_slot(mode):
    model, prompts, uni, refs = _reference(3, gguf.F16)
    stop, ref = refs[mode]
    eng = hip.OrpheusEngine(model.cfg, max_seqs=3)
    eng.load(model)
    d = next(u for u in range(3) if len(ref[u]) > 6)                     # still live after its admission and one launch of 5
    plain, _, _ = _launch_session(eng, mode, prompts, uni, 3, stop, [5])
    tiled, collected, reported = _launch_session(eng, mode, prompts, uni, 3, stop, [5], drop_utt=d)
    assert d not in reported and collected[d] is None, "a dropped slot is never reported"
    assert tiled[d] == ref[d][:6]
    for u in range(len(prompts)):
        if u != d:
            assert tiled[u] == plain[u] == ref[u] == collected[u], u
    assert sorted(reported) == [u for u in range(len(prompts)) if u != d]
    eng.close()


def test_calls_with_steps_in_flight_are_refused():
    model, prompts, uni, refs = _reference(3, gguf.F16)
    never, ref = refs["greedy"]
    eng = hip.OrpheusEngine(model.cfg, max_seqs=3)
    eng.load(model)
    eng.stream_begin(3, MAX_NEW, never)
    eng.stream_admit([0, 1], prompts[:2])
    out, cnt, done, fin = eng.stream_wait()                              # nothing in flight: a pure look-in, the admissions' first ids
    assert cnt.tolist() == [1, 1, 0] and fin == [] and [out[0, 0], out[1, 0]] == [ref[0][0], ref[1][0]]
    eng.stream_launch(5)
    in_flight = [lambda: eng.stream_admit([2], prompts[2:3]), lambda: eng.stream_collect(0, 1), lambda: eng.stream_drop([0]), lambda: eng.stream_run(3),
                 lambda: eng.stream_launch(2)]
    for call in in_flight:
        with pytest.raises(hip.HipError, match="in flight"):
            call()
    for call in (lambda: eng.decode(prompts[0], 0), lambda: eng.generate_greedy(prompts[0], MAX_NEW, never), lambda: eng.gen_begin([prompts[0]], MAX_NEW, never),
                 lambda: eng.gen_launch(5), lambda: eng.step_batch([0], [3], [0]), lambda: eng.stream_begin(3, MAX_NEW, never)):
        with pytest.raises(hip.HipError):
            call()
    out, cnt, done, fin = eng.stream_wait()
    assert cnt.tolist() == [6, 6, 0] and fin == []
    assert out[0, :6].tolist() == ref[0][:6] and out[1, :6].tolist() == ref[1][:6]
    for bad, what in (([2], "not live"), ([3], "n_slots"), ([0, 0], "twice")):
        with pytest.raises(hip.HipError, match=what):
            eng.stream_drop(bad)
    eng.stream_admit([2], prompts[2:3])
    got = {}
    while len(got) < 3:
        eng.stream_launch(28)
        out, cnt, done, fin = eng.stream_wait()
        for s, c in fin:
            got[s] = out[s, :c].tolist()
            assert got[s] == eng.stream_collect(s, c).tolist()
    assert [got[0], got[1], got[2]] == ref[:3]
    eng.stream_admit([1], prompts[3:4])
    eng.stream_launch(4)
    eng.stream_end()                                                     # with steps in flight: synchronises and ends
    assert eng.generate_greedy(prompts[3], MAX_NEW, never).tolist() == ref[3]
    eng.close()


# ---- the runner ------------------------------------------------------------------------------------------------------------------------
FRAMES = 40
TEXTS = ["hello the zebra", "hello", "the zebra the hello a zoe", "a zoe", "zebra hello", "the the hello", "hello zoe the zebra"]
HEADS = [0, 1, 2, 2, 1, 2, 2]
MODES = {"greedy": dict(sample=0), "device": dict(sample=1, top_k=8, temperature=0.9, seed=1234)}


@pytest.fixture(scope="module")
def full_model(tmp_path_factory):
    full = synth.SynthOrpheusFull(scfg=synth.snac_tiny(max_frames=4 * FRAMES), max_gen=7 * FRAMES)
    return full, full.write_gguf(str(tmp_path_factory.mktemp("orpheus_stream_chunked") / "m.gguf"))


@pytest.fixture()
def no_noise():
    os.environ["TTS_SNAC_NO_NOISE"] = "1"
    yield
    os.environ.pop("TTS_SNAC_NO_NOISE", None)


@pytest.fixture(scope="module")
def session_runner(full_model):
    """one runner with three slots and, per mode, every text's generate() audio and ids (made without the noise block)"""
    full, path = full_model
    os.environ["TTS_SNAC_NO_NOISE"] = "1"
    try:
        r = runner.Runner(path, sample=0, max_seqs=3)
        refs = {}
        for mode, cfg in MODES.items():
            refs[mode] = []
            for t in TEXTS:
                pcm = r.generate(t, voice=b"zoe", **cfg)
                refs[mode].append((pcm, r.last_tokens(1).copy()))
    finally:
        os.environ.pop("TTS_SNAC_NO_NOISE", None)
    yield r, refs
    r.close()


@pytest.mark.parametrize("cf", [1, 3, 16])
@pytest.mark.parametrize("mode", ["greedy", "device"])
def test_session_chunks_equal_generate(full_model, session_runner, no_noise, mode, cf):
    full, _ = full_model
    r, refs = session_runner
    per = 4 * full.scfg.hop
    t_start = time.monotonic()
    got = r.generate_stream_chunked(TEXTS, chunk_frames=cf, voice=b"zoe", **MODES[mode])
    t_end = time.monotonic()
    assert not r.stopped
    for i, (ref, toks) in enumerate(refs[mode]):
        assert toks.size == 7 * FRAMES and ref.size == FRAMES * per     # random weights do not emit the stopping id
        mine = [(a, t) for utt, a, t in got if utt == i]
        assert len(mine) == -(-FRAMES // cf), f"utterance {i}: one chunk per utterance is not streaming"
        sizes = [a.size for a, _ in mine]
        assert all(s == cf * per for s in sizes[:-1]) and 0 < sizes[-1] <= cf * per, "all chunks full but the last"
        pcm = np.concatenate([a for a, _ in mine])
        assert pcm.size == ref.size
        assert np.abs(pcm - ref).max() <= 1e-6, f"utterance {i}, chunk_frames {cf}"
        assert np.array_equal(r.last_tokens(16 + i), toks), f"utterance {i}"
        stamps = [t for _, t in mine]
        assert stamps == sorted(stamps)
    for i in range(3):                                                   # admitted first: their first chunks come while the session runs
        first = min(t for utt, _, t in got if utt == i)
        assert first - t_start < 0.5 * (t_end - t_start), f"utterance {i}"


def test_a_callback_that_stops_one_utterance(full_model, session_runner, no_noise):
    full, _ = full_model
    r, refs = session_runner
    per = 4 * full.scfg.hop
    got = r.generate_stream_chunked(TEXTS, chunk_frames=3, voice=b"zoe", sample=0, on_chunk=lambda utt, a, t: utt != 1)
    assert r.stopped
    for i, (ref, toks) in enumerate(refs["greedy"]):
        mine = [a for utt, a, _ in got if utt == i]
        if i == 1:
            assert len(mine) == 1 and mine[0].size == 3 * per and np.abs(mine[0] - ref[:3 * per]).max() <= 1e-6
            short = r.last_tokens(16 + 1)
            assert 0 < short.size < toks.size and np.array_equal(short, toks[:short.size])
            continue
        assert len(mine) == -(-FRAMES // 3)
        assert np.abs(np.concatenate(mine) - ref).max() <= 1e-6, f"utterance {i}"
        assert np.array_equal(r.last_tokens(16 + i), toks)
    again = r.generate(TEXTS[0], voice=b"zoe", sample=0)
    assert np.array_equal(again, refs["greedy"][0][0]) and np.array_equal(r.last_tokens(1), refs["greedy"][0][1])
    with pytest.raises(runner.RunnerError):
        r.generate_stream_chunked(TEXTS, chunk_frames=0, voice=b"zoe", sample=0)


def _snac_inputs(full, toks):
    levels = [[], [], []]
    for i in range(len(toks) // 7):
        for ii in range(7):
            levels[HEADS[ii]].append(int(toks[i * 7 + ii]) - full.audio_offset)
    return np.array(levels[0] + levels[1] + levels[2], dtype=np.uint32), len(levels[2])


def test_session_chunks_with_the_noise_block(full_model):
    """the reference construction of test_gpu_orpheus_chunked.py::test_chunks_with_the_noise_block: the session draws each frame's noise once,
    frame-major, from the engine generate() draws layer-major from, and a finished utterance has consumed what its generate() would"""
    from rng_oracle import minstd0_normal
    full, path = full_model
    scfg = full.scfg
    so = orc.SnacOracle(full.snac)
    r = runner.Runner(path, sample=0, max_seqs=3)   # a fresh runner: the engine is at its first state
    got = r.generate_stream_chunked(TEXTS[:1], chunk_frames=3, voice=b"zoe", sample=0)
    codes, T = _snac_inputs(full, r.last_tokens(16))
    F = T // 4
    assert F == FRAMES and len(got) == -(-FRAMES // 3)
    draws, _, _ = minstd0_normal(so.noise_len(T))
    ups = np.cumprod(scfg.strides)
    per_frame = draws.reshape(F, -1)   # frame-major: [frame][layer 0 | layer 1 | ...]
    offs = np.concatenate([[0], np.cumsum(4 * ups)])
    relaid = np.concatenate([per_frame[:, offs[l]:offs[l + 1]].reshape(-1) for l in range(len(ups))])
    ref = so.decode(codes, T, relaid)
    pcm = np.concatenate([a for _, a, _ in got])
    assert pcm.shape == ref.shape and np.abs(pcm - ref).max() < 1e-4
    r.close()
    r = runner.Runner(path, sample=0, max_seqs=3)
    r.generate_stream_chunked(TEXTS[:2], chunk_frames=16, voice=b"zoe", sample=0)
    assert r.last_tokens(16).size == r.last_tokens(17).size == 7 * FRAMES
    _, state, saved = minstd0_normal(2 * so.noise_len(T))               # both utterances' draws, whatever their interleaving
    pcm2 = r.generate(TEXTS[0], voice=b"zoe", sample=0)
    codes2, T2 = _snac_inputs(full, r.last_tokens(1))
    noise2, _, _ = minstd0_normal(so.noise_len(T2), state, saved)
    assert np.abs(pcm2 - so.decode(codes2, T2, noise2)).max() < 1e-4
    r.close()
