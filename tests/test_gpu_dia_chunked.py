"""GPU: chunked Dia audio.  The generation loop in pieces (tts_hip_dia_gen_begin / _launch / _wait) against tts_hip_dia_generate, and the
runner's chunked generation (dia_runner::generate_chunked / generate_batch_chunked) against generate() / generate_batch() in both loop
modes.  160 steps give an utterance well over 100 codec frames against the tiny codec's 19-frame halo."""
import os
import time

import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import hip, runner, synth

pytestmark = pytest.mark.gpu

MAX_GEN = 160
MARK = 0xFFFFFFFF
TEXT = " Hi there [S2] ok"
TEXTS = [" Hi there [S2] ok", "[S1] another one.", "[S2] short"]
LAUNCHES = (1, 5, 16, 37)


def relerr(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _args(cfg):
    return dict(delay_pattern=[0, 8, 9, 10, 11, 12, 13, 14, 15], bos=cfg.bos, eos=cfg.eos, pad=cfg.pad, max_delay=cfg.max_delay)


@pytest.fixture(scope="module")
def engine():
    model = synth.build_dia(synth.dia_tiny(max_gen=MAX_GEN), suppress_special=False)
    eng = hip.DiaEngine(model.cfg, max_utterances=3)
    eng.load(model)
    for u, t in enumerate(TEXTS):
        eng.encode_slot(u, *orc.dia_tokenize(t, model.cfg.max_ctx))
    yield model.cfg, eng
    eng.close()


def _sampling(cfg, n_utt, mode):
    if mode == "greedy":
        return {}
    u = np.random.default_rng(21).random((MAX_GEN, n_utt, cfg.n_out), dtype=np.float32)
    return dict(uniforms=u, top_k=12, temperature=0.9, repetition_penalty=1.3 if mode == "sampled_rep" else 1.0)


@pytest.mark.parametrize("mode", ["greedy", "sampled", "sampled_rep"])
@pytest.mark.parametrize("n_utt", [1, 3])
def test_loop_in_pieces_equals_generate(engine, n_utt, mode):
    cfg, eng = engine
    kw = dict(_args(cfg), **_sampling(cfg, n_utt, mode))
    ref = eng.generate(n_utt, MAX_GEN, **kw)
    assert all(len(r) > cfg.max_delay for r in ref)
    eng.gen_begin(n_utt, MAX_GEN, **kw)
    prev = np.zeros(n_utt, dtype=np.uint32)
    snap = None
    launched = k = 0
    while True:
        size = LAUNCHES[k % len(LAUNCHES)]
        eng.gen_launch(size)
        launched = min(launched + size, MAX_GEN + 1)
        if k == 2:   # a look-in that takes nothing: the rows stay for the next one
            out, steps, done, ran = eng.gen_wait(take=False)
            assert ran == launched and (steps >= prev).all()
            for u in range(n_utt):
                assert (out[u, prev[u]:] == MARK).all()
        out, steps, done, ran = eng.gen_wait()
        assert ran == launched
        for u in range(n_utt):
            assert prev[u] <= steps[u] <= min(ran, MAX_GEN)
            assert (out[u, :steps[u]] != MARK).all(), "no gap: every step so far has been handed out"
            assert (out[u, steps[u]:] == MARK).all(), "nothing beyond the steps made"
            if snap is not None:
                assert np.array_equal(out[u, :prev[u]], snap[u, :prev[u]]), "no overlap: earlier rows are not written again"
        snap, prev = out.copy(), steps
        k += 1
        if done.all() or ran == MAX_GEN + 1:
            break
    assert done.all()
    for u in range(n_utt):
        assert steps[u] == len(ref[u]) and np.array_equal(out[u, :steps[u]], ref[u]), (u, mode)
    eng.gen_launch(16)   # over: nothing is launched any more
    assert eng.gen_wait()[3] == ran


def test_a_step_after_an_abandoned_loop_works(engine):
    cfg, eng = engine
    ids = np.full(cfg.n_out, cfg.bos, dtype=np.uint32)
    before = eng.step(ids, 0).copy()
    eng.gen_begin(2, MAX_GEN, **_args(cfg))
    eng.gen_launch(5)   # in flight, never waited for
    after = eng.step(ids, 0)
    assert relerr(after, before) < 1e-5
    with pytest.raises(hip.HipError):
        eng.gen_launch(1)   # the step dropped the loop
    with pytest.raises(hip.HipError):
        eng.gen_wait()
    ref = eng.generate(1, 40, **_args(cfg))   # and the context generates as before
    eng.gen_begin(1, 40, **_args(cfg))
    eng.gen_launch(41)
    out, steps, done, _ = eng.gen_wait()
    assert done.all() and np.array_equal(out[0, :steps[0]], ref[0])
    eng.encode_slot(0, *orc.dia_tokenize(TEXTS[0], cfg.max_ctx))   # encode drops a finished loop as well


def test_new_symbols_resolve():
    L = hip.load_lib()
    for name in ("tts_hip_dia_gen_begin", "tts_hip_dia_gen_launch", "tts_hip_dia_gen_wait"):
        assert getattr(L, name) is not None
        assert name in hip.EXPORTS


@pytest.fixture(scope="module", params=[True, False], ids=["audio_ids_only", "special_ids"])
def dia_runner(request, tmp_path_factory):
    model = synth.build_dia(synth.dia_tiny(max_gen=MAX_GEN), suppress_special=request.param)
    path = model.write_gguf(str(tmp_path_factory.mktemp("dia_chunked") / "dia.gguf"))
    r = runner.Runner(path, sample=0, max_seqs=3)
    yield model, r, request.param
    r.close()


def _modes(suppressed):
    if suppressed:
        return [dict(sample=0), dict(sample=1, top_k=20, temperature=0.9, seed=1234)]
    # the special-id rows of the heads take part: frames with EOS / PAD are dropped, and max_tokens ends the loop through the countdown
    return [dict(sample=0, max_tokens=120), dict(sample=1, top_k=0, top_p=0.95, temperature=1.3, seed=77, max_tokens=120)]


@pytest.mark.parametrize("host_loop", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_chunks_equal_generate(dia_runner, host_loop, mode):
    model, r, suppressed = dia_runner
    hop = model.cfg.hop
    cfg = _modes(suppressed)[mode]
    if host_loop:
        os.environ["TTS_HOST_LOOP"] = "1"
    try:
        ref = r.generate(TEXT, **cfg)
        toks = r.last_tokens(1).copy()
        steps = toks.size // model.cfg.n_out
        assert steps == cfg.get("max_tokens", MAX_GEN) - 1 or not suppressed
        frames = ref.size // hop
        print(f"{steps} steps, {frames} kept frames")
        assert ref.size % hop == 0 and frames > 0
        if suppressed:
            assert frames > 100
        else:
            assert frames < steps - model.cfg.max_delay, "frames holding special ids must have been dropped"
        for cf in (1, 7, 32, 10000):
            chunks = r.generate_chunked(TEXT, chunk_frames=cf, **cfg)
            assert not r.stopped
            sizes = [a.size for a, _ in chunks]
            assert all(s % hop == 0 and 0 < s <= cf * hop for s in sizes)
            assert all(s == cf * hop for s in sizes[:-1]), "only the last chunk may be short"
            pcm = np.concatenate([a for a, _ in chunks])
            assert pcm.size == ref.size, f"chunk_frames {cf}"
            diff = float(np.abs(pcm - ref).max())
            print(f"chunk_frames {cf}: {len(chunks)} chunks, max |chunked - generate| = {diff:.3e}, bit-equal {np.array_equal(pcm, ref)}")
            assert diff <= 1e-6, f"chunk_frames {cf}"
            assert np.array_equal(r.last_tokens(1), toks)
            stamps = [t for _, t in chunks]
            assert stamps == sorted(stamps)
            if cf == 10000:
                assert len(chunks) == 1
    finally:
        os.environ.pop("TTS_HOST_LOOP", None)


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_chunks_equal_generate_batch(dia_runner, mode):
    model, r, suppressed = dia_runner
    cfg = _modes(suppressed)[mode]
    ref = r.generate_batch(TEXTS, **cfg)
    got = r.generate_batch_chunked(TEXTS, chunk_frames=16, **cfg)
    assert not r.stopped
    per = {i: [] for i in range(len(TEXTS))}
    for utt, a, t in got:
        per[utt].append((a, t))
    hop = model.cfg.hop
    for i, b in enumerate(ref):
        sizes = [a.size for a, _ in per[i]]
        assert all(s == 16 * hop for s in sizes[:-1]) and 0 < sizes[-1] <= 16 * hop
        pcm = np.concatenate([a for a, _ in per[i]])
        assert pcm.size == b.size and b.size > 0
        diff = float(np.abs(pcm - b).max())
        print(f"utterance {i}: max |chunked - generate_batch| = {diff:.3e}, bit-equal {np.array_equal(pcm, b)}")
        assert diff <= 1e-6, f"utterance {i}"
        stamps = [t for _, t in per[i]]
        assert stamps == sorted(stamps)


def test_audio_arrives_early_and_cancelling_stops(tmp_path):
    model = synth.build_dia(synth.dia_tiny(max_gen=MAX_GEN), suppress_special=True)   # greedy never stops early: MAX_GEN - 1 steps
    r = runner.Runner(model.write_gguf(str(tmp_path / "dia.gguf")), sample=0)
    ref = r.generate(TEXT)   # warm-up, and the reference
    full_tokens = r.last_tokens(1).copy()
    assert full_tokens.size == (MAX_GEN - 1) * model.cfg.n_out
    r.generate_chunked(TEXT, chunk_frames=16)   # warm-up of the window passes
    t_start = time.monotonic()
    chunks = r.generate_chunked(TEXT, chunk_frames=16)
    t_end = time.monotonic()
    assert np.abs(np.concatenate([a for a, _ in chunks]) - ref).max() <= 1e-6
    first = chunks[0][1] - t_start
    print(f"{len(chunks)} chunks, first after {first * 1e3:.1f} ms of {(t_end - t_start) * 1e3:.1f} ms")
    assert len(chunks) > 2
    assert first < 0.5 * (t_end - t_start), "the first chunk must arrive before half of the call's wall time"

    seen = []
    rc = r.generate_chunked(TEXT, chunk_frames=16, on_chunk=lambda a, t: seen.append(a) or False)
    assert r.stopped and len(rc) == 1 and len(seen) == 1
    assert 0 < r.last_tokens(1).size < full_tokens.size
    assert np.array_equal(r.last_tokens(1), full_tokens[:r.last_tokens(1).size])
    assert np.abs(rc[0][0] - ref[:rc[0][0].size]).max() <= 1e-6
    again = r.generate(TEXT)
    assert np.array_equal(again, ref) and np.array_equal(r.last_tokens(1), full_tokens)
    r.close()


def test_chunk_frames_zero_is_an_error(dia_runner):
    _, r, _ = dia_runner
    with pytest.raises(runner.RunnerError):
        r.generate_chunked(TEXT, chunk_frames=0)
    with pytest.raises(runner.RunnerError):
        r.generate_batch_chunked(TEXTS, chunk_frames=0)
