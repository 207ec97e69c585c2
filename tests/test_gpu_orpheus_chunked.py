"""GPU: chunked Orpheus audio.  SNAC windows (tts_hip_snac_decode_windows) against the whole-utterance decode and the oracle, the Orpheus
generation loops in pieces (tts_hip_orpheus_gen_*) against the one-call loops, and the runner's generate_chunked / generate_batch_chunked
against generate() / generate_batch() in every loop mode."""
import os
import time

import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import hip, runner, synth

pytestmark = pytest.mark.gpu

TEXT = "hello the zebra"
TEXTS = ["hello the zebra", "hello", "the zebra the hello a zoe"]
HEADS = [0, 1, 2, 2, 1, 2, 2]


def _levels(cfg, K, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, cfg.cb_size, 4 * K // r).astype(np.uint32) for r in cfg.repeats]


def _codes(levels, f0, f1):
    return np.concatenate([l[f0 * (4 // r):f1 * (4 // r)] for l, r in zip(levels, (4, 2, 1))])


def _noise_layers(cfg, K, seed):
    rng = np.random.default_rng(seed)
    out, up = [], 1
    for s in cfg.strides:
        up *= s
        out.append(rng.standard_normal(4 * K * up).astype(np.float32))
    return out


def _noise(cfg, layers, f0, f1):
    out, up = [], 1
    for s, l in zip(cfg.strides, layers):
        up *= s
        out.append(l[f0 * 4 * up:f1 * 4 * up])
    return np.concatenate(out)


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("layout", ["tiny", "24khz"])
def test_windows_equal_the_full_decode(layout, with_noise):
    K = 40
    cfg = synth.snac_tiny(max_frames=4 * K) if layout == "tiny" else synth.snac_24khz(max_frames=4 * K)
    model = synth.build_snac(cfg)
    eng = hip.SnacEngine(cfg)
    eng.load(model)
    o = orc.SnacOracle(model)
    h = eng.halo_frames()
    assert h == (5 if layout == "tiny" else 3)
    levels = _levels(cfg, K, 11)
    nl = _noise_layers(cfg, K, 12) if with_noise else None
    nz = (lambda a, b: _noise(cfg, nl, a, b)) if with_noise else (lambda a, b: None)
    full = eng.decode(_codes(levels, 0, K), 4 * K, nz(0, K))
    per = 4 * cfg.hop
    tol_oracle = 1e-4 if layout == "tiny" else 2e-4   # tests/test_gpu_snac.py's bars
    assert np.abs(full - o.decode(_codes(levels, 0, K), 4 * K, nz(0, K))).max() < tol_oracle
    edges = [0, 3, 19, 20, 31, K]   # clipped at 0, interior (one of a single frame), clipped at K
    ws = [(max(0, f0 - h), min(K, f1 + h), f0, f1) for f0, f1 in zip(edges[:-1], edges[1:])]
    args = [(_codes(levels, w0, w1), w1 - w0, f0 - w0, f1 - w0, nz(w0, w1)) for w0, w1, f0, f1 in ws]
    for split in (False, True):
        got = eng.decode_windows(args, split=split)   # several windows in one call
        for (w0, w1, f0, f1), g in zip(ws, got):
            assert g.shape == ((f1 - f0) * per,)
            assert np.abs(g - full[f0 * per:f1 * per]).max() <= 1e-6, f"window [{w0}, {w1}) keeping [{f0}, {f1})"
            ref = o.decode(_codes(levels, w0, w1), 4 * (w1 - w0), nz(w0, w1))[(f0 - w0) * per:(f1 - w0) * per]
            assert np.abs(g - ref).max() < tol_oracle
        assert np.abs(np.concatenate(got) - full).max() <= 1e-6
    one = eng.decode_windows(args[2:3])   # a single window of a single frame
    assert np.abs(one[0] - full[19 * per:20 * per]).max() <= 1e-6
    assert np.array_equal(full, eng.decode(_codes(levels, 0, K), 4 * K, nz(0, K)))   # the whole-utterance decode after window passes
    with pytest.raises(hip.HipError):
        eng.decode_windows([(_codes(levels, 0, 4), 4, 2, 5, nz(0, 4))])   # keeps frames beyond the window
    eng.close()


def _collect(eng, sizes):
    """run a begun generation to its end with launch sizes taken from `sizes` in turn"""
    ids, done = eng.gen_wait()
    i = 0
    while not done.all():
        eng.gen_launch(sizes[i % len(sizes)])
        i += 1
        new, done = eng.gen_wait()
        for a, b in zip(ids, new):
            assert np.array_equal(a, b[:a.size]), "ids handed out earlier must not change"
        ids = new
    return ids


@pytest.mark.parametrize("graph", [False, True])
def test_generation_in_pieces_equals_the_one_call_loops(graph):
    model = synth.build_orpheus(synth.orpheus_tiny())
    cfg = model.cfg
    if graph:
        os.environ["TTS_HIP_LLAMA_GRAPH"] = "1"
    try:
        eng = hip.OrpheusEngine(cfg)
    finally:
        os.environ.pop("TTS_HIP_LLAMA_GRAPH", None)
    eng.load(model)
    prompt = np.array([3, 17, 5, 9, 2], dtype=np.uint32)
    max_new, nostop = 45, cfg.vocab + 5
    ref = eng.generate_greedy(prompt, max_new, nostop)
    assert ref.size == max_new
    stop = int(ref[20])
    ref_stop = eng.generate_greedy(prompt, max_new, stop)
    assert 0 < ref_stop.size <= 21
    u = np.random.default_rng(5).random(max_new).astype(np.float32)
    ref_s = eng.generate_sampled(prompt, max_new, nostop, u, top_k=8, temperature=0.9, repetition_penalty=1.1)
    for sizes in ([1], [5], [8], [64], [1, 5, 8, 64]):
        eng.gen_begin([prompt], max_new, nostop)
        assert np.array_equal(_collect(eng, sizes)[0], ref), sizes
        eng.gen_begin([prompt], max_new, stop)   # steps a launch ran past the stopping token are discarded
        assert np.array_equal(_collect(eng, sizes)[0], ref_stop), sizes
        eng.gen_begin([prompt], max_new, nostop, uniforms=u, top_k=8, temperature=0.9, repetition_penalty=1.1)
        assert np.array_equal(_collect(eng, sizes)[0], ref_s), sizes
    # between a launch and its wait the steps may still be running: every other call on the context is refused, the generation goes on
    eng.gen_begin([prompt], max_new, nostop)
    eng.gen_wait()
    eng.gen_launch(5)
    for call in (lambda: eng.decode(prompt, 0), lambda: eng.generate_greedy(prompt, max_new, nostop), lambda: eng.gen_begin([prompt], max_new, nostop),
                 lambda: eng.gen_launch(5), lambda: eng.step_batch([0], [3], [0])):
        with pytest.raises(hip.HipError):
            call()
    assert np.array_equal(_collect(eng, [8])[0], ref)
    assert np.array_equal(eng.generate_greedy(prompt, max_new, nostop), ref)
    with pytest.raises(hip.HipError):
        eng.gen_launch(4)   # no generation under way
    eng.close()


def test_lockstep_generation_in_pieces_equals_generate_batch():
    model = synth.build_orpheus(synth.orpheus_tiny())
    cfg = model.cfg
    eng = hip.OrpheusEngine(cfg, max_seqs=3)
    eng.load(model)
    prompts = [np.array([3, 17, 5, 9, 2], dtype=np.uint32), np.array([4, 4, 8], dtype=np.uint32), np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=np.uint32)]
    max_new, nostop = 30, cfg.vocab + 5
    ref = eng.generate_batch(prompts, max_new, nostop)
    stop = int(ref[1][11])
    ref_stop = eng.generate_batch(prompts, max_new, stop)
    assert min(r.size for r in ref_stop) < max_new
    u = np.random.default_rng(6).random((3, max_new)).astype(np.float32)
    ref_s = eng.generate_batch(prompts, max_new, nostop, uniforms=u, top_k=8, temperature=0.9)
    for sizes in ([1], [5], [64]):
        eng.gen_begin(prompts, max_new, nostop)
        assert all(np.array_equal(a, b) for a, b in zip(_collect(eng, sizes), ref)), sizes
        eng.gen_begin(prompts, max_new, stop)
        assert all(np.array_equal(a, b) for a, b in zip(_collect(eng, sizes), ref_stop)), sizes
        eng.gen_begin(prompts, max_new, nostop, uniforms=u, top_k=8, temperature=0.9)
        assert all(np.array_equal(a, b) for a, b in zip(_collect(eng, sizes), ref_s)), sizes
    eng.close()


FRAMES = 40


@pytest.fixture(scope="module")
def full_model(tmp_path_factory):
    full = synth.SynthOrpheusFull(scfg=synth.snac_tiny(max_frames=4 * FRAMES), max_gen=7 * FRAMES)
    return full, full.write_gguf(str(tmp_path_factory.mktemp("orpheus_chunked") / "m.gguf"))


@pytest.fixture()
def no_noise():
    os.environ["TTS_SNAC_NO_NOISE"] = "1"
    yield
    os.environ.pop("TTS_SNAC_NO_NOISE", None)


MODES = {"greedy": dict(sample=0), "device": dict(sample=1, top_k=8, temperature=0.9, seed=1234), "host": dict(sample=1, top_k=8, temperature=0.9, seed=1234)}


@pytest.mark.parametrize("mode", ["greedy", "device", "host"])
def test_chunks_equal_generate(full_model, no_noise, mode):
    full, path = full_model
    per = 4 * full.scfg.hop
    cfg = MODES[mode]
    if mode == "host":
        os.environ["TTS_HOST_LOOP"] = "1"
    try:
        r = runner.Runner(path, sample=0)
        ref = r.generate(TEXT, voice=b"zoe", **cfg)
        toks = r.last_tokens(1).copy()
        assert toks.size == 7 * FRAMES and ref.size == FRAMES * per   # random weights do not emit the stopping id
        for cf in (1, 3, 16, 10000):
            chunks = r.generate_chunked(TEXT, chunk_frames=cf, voice=b"zoe", **cfg)
            assert not r.stopped
            sizes = [a.size for a, _ in chunks]
            assert all(s % per == 0 and 0 < s <= cf * per for s in sizes)
            assert all(s == cf * per for s in sizes[:-1]), "only the last chunk may be short"
            assert len(chunks) == -(-FRAMES // cf), "one chunk of the whole utterance is not streaming"
            pcm = np.concatenate([a for a, _ in chunks])
            assert pcm.size == ref.size, f"chunk_frames {cf}"
            assert np.abs(pcm - ref).max() <= 1e-6, f"chunk_frames {cf}"
            assert np.array_equal(r.last_tokens(1), toks)
            stamps = [t for _, t in chunks]
            assert stamps == sorted(stamps)
        r.close()
    finally:
        os.environ.pop("TTS_HOST_LOOP", None)


@pytest.mark.parametrize("mode", ["greedy", "device"])
def test_batch_chunks_equal_generate_batch(full_model, no_noise, mode):
    full, path = full_model
    cfg = MODES[mode]
    r = runner.Runner(path, sample=0, max_seqs=4)
    ref = r.generate_batch(TEXTS, voice=b"zoe", **cfg)
    got = r.generate_batch_chunked(TEXTS, chunk_frames=3, voice=b"zoe", **cfg)
    assert not r.stopped
    per = {i: [] for i in range(len(TEXTS))}
    for utt, a, t in got:
        per[utt].append((a, t))
    for i, b in enumerate(ref):
        assert len(per[i]) > 2
        pcm = np.concatenate([a for a, _ in per[i]])
        assert pcm.size == b.size and b.size > 0
        assert np.abs(pcm - b).max() <= 1e-6, f"utterance {i}"
        stamps = [t for _, t in per[i]]
        assert stamps == sorted(stamps)
    # ready chunks are handed out before the next (blocking) piece of lock-step steps: every utterance's first chunk (frames 0..2, ready after
    # 8 of 40 frames) arrives in the first half of the call
    t_start = time.monotonic()
    got = r.generate_batch_chunked(TEXTS, chunk_frames=3, voice=b"zoe", **cfg)
    t_end = time.monotonic()
    for i in range(len(TEXTS)):
        first = min(t for utt, _, t in got if utt == i)
        assert first - t_start < 0.5 * (t_end - t_start), f"utterance {i}"
    r.close()


def _snac_inputs(full, toks):
    levels = [[], [], []]
    for i in range(len(toks) // 7):
        for ii in range(7):
            levels[HEADS[ii]].append(int(toks[i * 7 + ii]) - full.audio_offset)
    return np.array(levels[0] + levels[1] + levels[2], dtype=np.uint32), len(levels[2])


def test_chunks_with_the_noise_block(full_model):
    """Chunked generation draws the noise frame-major (per frame, for layer l, 4 * prod(stride_0..l) normals) from the engine generate() draws
    layer-major from: the chunks equal the oracle's decode of the whole utterance under the re-laid array, and a completed call leaves the
    engine where generate() would have."""
    from rng_oracle import minstd0_normal
    full, path = full_model
    scfg = full.scfg
    r = runner.Runner(path, sample=0)   # a fresh runner: the engine is at its first state
    chunks = r.generate_chunked(TEXT, chunk_frames=3, voice=b"zoe", sample=0)
    codes, T = _snac_inputs(full, r.last_tokens(1))
    F = T // 4
    assert F == FRAMES
    so = orc.SnacOracle(full.snac)
    draws, state, saved = minstd0_normal(so.noise_len(T))
    ups = np.cumprod(scfg.strides)
    per_frame = draws.reshape(F, -1)   # frame-major: [frame][layer 0 | layer 1 | ...]
    offs = np.concatenate([[0], np.cumsum(4 * ups)])
    relaid = np.concatenate([per_frame[:, offs[l]:offs[l + 1]].reshape(-1) for l in range(len(ups))])
    ref = so.decode(codes, T, relaid)
    pcm = np.concatenate([a for a, _ in chunks])
    assert pcm.shape == ref.shape and np.abs(pcm - ref).max() < 1e-4
    # a following generate() continues the stream where a generate() in its place would have (layer-major)
    pcm2 = r.generate(TEXT, voice=b"zoe", sample=0)
    noise2, _, _ = minstd0_normal(so.noise_len(T), state, saved)
    assert np.abs(pcm2 - so.decode(codes, T, noise2)).max() < 1e-4
    r.close()


def test_audio_arrives_early_and_cancelling_stops(full_model, no_noise):
    full, path = full_model
    r = runner.Runner(path, sample=0)
    ref = r.generate(TEXT, voice=b"zoe", sample=0)   # warm-up, and the reference
    full_tokens = r.last_tokens(1).copy()
    r.generate_chunked(TEXT, chunk_frames=4, voice=b"zoe", sample=0)   # warm-up of the window pass
    t_start = time.monotonic()
    chunks = r.generate_chunked(TEXT, chunk_frames=4, voice=b"zoe", sample=0)
    t_end = time.monotonic()
    assert np.abs(np.concatenate([a for a, _ in chunks]) - ref).max() <= 1e-6
    assert len(chunks) == FRAMES // 4
    assert chunks[0][1] - t_start < 0.5 * (t_end - t_start), "the first chunk must arrive before half of the call's wall time"

    seen = []
    rc = r.generate_chunked(TEXT, chunk_frames=4, voice=b"zoe", sample=0, on_chunk=lambda a, t: seen.append(a) or False)
    assert r.stopped and len(rc) == 1 and len(seen) == 1
    assert 0 < r.last_tokens(1).size < full_tokens.size
    assert np.abs(rc[0][0] - ref[:rc[0][0].size]).max() <= 1e-6
    again = r.generate(TEXT, voice=b"zoe", sample=0)
    assert np.array_equal(again, ref) and np.array_equal(r.last_tokens(1), full_tokens)
    with pytest.raises(runner.RunnerError):
        r.generate_chunked(TEXT, chunk_frames=0, voice=b"zoe", sample=0)
    r.close()
