"""GPU: chunked audio.  Codec windows (tts_hip_dac_decode_windows) against the whole-utterance decode, and the runner's chunked generation
(generate_chunked / generate_batch_chunked) against generate() / generate_batch() in every loop mode."""
import os
import time

import numpy as np
import pytest

from tts_cpp_amd import gguf, hip, runner, synth

pytestmark = pytest.mark.gpu

TEXT = "the quick brown fox"
TEXTS = ["the quick brown fox", "hello", "a much longer sentence with several more words in it"]


def _windows(K, h, edges):
    return [(max(0, f0 - h), min(K, f1 + h), f0, f1) for f0, f1 in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("layout,dac_f16", [("small", False), ("small", True), ("dac44k", False), ("dac44k", True)])
def test_windows_equal_the_full_decode(layout, dac_f16):
    if layout == "small":
        cfg = synth.small(weight_type=gguf.F32, dac_f16=dac_f16)
    else:   # DAC 44 kHz dims (1536 -> 96 channels, x512); the decoder part is irrelevant here
        cfg = synth.parler_mini(layers=1, prompt_vocab=64, ctx=64, dac_f16=dac_f16)
    model = synth.build(cfg)
    eng = hip.HipEngine(model.cfg, flags=hip.FLAG_NO_PARLER)
    eng.load(model)
    h = eng.dac_halo_frames()
    assert h == 10
    K = 70
    codes = np.random.default_rng(11).integers(0, cfg.cb_size, (K, cfg.n_out)).astype(np.uint32)
    full = eng.dac_decode(codes)
    hop = model.cfg.hop
    edges = [0, 3, 19, 20, 47, K]   # clipped at 0, interior (one of a single frame), clipped at K
    ws = _windows(K, h, edges)
    got = eng.dac_decode_windows([(codes[w0:w1], f0 - w0, f1 - w0) for w0, w1, f0, f1 in ws])
    for (w0, w1, f0, f1), g in zip(ws, got):
        assert g.shape == ((f1 - f0) * hop,)
        assert np.abs(g - full[f0 * hop:f1 * hop]).max() <= 1e-6, f"window [{w0}, {w1}) keeping [{f0}, {f1})"
    assert np.array_equal(np.concatenate(got), full) or np.abs(np.concatenate(got) - full).max() <= 1e-6
    eng.close()


@pytest.fixture(scope="module")
def tiny_runner(tmp_path_factory):
    model = synth.build(synth.tiny(weight_type=gguf.F16))
    path = model.write_gguf(str(tmp_path_factory.mktemp("chunked") / "m.gguf"))
    os.environ["TTS_HIP_MAX_SEQS"] = "4"
    try:
        r = runner.Runner(path, sample=0)
    finally:
        del os.environ["TTS_HIP_MAX_SEQS"]
    yield model, r
    r.close()


MODES = [dict(sample=0), dict(sample=1, top_k=20, temperature=0.9, seed=1234)]


@pytest.mark.parametrize("host_loop", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_chunks_equal_generate(tiny_runner, host_loop, mode):
    model, r = tiny_runner
    hop = model.cfg.hop
    cfg = MODES[mode]
    if host_loop:
        os.environ["TTS_HOST_LOOP"] = "1"
    try:
        ref = r.generate(TEXT, **cfg)
        t0, t1 = r.last_tokens(0).copy(), r.last_tokens(1).copy()
        assert ref.size > 30 * hop
        for cf in (1, 7, 32, 10000):
            chunks = r.generate_chunked(TEXT, chunk_frames=cf, **cfg)
            assert not r.stopped
            sizes = [a.size for a, _ in chunks]
            assert all(s % hop == 0 and 0 < s <= cf * hop for s in sizes)
            assert all(s == cf * hop for s in sizes[:-1]), "only the last chunk may be short"
            pcm = np.concatenate([a for a, _ in chunks])
            assert pcm.size == ref.size, f"chunk_frames {cf}"
            assert np.abs(pcm - ref).max() <= 1e-6, f"chunk_frames {cf}"
            assert np.array_equal(r.last_tokens(0), t0) and np.array_equal(r.last_tokens(1), t1)
            stamps = [t for _, t in chunks]
            assert stamps == sorted(stamps)
            if cf == 10000:
                assert len(chunks) == 1
    finally:
        os.environ.pop("TTS_HOST_LOOP", None)


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_chunks_equal_generate_batch(tiny_runner, mode):
    model, r = tiny_runner
    cfg = MODES[mode]
    ref = r.generate_batch(TEXTS, **cfg)
    got = r.generate_batch_chunked(TEXTS, chunk_frames=16, **cfg)
    assert not r.stopped
    per = {i: [] for i in range(len(TEXTS))}
    for utt, a, t in got:
        per[utt].append((a, t))
    for i, b in enumerate(ref):
        pcm = np.concatenate([a for a, _ in per[i]])
        assert pcm.size == b.size and b.size > 0
        assert np.abs(pcm - b).max() <= 1e-6, f"utterance {i}"
        stamps = [t for _, t in per[i]]
        assert stamps == sorted(stamps)


def test_audio_arrives_early_and_cancelling_stops(tmp_path):
    # 256 audio steps: max_generation = prompt + 256 (random weights never emit EOS)
    probe = synth.build(synth.small(weight_type=gguf.F16))
    path = probe.write_gguf(str(tmp_path / "p.gguf"))
    r = runner.Runner(path, sample=0)
    n_prompt = len(r.tokenize("hello there"))   # ids + EOS
    r.close()
    model = synth.build(synth.small(weight_type=gguf.F16, max_gen=256 + n_prompt))
    path = model.write_gguf(str(tmp_path / "m.gguf"))
    r = runner.Runner(path, sample=0)
    ref = r.generate("hello there")   # warm-up, and the reference
    full_tokens = r.last_tokens(1).copy()
    assert full_tokens.size == 256 * model.cfg.n_out
    t_start = time.monotonic()
    chunks = r.generate_chunked("hello there", chunk_frames=32)
    t_end = time.monotonic()
    assert np.abs(np.concatenate([a for a, _ in chunks]) - ref).max() <= 1e-6
    assert len(chunks) > 2
    assert chunks[0][1] - t_start < 0.5 * (t_end - t_start), "the first chunk must arrive before half of the call's wall time"

    seen = []
    rc = r.generate_chunked("hello there", chunk_frames=32, on_chunk=lambda a, t: seen.append(a) or False)
    assert r.stopped and len(rc) == 1 and len(seen) == 1
    assert 0 < r.last_tokens(1).size < full_tokens.size
    assert np.abs(rc[0][0] - ref[:rc[0][0].size]).max() <= 1e-6
    again = r.generate("hello there")
    assert np.array_equal(again, ref) and np.array_equal(r.last_tokens(1), full_tokens)
    r.close()


def test_chunk_frames_zero_is_an_error(tiny_runner):
    _, r = tiny_runner
    with pytest.raises(runner.RunnerError):
        r.generate_chunked(TEXT, chunk_frames=0)
