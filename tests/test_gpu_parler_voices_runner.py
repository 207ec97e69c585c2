"""Named voice descriptions through the C++ runner and the device pool (tts_generation_runner::add_voice, generation_configuration::voice).
A tiny Parler GGUF and a tiny T5 encoder GGUF, as tests/test_gpu_runner.py builds them for update_conditional_prompt.
  add_voice / list_voices; generate(text, voice=...) against the engine-level yardstick of tests/test_gpu_parler_voices.py: a context whose own
  description is that voice's T5 output, the cross-attention a launch of its own (tune cross_fold = 0); generate_batch with one voice;
  generate_stream with a voice and a sampler per text through one session; the continuous pool; an unknown voice."""
import numpy as np
import pytest

from tts_cpp_amd import gguf, hip, runner, synth

pytestmark = pytest.mark.gpu

DESCS = {"a": "calm low", "b": "bright fast clear"}
TEXTS = ["hello there", "good morning to you", "hi", "one two three", "so long", "yes", "well well well", "no"]
SAMPLERS = [dict(sample=0), dict(sample=1, seed=5, top_k=20, temperature=0.9, repetition_penalty=1.1)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("parler_voices")
    cfg = synth.tiny(weight_type=gguf.F32)
    model = synth.build(cfg)
    t5 = synth.build_t5(synth.t5_tiny(vocab=cfg.prompt_vocab, output_size=cfg.hidden))
    return dict(cfg=cfg, model=model, t5=t5, path=model.write_gguf(str(d / "m.gguf")), t5_path=t5.write_gguf(str(d / "t5.gguf")))


def _with_voices(f, **kw):
    r = runner.Runner(f["path"], **kw)
    for name, desc in DESCS.items():
        r.add_voice(name, f["t5_path"], desc)
    return r


def _encoding(f, ids):
    t5 = hip.T5Engine(f["t5"].cfg)
    t5.load(f["t5"])
    enc = t5.encode(ids)
    t5.close()
    return enc


def _engine_audio(f, enc, prompts):
    """the yardstick: greedy lock-step generation of `prompts` on a context whose own description is `enc` (None: the model file's), unfolded; per
    utterance the still-delayed ids and the PCM of their un-delayed frames"""
    cfg = f["cfg"]
    eng = hip.HipEngine(cfg, max_seqs=len(prompts), tune={"cross_fold": 0})
    eng.load(f["model"])
    if enc is not None:
        eng.set_text_encoding(enc)
    eng.prefill_batch(prompts)
    lens = np.array([len(p) for p in prompts])
    n_steps = int(cfg.max_gen - lens.min())
    toks, done = eng.generate_greedy(lens, n_steps)
    out = []
    for i in range(len(prompts)):
        steps = min(int(done[i]) if done[i] else n_steps, int(cfg.max_gen - lens[i]))
        ids = toks[:steps, i]
        frames = runner.parler_final_frames(ids, cfg.audio_vocab, True)
        out.append((ids.copy(), eng.dac_decode(frames) if len(frames) else np.zeros(0, dtype=np.float32)))
    eng.close()
    return out


def test_add_voice_list_voices_and_generate_with_a_voice(files):
    f = files
    cfg = f["cfg"]
    plain = runner.Runner(f["path"], sample=0)
    base = plain.generate(TEXTS[0])
    with pytest.raises(runner.RunnerError, match="unknown voice 'a'.*none"):
        plain.generate(TEXTS[0], sample=0, voice="a")
    assert np.array_equal(plain.generate(TEXTS[0]), base)
    plain.close()

    r = runner.Runner(f["path"], sample=0, max_seqs=4)
    assert r.list_voices() == []
    r.add_voice("a", f["t5_path"], DESCS["a"])
    ids_a = r.last_tokens(2).copy()
    r.add_voice("b", f["t5_path"], DESCS["b"])
    ids_b = r.last_tokens(2).copy()
    assert r.list_voices() == ["a", "b"]
    assert 1 < len(ids_a) <= 32 and 1 < len(ids_b) <= 32 and ids_a[-1] == 1 and not np.array_equal(ids_a, ids_b)
    assert np.array_equal(r.generate(TEXTS[0]), base), "the runner's own description is untouched"
    prompt = r.tokenize(TEXTS[0])
    got = {}
    for name, ids in (("a", ids_a), ("b", ids_b)):
        audio = r.generate(TEXTS[0], sample=0, voice=name)
        want_ids, want_pcm = _engine_audio(f, _encoding(f, ids), [prompt])[0]
        assert np.array_equal(r.last_tokens(1).reshape(-1, cfg.n_out), want_ids), name
        assert audio.size > 0 and np.array_equal(audio, want_pcm), name
        got[name] = audio
    assert not np.array_equal(got["a"], got["b"]) and not np.array_equal(got["a"], base)
    # chunked audio takes the voice too
    chunks = r.generate_chunked(TEXTS[0], chunk_frames=8, sample=0, voice="a")
    assert np.array_equal(np.concatenate([c[0] if isinstance(c, tuple) else c for c in chunks]), got["a"])
    # generate_batch with one voice: the lock-step yardstick at the same row count
    texts = TEXTS[:3]
    batch = r.generate_batch(texts, sample=0, voice="b")
    want = _engine_audio(f, _encoding(f, ids_b), [r.tokenize(t) for t in texts])
    for i in range(3):
        assert batch[i].size > 0 and np.array_equal(batch[i], want[i][1]), i
    # a known name is replaced; a description beyond 32 tokens is refused and names the limit; the list is unchanged
    r.add_voice("a", f["t5_path"], DESCS["b"])
    assert r.list_voices() == ["a", "b"] and np.array_equal(r.generate(TEXTS[0], sample=0, voice="a"), got["b"])
    with pytest.raises(runner.RunnerError, match="at most 32"):
        r.add_voice("long", f["t5_path"], "calm low bright fast calm low bright fast")   # more than 32 tokens, within the encoder's 64
    assert r.list_voices() == ["a", "b"]
    # an unknown voice aborts and lists the names; the runner still generates
    for call in (lambda: r.generate(TEXTS[0], sample=0, voice="nobody"), lambda: r.generate_batch(texts, sample=0, voice="nobody"),
                 lambda: r.generate_stream(texts, configs=[dict(sample=0, voice=""), dict(sample=0, voice="nobody"), dict(sample=0, voice="b")])):
        with pytest.raises(runner.RunnerError, match="unknown voice 'nobody'.*a, b"):
            call()
    assert np.array_equal(r.generate(TEXTS[0], sample=0, voice="b"), got["b"]) and np.array_equal(r.generate(TEXTS[0]), base)
    # a runner on the same weight arena has a bank of its own
    sib = runner.Runner(f["path"], sample=0, share_with=r)
    assert sib.list_voices() == [] and np.array_equal(sib.generate(TEXTS[0]), base)
    with pytest.raises(runner.RunnerError, match="unknown voice 'b'"):
        sib.generate(TEXTS[0], sample=0, voice="b")
    sib.add_voice("b", f["t5_path"], DESCS["a"])
    assert np.array_equal(sib.generate(TEXTS[0], sample=0, voice="b"), got["a"])
    assert np.array_equal(r.generate(TEXTS[0], sample=0, voice="b"), got["b"])
    sib.close()
    r.close()


def test_generate_stream_with_a_voice_and_a_sampler_per_text(files):
    """8 texts through 3 rows, voices "", "a", "b" and two samplers in turn: each utterance's ids and PCM are those of its own generate() with the
    same configuration on the same runner"""
    f = files
    r = _with_voices(f, sample=0, max_seqs=4)
    configs = [dict(SAMPLERS[i % 2], voice=["", "a", "b"][i % 3]) for i in range(len(TEXTS))]
    got = r.generate_stream(TEXTS, configs=configs)
    assert len(got) == len(TEXTS)
    bad = []
    for i, (t, c) in enumerate(zip(TEXTS, configs)):
        alone = r.generate(t, **c)
        print(i, c, got[i].size, alone.size, np.array_equal(got[i], alone))
        if not np.array_equal(got[i], alone):
            bad.append(i)
    assert not bad, bad
    assert len({g.tobytes() for g in got}) == len(TEXTS)
    r.close()


def test_continuous_pool_answers_three_voices_out_of_one_session(files):
    """add_voice through the pool, then six requests over three voices: one session serves them (no more sessions than for six requests with one
    voice), each with the audio of generate() with that voice"""
    f = files
    r = _with_voices(f, sample=0, max_seqs=4)
    voices = ["", "a", "b", "b", "", "a"]
    want = [r.generate(t, sample=0, voice=v) for t, v in zip(TEXTS, voices)]
    r.close()

    def serve(vs):
        pool = runner.Pool(f["path"], n_workers=1, max_batch=8, continuous=True, text_encoder_path=f["t5_path"], sample=0)
        for name, desc in DESCS.items():
            audio, bs, wk, err = pool.wait(pool.add_voice(name, desc), 60000)
            assert err == "" and audio.size == 0, err
        ids = [pool.submit(t, sample=0, voice=v) for t, v in zip(TEXTS, vs)]
        out = [pool.wait(i, 60000) for i in ids]
        bad = pool.wait(pool.submit("hello", sample=0, voice="nobody"), 60000)
        assert bad[0].size == 0 and "unknown voice 'nobody'" in bad[3] and "a, b" in bad[3]
        again = pool.wait(pool.submit(TEXTS[1], sample=0, voice="a"), 60000)
        st = pool.stats()
        pool.close()
        return out, again, st

    _, _, st_same = serve([""] * 6)
    out, again, st = serve(voices)
    for i, (audio, bs, wk, err) in enumerate(out):
        print(i, voices[i], audio.size, want[i].size, np.array_equal(audio, want[i]))
    assert all(err == "" for _, _, _, err in out)
    assert st["batches"] <= st_same["batches"], (st, st_same)
    assert [i for i, o in enumerate(out) if not np.array_equal(o[0], want[i])] == []
    assert again[3] == "" and np.array_equal(again[0], want[1])
