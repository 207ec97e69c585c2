"""orpheus_runner with more than 64 cache slots: the session and generate_batch follow max_seqs up to 256, above that the runner clamps and says so."""
import os

import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import gguf, synth

pytestmark = pytest.mark.gpu

# texts whose greedy generation stays inside the audio ids with the synthetic weights (tests/test_gpu_orpheus_stream.py generates them one by one)
TEXTS = ["hello the zebra", "a zebra", "the quick hello of the zebra there", "hello", "the zebra there hello", "a quick zebra", "of the hello",
         "zebra zebra the quick", "there a hello of zoe"]


@pytest.fixture(scope="module")
def full():
    return synth.SynthOrpheusFull(max_gen=28)


@pytest.fixture(scope="module")
def orpheus_gguf(full, tmp_path_factory):
    return full.write_gguf(str(tmp_path_factory.mktemp("orpheus_many_rows") / "orpheus.gguf"))


@pytest.fixture(scope="module")
def no_noise():
    old = os.environ.get("TTS_SNAC_NO_NOISE")
    os.environ["TTS_SNAC_NO_NOISE"] = "1"
    yield
    if old is None:
        del os.environ["TTS_SNAC_NO_NOISE"]
    else:
        os.environ["TTS_SNAC_NO_NOISE"] = old


def test_runner_with_96_slots_streams_100_texts_and_batches_70(full, orpheus_gguf, no_noise):
    """Runner(max_seqs=96): stream_capacity is 96; generate_stream answers 100 texts (the session refills four freed slots) with non-empty audio, equal
    for equal texts; generate_batch of 70 utterances (the live count crosses 64 downwards as they end) leaves ids that are the oracle's arg-max up to
    the bound when the oracle is teacher-forced with them."""
    import tokenizer_oracle
    from tts_cpp_amd import runner
    many = runner.Runner(orpheus_gguf, sample=0, max_seqs=96)
    assert many.stream_capacity() == 96
    texts = [TEXTS[i % len(TEXTS)] for i in range(100)]
    got = many.generate_stream(texts, voice=b"zoe", sample=0)
    assert len(got) == 100 and all(a.size > 0 for a in got)
    one = many.generate(TEXTS[0], voice=b"zoe", sample=0)
    assert one.shape == got[0].shape == got[len(TEXTS)].shape
    many.generate_batch(texts[:70], voice=b"zoe", sample=0)
    tok = tokenizer_oracle.BpeOracle(full.vocab_tokens, full.merges)
    o = orc.OrpheusOracle(full.orpheus, act_mode=1)
    tol = {gguf.F32: 2e-4, gguf.F16: 2e-3}.get(full.orpheus.cfg.weight_type, 3e-2)
    for u in (0, 37, 69):
        ids = many.last_tokens(16 + u).tolist()
        assert 0 < len(ids) <= full.max_gen
        prompt = full.specials["pre"] + tok.tokenize("zoe: " + texts[u]) + full.specials["app"]
        ref = o.decode(prompt, 0)
        for s, t in enumerate(ids):
            assert ref[t] >= ref.max() - 2 * tol * np.abs(ref).max(), (u, s, t, int(ref.argmax()))
            if s + 1 < len(ids):
                ref = o.decode([t], len(prompt) + s)
    many.close()


def test_runner_clamps_300_slots_to_256_and_says_so(orpheus_gguf, no_noise, capfd):
    from tts_cpp_amd import runner
    capfd.readouterr()
    r = runner.Runner(orpheus_gguf, sample=0, max_seqs=300)
    err = capfd.readouterr().err
    assert r.stream_capacity() == 256
    lines = [ln for ln in err.splitlines() if "max_seqs" in ln]
    assert len(lines) == 1 and "300" in lines[0] and "256" in lines[0], err
    r.close()
    capfd.readouterr()
    r = runner.Runner(orpheus_gguf, sample=0, max_seqs=64)      # no clamp, no line
    assert r.stream_capacity() == 64 and "max_seqs" not in capfd.readouterr().err
    r.close()
