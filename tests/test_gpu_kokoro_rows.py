"""GPU: the Kokoro duration pass for up to 8 clauses in one context (tts_hip_kokoro_durations_batch: kk_lstm_rows_kernel and the clause-aware
kernels of csrc/kokoro_kernels.h).  The contract is bit-equality: every clause's lengths and duration states are what tts_hip_kokoro_durations gives
for that clause alone on the same engine, under the same tune keys."""
import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import hip, synth

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def clauses(cfg, counts, seed):
    """token lists of the given lengths (bos, ids, eos)"""
    rng = np.random.default_rng(seed)
    return [np.concatenate([[0], rng.integers(1, cfg.vocab, n - 2), [0]]).astype(np.uint32) for n in counts]


def assert_batch_equals_alone(eng, toks, voices):
    alone = [eng.durations(t, v) for t, v in zip(toks, voices)]
    got = eng.durations_batch(toks, voices)
    assert len(got) == len(alone)
    for b, ((lens, hid), (ref_lens, ref_hid)) in enumerate(zip(got, alone)):
        assert lens.shape == ref_lens.shape and hid.shape == ref_hid.shape, b
        assert np.array_equal(lens, ref_lens), (b, "lens")
        assert np.array_equal(hid, ref_hid), (b, "hidden", float(np.abs(hid - ref_hid).max()))
    return got, alone


def test_tiny_model_mixed_lengths_and_voices_in_the_callers_order():
    """hid 16 (CP 4).  Equal lengths, the 3-token minimum, both sides of the 32-row boundary between the two projection kernels, two voices; unsorted."""
    model = synth.build_kokoro(synth.kokoro_tiny(max_ctx=160))
    eng = hip.KokoroEngine(model)
    counts = [5, 34, 3, 32, 31, 33, 5, 4]
    toks = clauses(model.cfg, counts, 1)
    voices = ["af_test", "bm_test"] * 4
    got, _ = assert_batch_equals_alone(eng, toks, voices)
    assert [g[0].size for g in got] == counts
    # the voice matters (so the per-clause style reached the kernels): the same clause under the other voice gives other states
    other = eng.durations_batch(toks, voices[::-1])
    assert not np.array_equal(other[1][1], got[1][1])
    eng.close()


@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_tiny_model_long_recurrence(D):
    """kk_lstm_rows_kernel<CP> for CP = 4, 8, 16, 32 (1, 2, 4, 8 workgroups per direction) over 130 steps: the step tag and the two-parity buffer wrap
    65 times, and sequences drop out at both parities (after 3 and after 129 steps) while another runs on."""
    model = synth.build_kokoro(synth.kokoro_tiny(max_ctx=160, dp_hidden=D))
    eng = hip.KokoroEngine(model)
    toks = clauses(model.cfg, [130, 129, 3], 2)
    assert_batch_equals_alone(eng, toks, ["af_test", "bm_test", "af_test"])
    eng.close()


def test_batch_sizes_and_refused_calls():
    model = synth.build_kokoro(synth.kokoro_tiny(max_ctx=160))
    cfg = model.cfg
    eng = hip.KokoroEngine(model)
    assert_batch_equals_alone(eng, clauses(cfg, [9], 3), ["af_test"])
    assert_batch_equals_alone(eng, clauses(cfg, [17, 17], 4), ["af_test", "af_test"])
    eight = clauses(cfg, [12, 40, 7, 40, 3, 21, 36, 8], 5)
    assert_batch_equals_alone(eng, eight, ["bm_test"] * 8)
    ok = clauses(cfg, [6, 5], 6)
    bad_token = [ok[0].copy(), ok[1].copy()]
    bad_token[1][2] = cfg.vocab
    for toks, voices in ((eight + ok[:1], ["af_test"] * 9),                      # B = 9
                         ([], []),                                                # B = 0
                         ([ok[0], ok[1][:2]], ["af_test"] * 2),                   # n = 2
                         (bad_token, ["af_test"] * 2),                            # token >= vocabulary
                         (ok, ["af_test", "nobody"])):                            # unknown voice
        with pytest.raises(hip.HipError):
            eng.durations_batch(toks, voices)
        assert_batch_equals_alone(eng, ok, ["af_test", "bm_test"])               # the context is still usable
    eng.close()


COUNTS_82M = [77, 40, 31, 12, 3]


@pytest.fixture(scope="module")
def m82():
    """the 82M-width model, five clauses and what the default engine gives for each alone (shared, read-only)"""
    model = synth.build_kokoro(synth.kokoro_82m())
    toks = clauses(model.cfg, COUNTS_82M, 82)
    voices = [model.cfg.voices[b % 2] for b in range(len(toks))]
    eng = hip.KokoroEngine(model)
    got, alone = assert_batch_equals_alone(eng, toks, voices)
    eng.close()
    return model, toks, voices, got


def test_82m_widths_equal_alone_and_match_the_oracle(m82):
    """hid 256 (CP 64), head size 64 (the LDS attention): 77 rows = two key chunks with a ragged last workgroup; 163 rows in all, so 64-row MFMA tiles hold
    rows of two clauses; 31 / 12 / 3 rows go the wave-per-output way.  Bit-equality is asserted where the fixture is built."""
    model, toks, voices, got = m82
    o = orc.KokoroOracle(model)
    for b, (t, v) in enumerate(zip(toks, voices)):
        ref_lens, ref_hid = o.durations(t, v)
        print(f"clause {b} ({t.size} rows): duration states vs oracle {relerr(got[b][1], ref_hid):.2e}")
        assert np.array_equal(got[b][0], ref_lens), b
        assert relerr(got[b][1], ref_hid) < 2e-3, b      # the bound of tests/test_gpu_kokoro.py at these widths (fp16-table GELU on both sides)


@pytest.mark.parametrize("tune", [{"kokoro_lstm_split": 0}, {"kokoro_mfma": 0}, {"kokoro_attn_lds": 0}], ids=["one_workgroup_lstm", "plain_kernels", "row_walking_attention"])
def test_82m_widths_fallbacks(m82, tune):
    """the same five clauses under each fallback key: bit-equal to the per-clause calls under the same key"""
    model, toks, voices, default = m82
    eng = hip.KokoroEngine(model, tune=tune)
    got, _ = assert_batch_equals_alone(eng, toks, voices)
    eng.close()
    if "kokoro_lstm_split" in tune:   # another summation order of the recurrent dot products: the key reached the batch pass
        assert not np.array_equal(got[0][1], default[0][1])
        assert relerr(got[0][1], default[0][1]) < 2e-3


TEXTS = ["abc de fgh", "abcdefgh abcdefgh. abcdefgh abcdefgh! abc", "a", "hgf ed cba hgf ed. cba hgf ed cba hgf", "de de de de",
         "fgh abc de fgh abc de? fgh abc de fgh a", "b"]


@pytest.mark.parametrize("rows", [8, 0])
def test_runner_generate_batch_with_and_without_duration_groups(tmp_path, monkeypatch, capfd, rows):
    """kokoro_runner::generate_batch with TTS_KOKORO_ROWS = 8 (durations first, 11 clauses in two groups, then the generation graphs with every noise
    stretch known) and = 0 (durations per clause): audio bit for bit that of generate() calls in a row, and the noise engine ends where they leave it."""
    from tts_cpp_amd import gguf, runner
    model = synth.build_kokoro(synth.kokoro_tiny())
    path = model.write_gguf(str(tmp_path / "kokoro.gguf"))
    vocab = gguf.Reader(path).kv["tokenizer.ggml.tokens"]
    assert sum(len(runner.kokoro_chunks(vocab, t, model.cfg.max_ctx)) for t in TEXTS) == 11
    seq = runner.Runner(path, voice=b"af_test")
    want = [seq.generate(t, voice=b"af_test") for t in TEXTS]
    after = seq.generate("abc", voice=b"af_test")
    seq.close()
    monkeypatch.setenv("TTS_KOKORO_ROWS", str(rows))
    monkeypatch.setenv("TTS_KOKORO_BATCH_TRACE", "1")
    bat = runner.Runner(path, voice=b"af_test", max_seqs=3)
    capfd.readouterr()
    got = bat.generate_batch(TEXTS, voice=b"af_test")
    trace = capfd.readouterr().err
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), u
    assert np.array_equal(bat.generate("abc", voice=b"af_test"), after)
    bat.close()
    # the switch was read: two duration groups (8 + 3 clauses) with rows on, none without
    assert ("group 0 (8 clauses" in trace and "group 1 (3 clauses" in trace) == (rows == 8), trace
    assert ("group" in trace) == (rows == 8), trace
