"""A second, larger mixed session on a context that has already served a smaller one: the per-slot records, penalty tables, uniforms and token
buffers must grow (grow_dev / grow_bufs in csrc/shim_internal.h), and every captured graph that held an old address must be dropped.  Per
model the same utterance, sampled with a repetition penalty, through session 2 of a context that ran session 1 first and through session 2
of a fresh context: the ids must be equal, exactly (same kernels, same device).  The utterance sits in the last slot of session 2, which
session 1 did not have."""
import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

SETTING = dict(top_k=12, top_p=0.9, temperature=0.9, repetition_penalty=1.3)
SMALL, LARGE = (2, 8), (3, 12)   # slots x steps of the two sessions


def _finish(eng, n_steps):
    """run the session's one utterance to its end -> its ids"""
    for _ in range(8):
        fin = eng.stream_run(n_steps)
        if fin:
            assert len(fin) == 1
            return eng.stream_collect(*fin[0])
    raise AssertionError("the utterance did not finish")


def _compare(first_then_second, second_only):
    got, alone = first_then_second, second_only
    assert len(alone) > 0 and len(np.unique(alone)) > 1, "the utterance must have produced ids"
    assert got.shape == alone.shape and np.array_equal(got, alone)


def test_parler_second_larger_mixed_session_equals_a_fresh_context():
    cfg = synth.small(weight_type=gguf.F16, ctx=40, max_gen=40)
    model = synth.build(cfg)
    rng = np.random.default_rng(31)
    prompt = rng.integers(3, cfg.prompt_vocab, 7).astype(np.uint32)
    uni = rng.random((1, LARGE[1], cfg.n_out), dtype=np.float32)

    def session(eng, slots, steps, slot):
        eng.stream_begin_mixed(slots, steps)
        eng.stream_admit_mixed([slot], [prompt], [SETTING], uni[:, :steps])
        ids = _finish(eng, steps)
        eng.stream_end()
        assert len(ids) == steps   # random weights: the budget ends it
        return ids

    def engine():
        eng = hip.HipEngine(cfg, max_seqs=LARGE[0] + 1, kv_positions=40, flags=hip.FLAG_NO_DAC)
        eng.load(model)
        return eng

    eng = engine()
    session(eng, *SMALL, slot=SMALL[0] - 1)
    got = session(eng, *LARGE, slot=LARGE[0] - 1)
    again = session(eng, *LARGE, slot=LARGE[0] - 1)   # nothing grows now: the graphs of the last session are replayed
    # The uniforms buffer alone moves: a one-shot selection over 64 rows needs more draws (64 x heads) than the session's block
    # ((12 + 1) x 4 x heads).  The next session has the same slots, steps and ids, so nothing but the moved buffer drops the captured sampled
    # step; replayed, it would read the draws from the freed address
    rows = 64
    assert rows * cfg.n_out > (LARGE[1] + 1) * (LARGE[0] + 1) * cfg.n_out
    eng.sample_logits(rng.standard_normal((rows, cfg.n_out, cfg.out_vocab)).astype(np.float32), rng.random((rows, cfg.n_out), dtype=np.float32), top_k=8)
    moved = session(eng, *LARGE, slot=LARGE[0] - 1)
    eng.close()
    fresh = engine()
    alone = session(fresh, *LARGE, slot=LARGE[0] - 1)
    fresh.close()
    _compare(got, alone)
    _compare(again, alone)
    _compare(moved, alone)


def test_dia_second_larger_mixed_session_equals_a_fresh_context():
    model = synth.build_dia(synth.dia_tiny(weight_type=gguf.F16), suppress_special=True)
    cfg = model.cfg
    args = dict(delay_pattern=[0, 8, 9, 10, 11, 12, 13, 14, 15], bos=cfg.bos, eos=cfg.eos, pad=cfg.pad, max_delay=cfg.max_delay)
    tokens, sentence_len = orc.dia_tokenize("[S1] the same one twice.", cfg.max_ctx)
    gens = (16, 24)
    assert cfg.max_delay < gens[0] < gens[1] <= cfg.max_gen
    uni = np.random.default_rng(32).random((1, gens[1], cfg.n_out), dtype=np.float32)

    def session(eng, max_gen, slot):
        eng.stream_begin_mixed(3, max_gen, **args)
        eng.stream_admit_mixed([slot], [tokens], [sentence_len], [SETTING], budgets=[max_gen], uniforms=uni[:, :max_gen])
        ids = _finish(eng, max_gen)
        eng.stream_end()
        assert len(ids) == max_gen - 1   # no EOS in this model
        return ids

    def engine():
        eng = hip.DiaEngine(cfg, max_utterances=3)
        eng.load(model)
        return eng

    eng = engine()
    session(eng, gens[0], slot=1)
    got = session(eng, gens[1], slot=2)
    eng.close()
    fresh = engine()
    alone = session(fresh, gens[1], slot=2)
    fresh.close()
    _compare(got, alone)


def test_orpheus_second_larger_mixed_session_equals_a_fresh_context():
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=gguf.F16))
    cfg = model.cfg
    rng = np.random.default_rng(33)
    prompt = rng.integers(0, cfg.vocab, 6).astype(np.uint32)
    uni = rng.random((1, LARGE[1]), dtype=np.float32)
    never = cfg.vocab + 7

    def session(eng, slots, max_new, slot):
        eng.stream_begin_mixed(slots, max_new, never)
        eng.stream_admit_mixed([slot], [prompt], [dict(SETTING)], uni[:, :max_new])
        ids = _finish(eng, max_new)
        eng.stream_end()
        assert len(ids) == max_new
        return ids

    def engine():
        eng = hip.OrpheusEngine(cfg, max_seqs=LARGE[0])
        eng.load(model)
        return eng

    eng = engine()
    session(eng, *SMALL, slot=SMALL[0] - 1)
    got = session(eng, *LARGE, slot=LARGE[0] - 1)
    eng.close()
    fresh = engine()
    alone = session(fresh, *LARGE, slot=LARGE[0] - 1)
    fresh.close()
    _compare(got, alone)
