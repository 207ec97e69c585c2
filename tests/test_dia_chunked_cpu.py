"""Chunked Dia audio on the host: the runner's incremental un-delay rule (dia_undelay through tts_c_dia_final_frames) against
dia_adjust_output_tokens on every prefix of a delayed token stream, and window stitching on the CPU DAC oracle at Dia's nine codebooks."""
import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import hip, runner, synth

NH, AUDIO_VOCAB, MAX_DELAY = 9, 64, 15
EOS, PAD = AUDIO_VOCAB, AUDIO_VOCAB + 1
PIECES = (1, 5, 16, 37)


def _stream(rng, body, n_special):
    """`body` steps of random audio ids with n_special ids >= audio_vocab sprinkled in, then the tail of an end-of-sequence countdown: head 0
    says EOS and tts_c_dia_check_stopping forces EOS / PAD into the delayed heads until it reports the stop"""
    t = rng.integers(0, AUDIO_VOCAB, (body, NH)).astype(np.uint32)
    for _ in range(n_special):
        t[rng.integers(0, body), rng.integers(0, NH)] = AUDIO_VOCAB + rng.integers(0, 4)
    tail, delay, pos = [], -1, body
    ids = rng.integers(0, AUDIO_VOCAB, NH).astype(np.uint32)
    ids[0] = EOS
    while True:
        stop, ids, delay = runner.dia_check_stopping(ids, EOS, PAD, MAX_DELAY, pos, 10 ** 6, delay)
        if stop:
            break
        tail.append(ids.copy())
        ids = np.where(ids >= AUDIO_VOCAB, ids, rng.integers(0, AUDIO_VOCAB, NH)).astype(np.uint32)   # forced ids stay, the others move on
        pos += 1
    assert len(tail) == MAX_DELAY - 1 and any(PAD in r for r in tail)
    return np.concatenate([t, np.stack(tail)])


@pytest.mark.parametrize("seed,body,n_special", [(0, 50, 0), (1, 61, 5), (2, 90, 12)])
def test_incremental_undelay_equals_the_full_rule_on_every_prefix(seed, body, n_special):
    toks = _stream(np.random.default_rng(seed), body, n_special)
    steps = len(toks)
    full = runner.dia_adjust_output_tokens(toks, AUDIO_VOCAB, MAX_DELAY)
    assert 0 < len(full) <= steps - MAX_DELAY
    if n_special:
        assert len(full) < steps - MAX_DELAY, "the sprinkled special ids and the countdown must drop frames"
    prev = 0
    for s in range(1, steps + 1):
        want = runner.dia_adjust_output_tokens(toks[:s], AUDIO_VOCAB, MAX_DELAY)
        assert len(want) >= prev and np.array_equal(want, full[:len(want)]), f"the frames of {s} steps must be a prefix of the whole stream's"
        prev = len(want)
        for piece in PIECES:
            got = runner.dia_final_frames(toks[:s], AUDIO_VOCAB, MAX_DELAY, piece)
            assert got.shape == want.shape and np.array_equal(got, want), f"{s} steps in pieces of {piece}"
    assert np.array_equal(runner.dia_final_frames(toks, AUDIO_VOCAB, MAX_DELAY), full)


def test_streams_shorter_than_max_delay_yield_nothing():
    rng = np.random.default_rng(5)
    for s in range(0, MAX_DELAY + 1):
        toks = rng.integers(0, AUDIO_VOCAB, (s, NH)).astype(np.uint32)
        for piece in (0,) + PIECES:
            assert len(runner.dia_final_frames(toks, AUDIO_VOCAB, MAX_DELAY, piece)) == 0, (s, piece)
    toks = rng.integers(0, AUDIO_VOCAB, (MAX_DELAY + 1, NH)).astype(np.uint32)
    assert len(runner.dia_final_frames(toks, AUDIO_VOCAB, MAX_DELAY, 1)) == 1


def _stitch(dac, codes, h, edges, hop):
    K = len(codes)
    out = []
    for f0, f1 in zip(edges[:-1], edges[1:]):
        w0, w1 = max(0, f0 - h), min(K, f1 + h)
        pcm = dac.decode(codes[w0:w1])
        out.append(pcm[(f0 - w0) * hop:(f1 - w0) * hop])
    return np.concatenate(out)


def test_windows_over_nine_codebooks_stitch_to_the_full_decode():
    model = synth.build_dia(synth.dia_tiny())
    cfg, dcfg = model.cfg, model.dac.cfg
    assert cfg.strides == (4, 2) and dcfg.n_out == NH
    h = hip.dac_halo_frames(hip.desc_for(dcfg))
    assert h == 19
    dac = orc.DacOracle(model.dac)
    K = 3 * h + 11
    codes = np.random.default_rng(3).integers(0, cfg.audio_vocab, (K, NH)).astype(np.uint32)
    full = dac.decode(codes)
    assert full.shape == (K * cfg.hop,)
    # the windows the runner cuts for chunk_frames 16: whole chunks while the right halo exists, then the rest; and odd-sized ones
    for edges in ([0, 16, 32, K], [0, 5, h + 7, h + 8, 2 * h + 9, K]):
        stitched = _stitch(dac, codes, h, edges, cfg.hop)
        assert stitched.shape == full.shape
        assert np.abs(stitched - full).max() <= 1e-6, edges
    short = _stitch(dac, codes, h - 1, [0, 5, h + 7, h + 8, 2 * h + 9, K], cfg.hop)
    assert np.abs(short - full).max() > 0, "h - 1 frames of halo must not be enough"
