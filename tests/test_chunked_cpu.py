"""Chunked audio on the host: the codec halo (tts_hip_dac_halo_frames) against the CPU DAC oracle, window stitching, and the runner's
incremental un-delay rule (tts_c_parler_final_frames) against pattern.undelay."""
import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import hip, runner, synth
from tts_cpp_amd.pattern import undelay

CONFIGS = {"tiny": synth.tiny, "small": synth.small}


def _model(name):
    return synth.build(CONFIGS[name]())


def _frame_diff(a, b, hop):
    """per frame: max |a - b| over its samples"""
    return np.abs(a - b).reshape(-1, hop).max(axis=1)


def _measured_halo(model, K, js):
    cfg = model.cfg
    dac = orc.DacOracle(model)
    rng = np.random.default_rng(7)
    codes = rng.integers(0, cfg.cb_size, (K, cfg.n_out)).astype(np.uint32)
    base = dac.decode(codes)
    reach = 0
    for j in js:
        c2 = codes.copy()
        h = j % cfg.n_out
        c2[j, h] = (c2[j, h] + 1 + rng.integers(0, cfg.cb_size - 1)) % cfg.cb_size
        changed = np.nonzero(_frame_diff(dac.decode(c2), base, cfg.hop) != 0)[0]
        assert changed.size and changed.min() > 0 and changed.max() < K - 1, "the perturbation must stay inside the utterance"
        reach = max(reach, int(j - changed.min()), int(changed.max() - j))
    return reach


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_halo_is_correct_and_tight(name):
    model = _model(name)
    h = hip.dac_halo_frames(hip.desc_for(model.cfg))
    K = 4 * h + 8
    js = [2 * h + 1, 2 * h + 3, 2 * h + 4]
    assert _measured_halo(model, K, js) == h


def test_halo_of_the_dac44k_layout():
    # Parler-Mini's codec (strides 8, 8, 4, 2, paddings ceil(s / 2)); the same layout as synth.small, whose halo the test above measures
    assert hip.dac_halo_frames(hip.desc_for(synth.parler_mini())) == 10
    assert hip.dac_halo_frames(hip.desc_for(synth.tiny())) == 19


def _stitch(dac, codes, h, edges, hop):
    K = len(codes)
    out = []
    for f0, f1 in zip(edges[:-1], edges[1:]):
        w0, w1 = max(0, f0 - h), min(K, f1 + h)
        pcm = dac.decode(codes[w0:w1])
        out.append(pcm[(f0 - w0) * hop:(f1 - w0) * hop])
    return np.concatenate(out)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_windows_with_the_halo_stitch_to_the_full_decode(name):
    model = _model(name)
    cfg = model.cfg
    h = hip.dac_halo_frames(hip.desc_for(cfg))
    dac = orc.DacOracle(model)
    K = 3 * h + 11
    codes = np.random.default_rng(3).integers(0, cfg.cb_size, (K, cfg.n_out)).astype(np.uint32)
    full = dac.decode(codes)
    edges = [0, 5, h + 7, 2 * h + 9, K]   # a window clipped at 0, interior ones, one clipped at K
    stitched = _stitch(dac, codes, h, edges, cfg.hop)
    assert stitched.shape == full.shape
    assert np.abs(stitched - full).max() <= 1e-6
    short = _stitch(dac, codes, h - 1, edges, cfg.hop)
    assert np.abs(short - full).max() > 0, "h - 1 frames of halo must not be enough"


def _delayed_stream(rng, steps, nh, audio_vocab, inject):
    t = rng.integers(0, audio_vocab, (steps, nh)).astype(np.uint32)
    for s in inject:   # non-audio ids (EOS / BOS / pad) mid-stream and at the end
        t[s, rng.integers(0, nh)] = audio_vocab + rng.integers(0, 3)
    return t


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_incremental_undelay_is_a_prefix_of_the_full_one(seed):
    rng = np.random.default_rng(seed)
    nh, audio_vocab = (9, 1024) if seed else (4, 64)
    steps = 60
    inject = sorted(set(rng.integers(0, steps, 6).tolist()) | {steps - 1, steps - 2})
    toks = _delayed_stream(rng, steps, nh, audio_vocab, inject)
    full = undelay(toks, audio_vocab)
    prev = 0
    for S in range(0, steps + 1):
        part = runner.parler_final_frames(toks[:S], audio_vocab, finished=False)
        assert part.shape[1] == nh and len(part) >= prev
        assert np.array_equal(part, full[:len(part)]), f"after {S} steps"
        prev = len(part)
        # a frame is final once its last delayed head exists: every frame < S - nh + 1 has been judged
        done = runner.parler_final_frames(toks[:S], audio_vocab, finished=True)
        assert np.array_equal(done, undelay(toks[:S], audio_vocab)), f"finished after {S} steps"
    assert np.array_equal(runner.parler_final_frames(toks, audio_vocab, finished=True), full)
