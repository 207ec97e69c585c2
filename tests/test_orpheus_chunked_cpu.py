"""Chunked Orpheus audio on the host: the SNAC halo (tts_hip_snac_halo_frames) against the CPU SNAC oracle — measured by perturbing one
code of each level and one noise sample of each layer — and window stitching with h and with h - 1 frames of halo."""
import numpy as np

import oracle as orc
from tts_cpp_amd import hip, synth

FRAME_TOKENS = 4   # one frame = one group of 7 Orpheus ids = 4 finest-level tokens


def _codes(cfg, K, seed):
    """K frames of random codes, one array per level (K, 2K, 4K ids)"""
    rng = np.random.default_rng(seed)
    T = FRAME_TOKENS * K
    return [rng.integers(0, cfg.cb_size, T // r).astype(np.uint32) for r in cfg.repeats]


def _flat(levels, f0=None, f1=None):
    """level-major ids of frames [f0, f1)"""
    if f0 is None:
        return np.concatenate(levels)
    return np.concatenate([l[f0 * (FRAME_TOKENS // r):f1 * (FRAME_TOKENS // r)] for l, r in zip(levels, (4, 2, 1))])


def _noise_layers(cfg, K, seed):
    """per layer: K frames x (4 * prod(stride_0..l)) normals"""
    rng = np.random.default_rng(seed)
    out, up = [], 1
    for s in cfg.strides:
        up *= s
        out.append(rng.standard_normal(FRAME_TOKENS * K * up).astype(np.float32))
    return out


def _noise_flat(cfg, layers, f0, f1):
    out, up = [], 1
    for s, l in zip(cfg.strides, layers):
        up *= s
        out.append(l[f0 * FRAME_TOKENS * up:f1 * FRAME_TOKENS * up])
    return np.concatenate(out)


def _changed_frames(a, b, per):
    return np.nonzero(np.abs(a - b).reshape(-1, per).max(axis=1) != 0)[0]


def test_halo_is_correct_and_tight():
    cfg = synth.snac_tiny(max_frames=4096)
    model = synth.build_snac(cfg)
    o = orc.SnacOracle(model)
    h = hip.snac_halo_frames(cfg)
    K = 4 * h + 8
    T, per = FRAME_TOKENS * K, FRAME_TOKENS * cfg.hop
    levels = _codes(cfg, K, 7)
    noise = _noise_layers(cfg, K, 8)
    base = o.decode(_flat(levels), T, _noise_flat(cfg, noise, 0, K))
    rng = np.random.default_rng(9)
    reach_codes = reach_noise = 0
    for j in (2 * h + 1, 2 * h + 3, 2 * h + 4):
        for li, r in enumerate(cfg.repeats):   # every id of frame j at this level, one at a time
            for k in range(FRAME_TOKENS // r):
                l2 = [l.copy() for l in levels]
                i = j * (FRAME_TOKENS // r) + k
                l2[li][i] = (l2[li][i] + 1 + rng.integers(0, cfg.cb_size - 1)) % cfg.cb_size
                ch = _changed_frames(o.decode(_flat(l2), T, _noise_flat(cfg, noise, 0, K)), base, per)
                assert ch.size and ch.min() > 0 and ch.max() < K - 1, "the perturbation must stay inside the utterance"
                reach_codes = max(reach_codes, int(j - ch.min()), int(ch.max() - j))
        up = 1
        for li, s in enumerate(cfg.strides):   # the first and the last noise sample of frame j in this layer
            up *= s
            for i in (j * FRAME_TOKENS * up, (j + 1) * FRAME_TOKENS * up - 1):
                n2 = [l.copy() for l in noise]
                n2[li][i] += 1.0
                ch = _changed_frames(o.decode(_flat(levels), T, _noise_flat(cfg, n2, 0, K)), base, per)
                assert ch.size and ch.min() > 0 and ch.max() < K - 1
                reach_noise = max(reach_noise, int(j - ch.min()), int(ch.max() - j))
    assert reach_codes == h
    assert reach_noise <= h


def test_halo_of_the_layouts():
    assert hip.snac_halo_frames(synth.snac_tiny()) == 5
    assert hip.snac_halo_frames(synth.snac_24khz()) == 3   # hubertsiuzdak/snac_24khz: strides 8, 8, 4, 2


def _stitch(o, cfg, levels, noise, K, h, edges):
    out = []
    per = FRAME_TOKENS * cfg.hop
    for f0, f1 in zip(edges[:-1], edges[1:]):
        w0, w1 = max(0, f0 - h), min(K, f1 + h)
        pcm = o.decode(_flat(levels, w0, w1), FRAME_TOKENS * (w1 - w0), None if noise is None else _noise_flat(cfg, noise, w0, w1))
        out.append(pcm[(f0 - w0) * per:(f1 - w0) * per])
    return np.concatenate(out)


def test_windows_with_the_halo_stitch_to_the_full_decode():
    cfg = synth.snac_tiny(max_frames=4096)
    o = orc.SnacOracle(synth.build_snac(cfg))
    h = hip.snac_halo_frames(cfg)
    K = 3 * h + 11
    levels = _codes(cfg, K, 3)
    edges = [0, 3, h + 7, h + 8, 2 * h + 9, K]   # a window clipped at 0, interior ones (one of a single frame), one clipped at K
    for noise in (None, _noise_layers(cfg, K, 4)):
        full = o.decode(_flat(levels), FRAME_TOKENS * K, None if noise is None else _noise_flat(cfg, noise, 0, K))
        stitched = _stitch(o, cfg, levels, noise, K, h, edges)
        assert stitched.shape == full.shape
        assert np.abs(stitched - full).max() <= 1e-6
        short = _stitch(o, cfg, levels, noise, K, h - 1, edges)
        assert np.abs(short - full).max() > 0, "h - 1 frames of halo must not be enough"


def test_oracle_windows_with_halo_frames_match_the_full_decode_at_both_layouts():
    """Windows of 2 kept frames with snac_halo_frames(cfg) frames either side, at the start, the end and two interior positions of a 24-frame
    utterance: the oracle alone reproduces its own full decode within 1e-5 at snac_tiny and at snac_24khz (tests/test_gpu_snac.py decodes the
    same windows on the device and holds them to the float64 decode of the whole utterance).  Measured on the oracle for these windows without
    noise: at snac_tiny a 3-frame halo leaves 5.0e-4, a 4-frame halo 1.1e-5, the 5 frames of snac_halo_frames nothing; at snac_24khz a 2-frame
    halo leaves 1.1e-4 and the 3 frames of snac_halo_frames nothing.  So the halo comes from snac_halo_frames, never from a constant."""
    K = 24
    for cfg, noises in ((synth.snac_tiny(max_frames=4096), (False, True)), (synth.snac_24khz(max_frames=4096), (False,))):
        o = orc.SnacOracle(synth.build_snac(cfg))
        h = hip.snac_halo_frames(cfg)
        per = FRAME_TOKENS * cfg.hop
        levels = _codes(cfg, K, 24)
        for with_noise in noises:
            noise = _noise_layers(cfg, K, 25) if with_noise else None
            full = o.decode(_flat(levels), FRAME_TOKENS * K, None if noise is None else _noise_flat(cfg, noise, 0, K))
            for f0 in (0, 9, 14, K - 2):
                got = _stitch(o, cfg, levels, noise, K, h, [f0, f0 + 2])
                err = float(np.abs(got - full[f0 * per:(f0 + 2) * per]).max())
                print(f"latent {cfg.latent} noise={with_noise} frames [{f0}, {f0 + 2}) halo {h}: {err:.2e}")
                assert err <= 1e-5, (cfg.latent, with_noise, f0, err)
