"""GPU parity: the SNAC codec (tts_hip_snac_decode; Orpheus' audio decoder, src/decoder/snac_model.cpp) against the
oracle (orc_snac_decode, pinned to a float64 torch restatement in tests/golden/tiny_snac.npz by tests/test_oracle_cpu.py).
PCM is a tanh output: 1e-4 absolute, as for DAC.

The stage tests further down hold every stage of the pass ("snac:<stage>" snapshots) and the PCM to float64 torch_snac
(tests/golden/make_golden.py) computed here, at lengths of several tiles, in ragged passes and in windows."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import hip, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "tiny_snac.npz")


def rand_codes(cfg, T, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, cfg.cb_size, T // r) for r in cfg.repeats]).astype(np.uint32)


@pytest.mark.parametrize("flags", [0, hip.FLAG_VALU_GEMM])
def test_tiny_snac_matches_oracle_and_golden(flags):
    model = synth.build_snac(synth.snac_tiny())
    eng = hip.SnacEngine(model.cfg, flags=flags)
    eng.load(model)
    o = orc.SnacOracle(model)
    g = np.load(GOLD)
    T = int(g["T"])
    pcm_n = eng.decode(g["codes"], T, g["noise"])
    pcm_c = eng.decode(g["codes"], T, None)
    assert np.abs(pcm_n - g["pcm_noise"]).max() < 1e-4 and np.abs(pcm_c - g["pcm_clean"]).max() < 1e-4
    assert np.abs(pcm_n - pcm_c).max() > 1e-3          # the noise block does something
    for T2 in (4, 8, 40):
        codes = rand_codes(model.cfg, T2, T2)
        noise = np.random.default_rng(T2).standard_normal(o.noise_len(T2)).astype(np.float32)
        assert np.abs(eng.decode(codes, T2, noise) - o.decode(codes, T2, noise)).max() < 1e-4, T2
    assert eng.decode(np.zeros(0, dtype=np.uint32), 0).size == 0
    with pytest.raises(hip.HipError):
        eng.decode(rand_codes(model.cfg, 8, 1)[:-1].tolist() + [model.cfg.cb_size], 8)   # id outside the codebook
    with pytest.raises(hip.HipError):
        eng.decode(rand_codes(model.cfg, 8, 1), 6)                                          # T not a multiple of 4
    eng.close()


def test_snac_24khz_shapes():
    """hubertsiuzdak/snac_24khz dims (768 -> 1024 -> 512 -> 256 -> 128 -> 64 channels, strides 8,8,4,2, codebooks 4096 x 8):
    every pointwise conv and transposed conv on its MFMA tile."""
    model = synth.build_snac(synth.snac_24khz(max_frames=16))
    eng = hip.SnacEngine(model.cfg)
    eng.load(model)
    o = orc.SnacOracle(model)
    T = 8
    codes = rand_codes(model.cfg, T, 3)
    noise = np.random.default_rng(3).standard_normal(o.noise_len(T)).astype(np.float32)
    pcm = eng.decode(codes, T, noise)
    assert pcm.shape == (T * 512,)
    assert np.abs(pcm - o.decode(codes, T, noise)).max() < 2e-4
    assert np.array_equal(pcm, eng.decode(codes, T, noise))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
# Every stage against float64.  A stage may differ from float64 by max(4 x d_ref[stage], 1e-6) of max|f64|: d_ref is the distance of the
# fp32 oracle from the same float64 arrays (measured by tests/test_oracle_cpu.py::test_snac_oracle_stages_match_float64, the table in its
# docstring, on the codes and noise of snac_case), 4 x because kernel and oracle are both fp32 accumulations in different orders, and the
# floor covers stage 0, where both may be exact to an ulp.  PCM: 2e-4 absolute.
# ------------------------------------------------------------------------------------------------------------------------------------------
D_REF = {
    ("snac_tiny", True): (1.14e-07, 3.10e-07, 4.70e-07, 3.86e-07, 5.03e-07),
    ("snac_tiny", False): (1.14e-07, 3.10e-07, 4.55e-07, 4.85e-07, 4.21e-07),
    ("snac_24khz", True): (8.74e-08, 1.44e-06, 1.68e-06, 1.38e-06, 1.27e-06, 1.23e-06, 1.05e-06),
    ("snac_24khz", False): (8.74e-08, 1.44e-06, 1.72e-06, 1.42e-06, 1.27e-06, 1.12e-06, 1.04e-06),
}
PCM_BAR = 2e-4
EDGE = 64   # the first and the last EDGE positions of a stage are also held to the bar on their own
FRAME_TOKENS = 4


def stage_bars(layout, with_noise):
    return [max(4 * d, 1e-6) for d in D_REF[(layout, with_noise)]]


@functools.lru_cache(maxsize=None)
def make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(__file__), "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def snac_model(layout, max_frames):
    return synth.build_snac(getattr(synth, layout)(max_frames=max_frames))


def noise_len(cfg, T):
    n, L = 0, T
    for s in cfg.strides:
        L *= s
        n += L
    return n


@functools.lru_cache(maxsize=None)
def snac_case(layout, T, seed=None):
    """codes and noise of a T-token utterance (seed None: the ones d_ref was measured on), read-only"""
    cfg = getattr(synth, layout)()
    codes = rand_codes(cfg, T, T if seed is None else seed)
    noise = np.random.default_rng((T if seed is None else seed) + 1).standard_normal(noise_len(cfg, T)).astype(np.float32)
    codes.setflags(write=False)
    noise.setflags(write=False)
    return codes, noise


@functools.lru_cache(maxsize=None)
def f64_ref(layout, T, with_noise, seed=None):
    """float64 torch_snac of snac_case: (pcm, [stages]), computed once and read-only"""
    codes, noise = snac_case(layout, T, seed)
    pcm, st = make_golden().torch_snac(snac_model(layout, 128), codes, T, noise if with_noise else None, stages=True)
    out = pcm.numpy(), [a.numpy() for a in st]
    out[0].setflags(write=False)
    for a in out[1]:
        a.setflags(write=False)
    return out


def check_stages(eng, ref_stages, bars, label):
    """every "snac:<stage>" snapshot against float64: the whole stage, its first and its last EDGE positions; prints the worst values, then asserts"""
    bad = []
    for st, (ref, bar) in enumerate(zip(ref_stages, bars)):
        act = eng.debug_read(f"snac:{st}", ref.size)
        assert act.size == ref.size, (label, st, act.size, ref.shape)
        err = np.abs(act.reshape(ref.shape) - ref) / np.abs(ref).max()
        whole, first, last = float(err.max()), float(err[:, :EDGE].max()), float(err[:, -EDGE:].max())
        print(f"{label} stage {st} {ref.shape}: worst {whole:.2e} (first {EDGE}: {first:.2e}, last {EDGE}: {last:.2e}) bar {bar:.2e}")
        if not whole < bar:
            bad.append((st, "first" if not first < bar else "last" if not last < bar else "interior", whole))
    assert not bad, (label, bad)


@pytest.mark.parametrize("flags,with_noise", [(0, True), (0, False), (hip.FLAG_VALU_GEMM, True)], ids=["mfma-noise", "mfma-clean", "valu-noise"])
def test_snac_24khz_stages_at_a_length_of_several_tiles(flags, with_noise):
    """snac_24khz at T = 76 (19 frames): stage lengths 76, 608, 4864, 19456, 38912, so the embed groups (64), the depthwise groups (256) and
    every conv position tile (64, 128, 256) run full tiles, a tile boundary and a partial last tile, the 1024- and 512-channel layers too;
    the scalar-FMA fallback at the same dims."""
    layout, T = "snac_24khz", 76
    model = snac_model(layout, 128)
    codes, noise = snac_case(layout, T)
    pcm64, st64 = f64_ref(layout, T, with_noise)
    assert [a.shape[1] for a in st64] == [76, 76, 608, 4864, 19456, 38912, 38912]
    eng = hip.SnacEngine(model.cfg, flags=flags)
    eng.load(model)
    eng.set_debug(True)
    pcm = eng.decode(codes, T, noise if with_noise else None)
    err = float(np.abs(pcm - pcm64).max())
    print(f"snac_24khz T={T} flags={flags} noise={with_noise}: PCM worst {err:.2e} (first {EDGE}: {np.abs(pcm - pcm64)[:EDGE].max():.2e}, "
          f"last {EDGE}: {np.abs(pcm - pcm64)[-EDGE:].max():.2e}) bar {PCM_BAR:.0e}")
    check_stages(eng, st64, stage_bars(layout, with_noise), f"snac_24khz T={T} flags={flags} noise={with_noise}")
    assert err < PCM_BAR
    eng.set_debug(False)
    assert np.array_equal(eng.decode(codes, T, noise if with_noise else None), pcm)   # the snapshots change nothing
    eng.close()


@pytest.mark.parametrize("T", [60, 64, 68, 128, 132])
def test_snac_tiny_stages_around_the_group_sizes(T):
    """snac_tiny below, at and above the 64-token embed group, and (strides 4, 2) at and above multiples of the 256-position depthwise group
    after upsampling (64 * 4 = 256, 68 * 4 = 272, 128 * 8 = 1024), max_frames == T: the buffers hold exactly this utterance"""
    layout = "snac_tiny"
    model = snac_model(layout, T)
    codes, noise = snac_case(layout, T)
    pcm64, st64 = f64_ref(layout, T, True)
    eng = hip.SnacEngine(model.cfg)
    eng.load(model)
    eng.set_debug(True)
    pcm = eng.decode(codes, T, noise)
    err = float(np.abs(pcm - pcm64).max())
    print(f"snac_tiny T={T}: PCM worst {err:.2e} bar {PCM_BAR:.0e}")
    check_stages(eng, st64, stage_bars(layout, True), f"snac_tiny T={T}")
    assert err < PCM_BAR
    eng.close()


@pytest.mark.parametrize("layout,frames,with_noise", [
    ("snac_tiny", (19, 1, 7, 12, 2), True),      # the longest utterance first
    ("snac_tiny", (2, 12, 7, 1, 19), True),      # ... and last: LS is the longest, every shorter row has a neighbour's samples beyond its edge
    ("snac_tiny", (19, 1, 7, 12, 2), False),
    ("snac_24khz", (5, 1, 3), True),
    ("snac_24khz", (3, 1, 5), True),
], ids=["tiny-first", "tiny-last", "tiny-first-clean", "24khz-first", "24khz-last"])
def test_snac_ragged_pass_matches_float64_per_utterance(layout, frames, with_noise):
    """decode_windows with utterances of different lengths (grid.z, per-utterance valid length), keep = the whole window, per-window noise:
    each output is the float64 decode of that utterance alone with its own noise (2e-4), and eng.decode of it bit for bit; the same through
    _begin / _end; utterance 0's stages of the ragged pass against float64 as well."""
    model = snac_model(layout, 128)
    eng = hip.SnacEngine(model.cfg)
    eng.load(model)
    cases = [snac_case(layout, FRAME_TOKENS * f, 100 + i) for i, f in enumerate(frames)]
    wins = [(c, f, 0, f, nz if with_noise else None) for (c, nz), f in zip(cases, frames)]
    eng.set_debug(True)
    outs = eng.decode_windows(wins)
    check_stages(eng, f64_ref(layout, FRAME_TOKENS * frames[0], with_noise, 100)[1], stage_bars(layout, with_noise), f"{layout} ragged {frames} utterance 0")
    eng.set_debug(False)
    outs_split = eng.decode_windows(wins, split=True)
    worst = 0.0
    for i, ((c, nz), f) in enumerate(zip(cases, frames)):
        T = FRAME_TOKENS * f
        pcm64 = f64_ref(layout, T, with_noise, 100 + i)[0]
        assert outs[i].shape == pcm64.shape
        err = float(np.abs(outs[i] - pcm64).max())
        worst = max(worst, err)
        print(f"{layout} ragged {frames} noise={with_noise} utterance {i} ({f} frames): PCM worst {err:.2e} bar {PCM_BAR:.0e}")
        assert err < PCM_BAR, i
        assert np.array_equal(outs[i], eng.decode(c, T, nz if with_noise else None)), i
        assert np.array_equal(outs_split[i], outs[i]), i
    eng.close()


def test_snac_24khz_windows_match_float64_of_the_whole_utterance():
    """Windows of 2 kept frames with halo_frames() frames either side, at the start, the end and two interior positions of a 24-frame utterance,
    in one pass: the kept PCM is the same samples of the float64 decode of the WHOLE utterance (2e-4, no noise) — held against the reference,
    not against the engine's own full decode.  (tests/test_orpheus_chunked_cpu.py: the oracle's own windows with this halo reproduce its full
    decode, so the halo is not what this bar measures.)"""
    layout, K = "snac_24khz", 24
    model = snac_model(layout, 128)
    cfg = model.cfg
    T = FRAME_TOKENS * K
    codes, _ = snac_case(layout, T)
    pcm64 = f64_ref(layout, T, False)[0]
    levels, off = [], 0
    for r in cfg.repeats:
        levels.append(codes[off:off + T // r])
        off += T // r
    eng = hip.SnacEngine(cfg)
    eng.load(model)
    h = eng.halo_frames()
    per = FRAME_TOKENS * cfg.hop
    wins, kept = [], []
    for f0 in (0, 9, 14, K - 2):
        w0, w1 = max(0, f0 - h), min(K, f0 + 2 + h)
        wc = np.concatenate([l[w0 * (FRAME_TOKENS // r):w1 * (FRAME_TOKENS // r)] for l, r in zip(levels, cfg.repeats)])
        wins.append((wc, w1 - w0, f0 - w0, f0 - w0 + 2, None))
        kept.append(f0)
    outs = eng.decode_windows(wins)
    for f0, out in zip(kept, outs):
        ref = pcm64[f0 * per:(f0 + 2) * per]
        assert out.shape == ref.shape
        err = float(np.abs(out - ref).max())
        print(f"snac_24khz window frames [{f0}, {f0 + 2}) of {K}, halo {h}: PCM worst {err:.2e} bar {PCM_BAR:.0e}")
        assert err < PCM_BAR, f0
    eng.close()
