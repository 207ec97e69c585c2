"""GPU parity: every stage of the DAC-44k decode ("dac:<stage>" snapshots: 0 the quantizer sum, 1 the first conv, 2 + i the end of block i) and
its PCM against float64 torch_dac (tests/golden/make_golden.py) computed here, at lengths past the first position tile of every kernel, around
the tile sizes, in ragged passes and in passes split by TTS_HIP_DAC_GROUP.  tests/test_gpu_dac.py holds the same path to the fp32 oracle at 3
frames, where every layer of the two wide blocks runs inside one tile.

Position tiles of the product path: conv_b3p_kernel 256 (k = 7 at 768 / 384 channels, k = 1 at 768) and 512 (k = 1 at 384), convt_b3_kernel 256
input positions with ti = 0..L inclusive, resunit_t7_kernel 256 (192 channels) and 512 (96 channels), dac_embed_tile_kernel 64 frames,
conv1d_cout1_kernel 256.  A row's stride is its length (dac_row_stride), so a halo read past a row's end lands in the next channel's row: the
masking at the tile that straddles the end is what these lengths run.

Bars (derived, not chosen): the device is held to the project's bar against the oracle plus the oracle's own distance d_ref from float64
(tests/test_oracle_cpu.py::test_dac_oracle_stages_match_float64, the table in its docstring, measured at 70 frames and used at every length:
it is the minor term).
  fp32 arithmetic (every ARITH_CASES row, FLAG_VALU_GEMM, FLAG_DAC_F32 on F16 tensors with the f16_conv = 0 row of d_ref):
      stage 0 max(4 x d_ref, 1e-6), stages >= 1  1e-5 + d_ref[stage], all of max|f64|; PCM 2e-4 absolute and, as the last stage,
      1e-5 x max|pcm64| + d_ref_pcm.
  F16 tensors, fp16 activations: stage 0 as above, stages >= 1  F16_DAC_TOL + d_ref16[stage]; PCM F16_DAC_TOL + d_ref16_pcm absolute.

Measured on the MI355X at 70 frames: the worst stage >= 1 (which one), of max|f64|, and the PCM, absolute, each next to its bar:
    arithmetic (test id)                     worst stage   its bar    PCM       its bar
    default_fp16_hi_lo                       5.15e-06 (4)  1.25e-05   3.13e-06  8.13e-06
    bf16x3, bf16x3_by_env                    2.58e-06 (3)  1.26e-05   1.64e-06  8.13e-06
    exact_fp32, exact_fp32_by_key            3.81e-06 (1)  1.42e-05   1.75e-06  8.13e-06
    units_unfused, units_unfused_conv1_mfma  5.18e-06 (4)  1.25e-05   3.16e-06  8.13e-06
    convt_fp32                               4.14e-06 (2)  1.26e-05   2.55e-06  8.13e-06
    no_planes                                4.90e-06 (4)  1.25e-05   2.99e-06  8.13e-06
    tap_pairs                                4.62e-06 (4)  1.25e-05   2.95e-06  8.13e-06
    convt_fp32_input, units_weights_by_registers: the default's figures (the same products in the same order)
    valu                                     4.03e-06 (1)  1.42e-05   1.46e-06  8.13e-06
    f16_tensors_fp32_activations             1.80e-06 (1)  1.27e-05   9.10e-07  8.21e-06
    f16_default                              5.01e-04 (4)  1.51e-03   3.67e-04  1.36e-03
    f16_tile_kernels                         5.21e-04 (5)  1.48e-03   3.64e-04  1.36e-03
Other lengths, default arithmetic: 31 .. 65 frames worst stage 4.1 - 4.6e-06, PCM 3.1e-06 (bars 7.5 - 8.3e-06); 256 / 257 frames stage 2 3.7 / 3.2e-06,
windows 1.3 - 2.7e-06 (bars 5.3 - 7.5e-06); ragged passes PCM 3.1e-06, one frame alone 3.2e-07 (bar 3.3e-06); F16 tensors at 32 / 33 frames stages
5.3 / 5.7e-04, PCM 3.6 / 4.8e-04.  Stage 0 is 1.5e-07 everywhere (bar 1e-06)."""
import collections
import functools
import importlib.util
import os

import numpy as np
import pytest

from test_gpu_dac import ARITH_CASES, F16_DAC_TOL
from tts_cpp_amd import hip, synth

pytestmark = pytest.mark.gpu

# d_ref: (stage 0 .. 5 of max|f64|, PCM absolute) — the table of tests/test_oracle_cpu.py::test_dac_oracle_stages_match_float64
D_REF = {
    "f32": (1.53e-07, 4.19e-06, 2.58e-06, 2.64e-06, 2.54e-06, 2.24e-06, 1.66e-06),
    "f16_im2col": (1.34e-07, 2.39e-04, 3.46e-04, 4.25e-04, 5.06e-04, 4.81e-04, 3.61e-04),
    "f16_exact": (1.34e-07, 2.67e-06, 2.32e-06, 2.64e-06, 2.76e-06, 2.32e-06, 1.74e-06),
}
PCM_BAR = 2e-4
EDGE = 64    # the first and the last EDGE positions of a stage are reported on their own
HOP = 512
HALO = 12    # frames either side of a window: the decoder's receptive field is 10 (tts_hip_dac_halo_frames)


Bars = collections.namedtuple("Bars", "stages pcm_abs pcm_rel d_pcm")


def stage_bars(ref_row, fp16_activations):
    """stages: the bar per stage, of max|f64|; pcm_abs: the absolute PCM bar; pcm_rel (fp32 arithmetic): the PCM as the last stage, of max|pcm64|"""
    d = D_REF[ref_row]
    first = max(4 * d[0], 1e-6)
    if fp16_activations:
        return Bars([first] + [F16_DAC_TOL + x for x in d[1:6]], F16_DAC_TOL + d[6], None, d[6])
    return Bars([first] + [1e-5 + x for x in d[1:6]], PCM_BAR, 1e-5, d[6])


def pcm_bar(bars, pcm64):
    """the absolute bar on a PCM array: the project's, and for fp32 arithmetic the PCM as the last stage (1e-5 of max|pcm64| + d_ref_pcm) as well.
    For a window of an utterance max|pcm64| is the window's own, at most the utterance's: the stricter reading."""
    if bars.pcm_rel is None:
        return bars.pcm_abs
    return min(bars.pcm_abs, bars.pcm_rel * float(np.abs(pcm64).max()) + bars.d_pcm)


@functools.lru_cache(maxsize=None)
def make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(__file__), "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def dac_model(dac_f16):
    return synth.build(synth.parler_mini(layers=1, prompt_vocab=64, ctx=64, dac_f16=dac_f16))   # decoder part irrelevant here


@functools.lru_cache(maxsize=None)
def dac_case(frames, seed=None):
    """codes of an F-frame utterance (seed None: F itself, the codes d_ref was measured on at F = 70), read-only"""
    cfg = dac_model(False).cfg
    codes = np.random.default_rng(frames if seed is None else seed).integers(0, cfg.cb_size, (frames, cfg.n_out)).astype(np.uint32)
    codes.setflags(write=False)
    return codes


def frozen(a):
    a = a.numpy()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def f64_ref(dac_f16, frames, seed=None, last_stage=None):
    """float64 torch_dac of dac_case: (pcm, [stages]) (pcm None with last_stage), computed once and read-only"""
    if frames == 0:
        return np.zeros(0), []
    if last_stage is not None:
        return None, [frozen(a) for a in make_golden().torch_dac(dac_model(dac_f16), dac_case(frames, seed), last_stage=last_stage)]
    pcm, st = make_golden().torch_dac(dac_model(dac_f16), dac_case(frames, seed), stages=True)
    return frozen(pcm), [frozen(a) for a in st]


@functools.lru_cache(maxsize=None)
def f64_window(dac_f16, frames, f0, f1):
    """float64 PCM of frames [f0, f1) of dac_case(frames), from a decode of the surrounding +-HALO frames alone (finite receptive field)"""
    lo, hi = max(0, f0 - HALO), min(frames, f1 + HALO)
    pcm = make_golden().torch_dac(dac_model(dac_f16), dac_case(frames)[lo:hi])
    return frozen(pcm[(f0 - lo) * HOP:(f1 - lo) * HOP])


def engine(dac_f16=False, flags=0, tune=None):
    model = dac_model(dac_f16)
    eng = hip.HipEngine(model.cfg, flags=hip.FLAG_NO_PARLER | flags, tune=tune or {})
    eng.load(model)
    return eng


def worst_of(err):
    """(worst, first EDGE, last EDGE, position of the worst modulo 256) of an error array whose last axis is the position"""
    pos = int(np.unravel_index(int(err.argmax()), err.shape)[-1])
    return float(err.max()), float(err[..., :EDGE].max()), float(err[..., -EDGE:].max()), pos


def check_stages(eng, ref_stages, bars, label):
    """every "dac:<stage>" snapshot against float64: the whole stage, its first and its last EDGE positions; prints them, then asserts; -> worst stage >= 1"""
    bad, worst = [], 0.0
    for st, (ref, bar) in enumerate(zip(ref_stages, bars.stages)):
        act = eng.debug_read(f"dac:{st}", ref.size)
        assert act.size == ref.size, (label, st, act.size, ref.shape)
        whole, first, last, pos = worst_of(np.abs(act.reshape(ref.shape) - ref) / np.abs(ref).max())
        print(f"{label} stage {st} {ref.shape}: worst {whole:.2e} (first {EDGE}: {first:.2e}, last {EDGE}: {last:.2e}) bar {bar:.2e}")
        if st:
            worst = max(worst, whole)
        if not whole < bar:
            bad.append((st, f"{whole:.2e} at position {pos} = {pos % 256} mod 256 of {ref.shape[1]}", f"first {first:.2e}", f"last {last:.2e}"))
    assert not bad, (label, bad)
    return worst


def check_pcm(pcm, pcm64, bars, label):
    assert pcm.shape == pcm64.shape, (label, pcm.shape, pcm64.shape)
    if pcm.size == 0:
        return 0.0
    bar = pcm_bar(bars, pcm64)
    whole, first, last, pos = worst_of(np.abs(pcm - pcm64))
    print(f"{label} PCM ({pcm.size}): worst {whole:.2e} (first {EDGE}: {first:.2e}, last {EDGE}: {last:.2e}) bar {bar:.2e}")
    assert whole < bar, (label, f"{whole:.2e} at sample {pos} = {pos % 256} mod 256 of {pcm.size}", f"first {first:.2e}", f"last {last:.2e}", f"bar {bar:.2e}")
    return whole


F16_PLANES = 8 | 128
STAGE_CASES = [
    # (id, environment, tts_hip_tune keys, extra flags, F16 tensors, tts_hip_dac_arith bits expected, d_ref row, fp16 activations)
    *[(name, env, tune, 0, False, arith, "f32", False) for name, env, tune, arith in ARITH_CASES],
    ("valu", {}, {}, hip.FLAG_VALU_GEMM, False, 16, "f32", False),                          # the scalar-FMA kernels
    ("f16_default", {}, {}, 0, True, F16_PLANES, "f16_im2col", True),                       # F16 tensors: the plane kernels with one fp16 plane
    ("f16_tile_kernels", {}, {"dac_f16_planes": 0}, 0, True, 8, "f16_im2col", True),        # ... the fp16 tile kernels of round 2
    ("f16_tensors_fp32_activations", {}, {}, hip.FLAG_DAC_F32, True, 1 | 2 | 4 | 32 | 64, "f16_exact", False),
]


@pytest.mark.parametrize("case", STAGE_CASES, ids=[c[0] for c in STAGE_CASES])
def test_dac_44k_stages_at_a_length_of_several_tiles(case, monkeypatch):
    """70 frames: stage lengths 70, 70, 560, 4480, 17920, 35840.  The embed tiles (64 frames) and the block-0 kernels (256 positions) cross a
    boundary, block 1 crosses its 256- and its 512-position tiles with a partial last tile each, the dilation-9 halos cross tile boundaries
    in both wide blocks — under the product default, every fallback switch (ARITH_CASES), the scalar-FMA kernels and the three arithmetics of
    F16 tensors.  All six snapshots and the PCM against float64; then the same decode without the snapshots bit for bit (debug mode makes the
    wide blocks also write an fp32 tensor that production skips)."""
    name, env, tune, flags, dac_f16, arith, ref_row, fp16_act = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    F = 70
    codes = dac_case(F)
    pcm64, st64 = f64_ref(dac_f16, F)
    assert [a.shape[1] for a in st64] == [70, 70, 560, 4480, 17920, 35840]
    bars = stage_bars(ref_row, fp16_act)
    eng = engine(dac_f16, flags, tune)
    assert eng.L.tts_hip_dac_arith(eng.ctx) == arith
    eng.set_debug(True)
    pcm = eng.dac_decode(codes)
    label = f"dac_44k F={F} {name}"
    worst = check_stages(eng, st64, bars, label)
    err = check_pcm(pcm, pcm64, bars, label)
    print(f"{label}: worst stage >= 1 {worst:.2e}, PCM {err:.2e}")
    eng.set_debug(False)
    assert np.array_equal(eng.dac_decode(codes), pcm)   # the snapshots change nothing
    eng.close()


@pytest.mark.parametrize("F,dac_f16", [(31, False), (32, False), (33, False), (64, False), (65, False), (32, True), (33, True)],
                         ids=["31", "32", "33", "64", "65", "32-f16", "33-f16"])
def test_dac_44k_stages_around_the_tile_sizes(F, dac_f16):
    """8 F = 256: block 0 is exactly one tile and block 1's transposed conv gets a second tile holding only ti = L; 264: block 0 ends 8 positions
    into its second tile; 512 and 520: the same at the 512-position tiles of block 1's k = 1 convs; 64 and 65 frames are the embed-tile
    edges; 31 stays below all of them.  Default arithmetic, and F16 tensors on the plane kernels at 32 and 33."""
    pcm64, st64 = f64_ref(dac_f16, F)
    bars = stage_bars("f16_im2col" if dac_f16 else "f32", dac_f16)
    eng = engine(dac_f16)
    eng.set_debug(True)
    pcm = eng.dac_decode(dac_case(F))
    label = f"dac_44k F={F}{' f16' if dac_f16 else ''}"
    check_stages(eng, st64, bars, label)
    check_pcm(pcm, pcm64, bars, label)
    eng.close()


@pytest.mark.parametrize("F", [256, 257])
def test_dac_44k_first_layers_past_one_tile(F):
    """The first conv (1024 -> 1536, k = 7), the first transposed conv (ti = 256 alone in a tile, then one real position in it) and five embed
    tiles: stages 0..2 against float64, and the PCM on windows of 2 frames at frames 0, 254, 256 and F - 2 (cut at the utterance's end), each
    against a float64 decode of the surrounding +-12 frames (the receptive-field argument of test_measured_codec_shape_windows_match_oracle).
    Dia generates up to 3072 frames through this path."""
    _, st64 = f64_ref(False, F, None, 2)
    assert [a.shape[1] for a in st64] == [F, F, 8 * F]
    bars = stage_bars("f32", False)
    eng = engine()
    eng.set_debug(True)
    pcm = eng.dac_decode(dac_case(F))
    assert pcm.shape == (F * HOP,)
    check_stages(eng, st64, bars, f"dac_44k F={F}")
    for f0 in sorted({0, 254, 256, F - 2}):
        f1 = min(f0 + 2, F)
        if f0 < f1:
            check_pcm(pcm[f0 * HOP:f1 * HOP], f64_window(False, F, f0, f1), bars, f"dac_44k F={F} frames [{f0}, {f1})")
    eng.close()


@pytest.mark.parametrize("frames,dac_f16", [((70, 1, 33, 0, 32), False), ((32, 0, 33, 1, 70), False), ((70, 1, 33, 0, 32), True)],
                         ids=["longest-first", "longest-last", "longest-first-f16"])
def test_dac_44k_ragged_pass_matches_float64_per_utterance(frames, dac_f16, monkeypatch):
    """Utterances of different lengths in one pass (grid.z, per-utterance valid lengths).  With the longest last, every shorter row has a
    neighbour's samples beyond its end, mid-tile in the wide classes.  Every output against the float64 decode of that utterance alone, and
    bit for bit the single decode of it on the same engine AFTER the long pass (stale buffer contents lie beyond the row); a second engine
    with TTS_HIP_DAC_GROUP=2 splits the batch into three passes, one straddling the empty utterance (code_off / pcm_off over ragged lengths):
    bit for bit the one-pass outputs."""
    ref_row = "f16_im2col" if dac_f16 else "f32"
    bars = stage_bars(ref_row, dac_f16)
    utts = [dac_case(f) for f in frames]
    eng = engine(dac_f16)
    assert eng.L.tts_hip_dac_arith(eng.ctx) == (F16_PLANES if dac_f16 else ARITH_CASES[0][3])
    outs = eng.dac_decode_batch(utts)
    assert len(outs) == len(frames)
    for i, (f, out) in enumerate(zip(frames, outs)):
        check_pcm(out, f64_ref(dac_f16, f)[0], bars, f"dac_44k ragged {frames}{' f16' if dac_f16 else ''} utterance {i} ({f} frames)")
    for i, (c, out) in enumerate(zip(utts, outs)):
        assert np.array_equal(out, eng.dac_decode(c)), i
    eng.close()
    monkeypatch.setenv("TTS_HIP_DAC_GROUP", "2")
    eng2 = engine(dac_f16)
    outs2 = eng2.dac_decode_batch(utts)
    eng2.close()
    assert len(outs2) == len(outs)
    for i, (a, b) in enumerate(zip(outs, outs2)):
        assert a.shape == b.shape and np.array_equal(a, b), i
