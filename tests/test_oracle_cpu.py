"""CPU tests of the oracle: golden vectors (independent float64 torch restatement), PyTorch primitive
semantics, block formats.  The oracle is the checker for the HIP path, so it is pinned first."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import oracle as orc
from tts_cpp_amd import gguf, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tiny_f32.npz")


def relerr(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def tiny_f32():
    return synth.build(synth.tiny(weight_type=gguf.F32))


def test_golden_parler_decode(tiny_f32):
    g = np.load(GOLD)
    cfg = tiny_f32.cfg
    o = orc.ParlerOracle(tiny_f32, act_mode=0, gelu_mode=0)
    _, h0 = o.decode(g["prompt"], 0, audio=False, want_logits=False, want_hidden=True)
    assert relerr(h0, g["prompt_hidden"]) < 2e-5
    for s in range(g["audio_ids"].shape[0]):
        lg, h = o.decode(g["audio_ids"][s], len(g["prompt"]) + s, audio=True, want_hidden=True)
        assert relerr(lg[:, 0, :], g["logits"][s]) < 2e-5, s
        assert relerr(h[0], g["hidden"][s]) < 2e-5, s
        assert (lg[:, 0, :].argmax(-1) == g["logits"][s].argmax(-1)).all()
    n_pos = g["k_layer0"].shape[0]
    k0, _ = o.get_kv(0, n_pos)
    _, v1 = o.get_kv(cfg.layers - 1, n_pos)
    assert relerr(k0, g["k_layer0"]) < 2e-5
    assert relerr(v1, g["v_last"]) < 2e-5


def test_golden_dac(tiny_f32):
    g = np.load(GOLD)
    d = orc.DacOracle(tiny_f32)
    pcm = d.decode(g["codes"])
    assert pcm.shape == g["pcm"].shape
    assert np.abs(pcm - g["pcm"]).max() < 2e-5
    for st in range(2 + len(tiny_f32.cfg.strides)):
        _, act = d.decode(g["codes"], stage=st)
        assert relerr(act, g[f"dac_stage{st}"]) < 2e-5, st


@pytest.mark.parametrize("K,pad,dil", [(7, 3, 1), (7, 9, 3), (7, 27, 9), (1, 0, 1)])
def test_conv1d_vs_torch(K, pad, dil):
    rng = np.random.default_rng(K * 100 + dil)
    cin, cout, L = 5, 6, 50
    x = rng.standard_normal((cin, L)).astype(np.float32)
    w = rng.standard_normal((cout, cin, K)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    y = np.empty((cout, L), dtype=np.float32)
    orc.lib().orc_conv1d(orc.f32p(x), cin, L, orc.f32p(w), orc.f32p(b), cout, K, pad, dil, orc.f32p(y))
    ref = Fn.conv1d(torch.from_numpy(x)[None].double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=pad, dilation=dil)[0].numpy()
    assert np.abs(y - ref).max() < 1e-4


@pytest.mark.parametrize("stride,pad", [(8, 4), (4, 2), (2, 1), (5, 3)])
def test_conv_transpose1d_vs_torch(stride, pad):
    rng = np.random.default_rng(stride)
    cin, cout, L, K = 6, 4, 11, 2 * stride
    x = rng.standard_normal((cin, L)).astype(np.float32)
    w = rng.standard_normal((cin, cout, K)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    Lout = (L - 1) * stride - 2 * pad + K
    y = np.empty((cout, Lout), dtype=np.float32)
    orc.lib().orc_conv_transpose1d(orc.f32p(x), cin, L, orc.f32p(w), orc.f32p(b), cout, K, stride, pad, orc.f32p(y))
    ref = Fn.conv_transpose1d(torch.from_numpy(x)[None].double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=stride, padding=pad)[0].numpy()
    assert ref.shape == y.shape
    assert np.abs(y - ref).max() < 1e-4
    if stride % 2 == 0 and pad == stride // 2:
        assert Lout == L * stride  # DAC blocks upsample by exactly their stride


def test_layer_norm_and_gelu_vs_torch():
    rng = np.random.default_rng(3)
    H = 256
    x = (rng.standard_normal(H) * 3 + 1).astype(np.float32)
    w = rng.standard_normal(H).astype(np.float32)
    b = rng.standard_normal(H).astype(np.float32)
    y = np.empty(H, dtype=np.float32)
    orc.lib().orc_layer_norm(orc.f32p(x), H, orc.f32p(w), orc.f32p(b), orc.f32p(y))
    ref = Fn.layer_norm(torch.from_numpy(x).double(), (H,), torch.from_numpy(w).double(), torch.from_numpy(b).double(), 1e-5).numpy()
    assert np.abs(y - ref).max() < 1e-5
    xs = np.linspace(-12, 12, 4001).astype(np.float32)
    g0 = np.array([orc.lib().orc_gelu(float(v), 0) for v in xs], dtype=np.float32)
    refg = Fn.gelu(torch.from_numpy(xs).double(), approximate="tanh").numpy()
    assert np.abs(g0 - refg).max() < 2e-6
    # ggml fp16-table mode: fp16-precision of the same function, identity/zero outside (-10, 10)
    g1 = np.array([orc.lib().orc_gelu(float(v), 1) for v in xs], dtype=np.float32)
    inside = np.abs(xs) < 10
    assert np.abs(g1[inside] - refg[inside]).max() < 6e-3
    assert (g1[xs >= 10] == xs[xs >= 10]).all() and (g1[xs <= -10] == 0).all()
    assert (g1[inside] == g1[inside].astype(np.float16).astype(np.float32)).all()  # table entries are fp16


def test_fp16_conversion_matches_numpy():
    L = orc.lib()
    bits = np.arange(0, 65536, dtype=np.uint16)
    vals = bits.view(np.float16).astype(np.float32)
    mine = np.array([L.orc_h2f(int(b)) for b in bits[::7]], dtype=np.float32)
    ref = vals[::7]
    ok = (mine == ref) | (np.isnan(mine) & np.isnan(ref))
    assert ok.all()
    rng = np.random.default_rng(0)
    f = np.concatenate([rng.standard_normal(5000).astype(np.float32) * s for s in (1e-8, 1e-5, 1e-3, 1, 1e3, 7e4)])
    f = np.concatenate([f, np.array([0.0, -0.0, 65504.0, 65519.9, 65520.0, 1e9, -1e9, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25], dtype=np.float32)])
    with np.errstate(over="ignore"):
        ref16 = f.astype(np.float16).view(np.uint16)
    mine16 = np.array([L.orc_f2h(float(v)) for v in f], dtype=np.uint16)
    assert (mine16 == ref16).all()


@pytest.mark.parametrize("ttype", [gguf.Q4_0, gguf.Q5_0, gguf.Q8_0, gguf.F16])
def test_block_formats(ttype):
    rng = np.random.default_rng(ttype)
    x = (rng.standard_normal(32 * 64) * rng.uniform(0.01, 3, 32 * 64)).astype(np.float32)
    q_c = orc.quantize(ttype, x)
    if ttype != gguf.F16:
        q_np = synth.quantize(x, ttype)
        assert (q_c == q_np).all(), "numpy quantiser (synth) and oracle quantiser disagree"
    dq = orc.dequantize(ttype, q_c, x.size)
    tol = {gguf.Q4_0: 0.13, gguf.Q5_0: 0.065, gguf.Q8_0: 0.005, gguf.F16: 0.0006}[ttype]  # one quantisation step (clamped end included)
    blk = np.abs(x).reshape(-1, 32).max(axis=1).repeat(32)
    assert (np.abs(dq - x) <= tol * blk + 1e-7).all()
    # dequantised values re-quantise to themselves (formats are idempotent)
    assert (orc.quantize(ttype, dq) == q_c).all() or ttype in (gguf.Q4_0, gguf.Q5_0)


def test_mul_mat_modes():
    rng = np.random.default_rng(11)
    K, N, R = 256, 48, 3
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    x = rng.standard_normal((R, K)).astype(np.float32)
    exact = x.astype(np.float64) @ w.astype(np.float64).T
    y = orc.mul_mat(gguf.F32, w.tobytes(), K, N, x)
    assert np.abs(y - exact).max() < 1e-5
    w16 = w.astype(np.float16)
    y0 = orc.mul_mat(gguf.F16, w16.tobytes(), K, N, x, act_mode=0)
    assert np.abs(y0 - x.astype(np.float64) @ w16.astype(np.float64).T).max() < 1e-5
    y1 = orc.mul_mat(gguf.F16, w16.tobytes(), K, N, x, act_mode=1)
    x16 = x.astype(np.float16).astype(np.float64)
    assert np.abs(y1 - x16 @ w16.astype(np.float64).T).max() < 1e-5
    for t in (gguf.Q4_0, gguf.Q5_0, gguf.Q8_0):
        q = orc.quantize(t, w)
        wd = orc.dequantize(t, q, w.size).reshape(N, K).astype(np.float64)
        ya = orc.mul_mat(t, q, K, N, x, act_mode=0)
        assert np.abs(ya - x.astype(np.float64) @ wd.T).max() < 1e-5
        yb = orc.mul_mat(t, q, K, N, x, act_mode=1)  # Q8_0 activations: close to, not equal to, the fp32-activation result
        assert np.abs(yb - ya).max() < 0.05 * np.abs(ya).max()


def test_generation_bookkeeping():
    L = orc.lib()
    n_out, bos, eos = 4, 65, 64
    last = np.array([5, 6, 7, 8], dtype=np.uint32)
    seen = np.array([0, 0, 1, 0], dtype=np.uint8)
    nxt = np.empty(4, dtype=np.uint32)
    import ctypes as C
    for step, exp in [(0, [65, 65, 65, 65]), (1, [5, 65, 65, 65]), (3, [5, 6, 64, 65]), (9, [5, 6, 64, 8])]:
        L.orc_parler_next_ids(n_out, step, orc.u32p(last), seen.ctypes.data_as(C.POINTER(C.c_uint8)), bos, eos, orc.u32p(nxt))
        assert nxt.tolist() == exp
    # un-delay: frame i, head k <- token at step i+k; frames with a special id are dropped
    steps = 7
    toks = (np.arange(steps * n_out) % 50).astype(np.uint32).reshape(steps, n_out)
    toks[2, 1] = eos  # step 2 head 1 -> poisons frame 1
    flat = toks.reshape(-1).copy()
    out = np.empty_like(flat)
    n = L.orc_parler_adjust_output_tokens(orc.u32p(flat), flat.size, n_out, 64, eos, orc.u32p(out))
    frames = out[:n].reshape(-1, n_out)
    expect = [[toks[i + k, k] for k in range(n_out)] for i in range(steps - n_out + 1) if i != 1]
    assert frames.tolist() == [[int(v) for v in r] for r in expect]


def test_t5_encoder_oracle_matches_torch_golden_and_bucket_quirk():
    """orc_t5_encode (src/models/parler/t5/model.cpp:216-320 restated) against tests/golden/tiny_t5.npz (float64 torch:
    rms norm, unscaled attention + relative bias, gated tanh-GELU, final norm, down projection), and the relative
    position buckets against the formula as the reference writes it — integer division inside the log (:314)."""
    import math
    from tts_cpp_amd import synth as sy
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_t5.npz"))
    o = orc.T5Oracle(sy.build_t5(sy.t5_tiny()), act_mode=0, gelu_mode=0)
    assert np.abs(o.encode(g["ids"]) - g["out"]).max() < 2e-5
    o2 = orc.T5Oracle(sy.build_t5(sy.t5_tiny(output_size=192, seed=0x76)), act_mode=0, gelu_mode=0)
    assert np.abs(o2.encode(g["ids"][:23]) - g["out_proj"]).max() < 2e-5
    den = float(np.float32(math.log(128.0 / 8)))
    for key in range(0, 200, 7):
        for query in (0, 3, 50, 199):
            ab = abs(key - query)
            v = ab if ab < 8 else min(15, 8 + int((math.log(ab // 8) / den) * 8))
            assert o.bucket(key, query) == (16 if key > query else 0) + v
    assert o.bucket(12, 0) == 16 + 8      # HF's float division would give 9: the reference's quirk is kept
    # F16 / quantised weights run (ggml activation conversion) and stay close to the F32 model they were made from
    ids = g["ids"][:11]
    ref = orc.T5Oracle(sy.build_t5(sy.t5_tiny())).encode(ids)
    for wt, tol in ((gguf.F16, 5e-3), (gguf.Q8_0, 3e-2)):
        out = orc.T5Oracle(sy.build_t5(sy.t5_tiny(weight_type=wt))).encode(ids)
        assert np.abs(out - ref).max() / np.abs(ref).max() < tol


def test_snac_decoder_oracle_matches_torch_golden():
    """orc_snac_decode (src/decoder/snac_model.cpp:86-159 restated) against tests/golden/tiny_snac.npz (float64 torch:
    repeat_interleave'd codebook levels, depthwise + pointwise convs, ConvTranspose1d, noise block, snake, tanh)."""
    from tts_cpp_amd import synth as sy
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_snac.npz"))
    o = orc.SnacOracle(sy.build_snac(sy.snac_tiny()))
    T = int(g["T"])
    assert np.abs(o.decode(g["codes"], T, g["noise"]) - g["pcm_noise"]).max() < 2e-6
    assert np.abs(o.decode(g["codes"], T, None) - g["pcm_clean"]).max() < 2e-6
    # depthwise conv primitive against torch
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 40)).astype(np.float32)
    w = rng.standard_normal((5, 1, 7)).astype(np.float32)
    b = rng.standard_normal(5).astype(np.float32)
    for dil in (1, 3, 9):
        y = np.empty_like(x)
        orc.lib().orc_conv1d_dw.argtypes = [orc.fp, C.c_int, C.c_int64, orc.fp, orc.fp, C.c_int, C.c_int, C.c_int, orc.fp]
        orc.lib().orc_conv1d_dw.restype = None
        orc.lib().orc_conv1d_dw(orc.f32p(x), 5, 40, orc.f32p(w), orc.f32p(b), 7, 3 * dil, dil, orc.f32p(y))
        ref = Fn.conv1d(torch.from_numpy(x)[None].double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=3 * dil, dilation=dil, groups=5)[0]
        assert np.abs(y - ref.numpy()).max() < 1e-5


def _make_golden():
    """tests/golden/make_golden.py as a module: the float64 torch restatements the golden vectors were made with"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(__file__), "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def snac_case(cfg, T):
    """the codes and the noise of the SNAC stage tests (tests/test_gpu_snac.py decodes the same ones on the device)"""
    rng = np.random.default_rng(T)
    codes = np.concatenate([rng.integers(0, cfg.cb_size, T // r) for r in cfg.repeats]).astype(np.uint32)
    n, L = 0, T
    for s in cfg.strides:
        L *= s
        n += L
    return codes, np.random.default_rng(T + 1).standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "clean"])
@pytest.mark.parametrize("layout,T", [("snac_tiny", 80), ("snac_24khz", 76)])
def test_snac_oracle_stages_match_float64(layout, T, with_noise):
    """Every stage of orc_snac_decode (0 the summed codebook levels, 1 after `in` and `up`, 2 + i the end of block i, last the PCM) against
    float64 torch_snac computed here, at lengths of many tiles: 2e-5 of max|f64| per stage, the bar of the other oracle stages.

    d_ref[stage] = max|orc - f64| / max|f64| as measured (tests/test_gpu_snac.py holds the device to max(4 x d_ref, 1e-6)):

        layout      noise   stage 0   1         2         3         4         5         6
        snac_tiny   yes     1.14e-07  3.10e-07  4.70e-07  3.86e-07  5.03e-07
        snac_tiny   no      1.14e-07  3.10e-07  4.55e-07  4.85e-07  4.21e-07
        snac_24khz  yes     8.74e-08  1.44e-06  1.68e-06  1.38e-06  1.27e-06  1.23e-06  1.05e-06
        snac_24khz  no      8.74e-08  1.44e-06  1.72e-06  1.42e-06  1.27e-06  1.12e-06  1.04e-06

    The float64 PCM at snac_24khz, T = 76, with noise: max |x| 0.31, median 0.077, no sample above 0.99, 0.3 % below 1e-3 (not saturated: an
    absolute bar on PCM means something).  The oracle takes 0.15 s / 0.5 s / 1.3 s for T = 8 / 28 / 76 at these dims."""
    from tts_cpp_amd import synth as sy
    model = sy.build_snac(getattr(sy, layout)(max_frames=128))
    cfg = model.cfg
    o = orc.SnacOracle(model)
    codes, noise = snac_case(cfg, T)
    if not with_noise:
        noise = None
    pcm64, st64 = _make_golden().torch_snac(model, codes, T, noise, stages=True)
    pcm, st = o.decode_stages(codes, T, noise)
    assert len(st) == len(st64) == 3 + len(cfg.strides)
    d = []
    for a, r in zip(st, st64):
        assert a.shape == tuple(r.shape)
        d.append(relerr(a, r.numpy()))
    print(f"{layout} T={T} noise={with_noise}: d_ref per stage " + " ".join(f"{x:.2e}" for x in d))
    assert max(d) < 2e-5, d
    assert np.abs(pcm - pcm64.numpy()).max() < 2e-6
    assert np.array_equal(st[-1][0], pcm)
    # one stage at a time gives the same arrays, and a caller that asks for none the same PCM
    assert np.array_equal(o.decode(codes, T, noise), pcm)
    if layout == "snac_tiny":
        for k in range(len(st)):
            p2, a2 = o.decode(codes, T, noise, stage=k)
            assert np.array_equal(p2, pcm) and np.array_equal(a2, st[k]), k


F16_DAC_TOL = 1e-3   # the fp16-im2col noise floor (tests/test_gpu_dac.py)
DAC_STAGE_ROWS = [
    # (id, F16 codec tensors, DacOracle f16_conv, bar per stage and for the PCM, of max|f64|)
    ("f32", False, None, 2e-5),
    ("f16_im2col", True, None, F16_DAC_TOL),
    ("f16_exact", True, 0, 2e-5),
]


@pytest.mark.parametrize("row", DAC_STAGE_ROWS, ids=[r[0] for r in DAC_STAGE_ROWS])
def test_dac_oracle_stages_match_float64(row):
    """Every stage of orc_dac_decode (0 the quantizer sum, 1 the first conv, 2 + i the end of block i) and its PCM against float64 torch_dac
    computed here, at the DAC-44k dims and 70 frames (stage lengths 70, 70, 560, 4480, 17920, 35840: many position tiles of every device
    kernel), codes np.random.default_rng(70): F32 tensors and F16 tensors read exactly (f16_conv = 0) at 2e-5 of max|f64|, the bar of the other
    oracle stages; F16 tensors with ggml's fp16 im2col (the default for them) at the fp16-im2col floor F16_DAC_TOL.  The float64 reference of
    an F16 model reads the same fp16-rounded kernels and keeps its activations in float64.

    d_ref[stage] = max|orc - f64| / max|f64| as measured, PCM absolute (tests/test_gpu_dac_stages.py derives the device's bars from this table):

        tensors              stage 0   1         2         3         4         5         PCM
        F32                  1.53e-07  4.19e-06  2.58e-06  2.64e-06  2.54e-06  2.24e-06  1.66e-06
        F16, fp16 im2col     1.34e-07  2.39e-04  3.46e-04  4.25e-04  5.06e-04  4.81e-04  3.61e-04
        F16, f16_conv = 0    1.34e-07  2.67e-06  2.32e-06  2.64e-06  2.76e-06  2.32e-06  1.74e-06

    The float64 PCM (F32 tensors): max |x| 0.65, median 0.105, nothing near saturation, so an absolute bar on the PCM means something."""
    from tts_cpp_amd import synth as sy
    name, dac_f16, f16_conv, bar = row
    frames = 70
    model = sy.build(sy.parler_mini(layers=1, prompt_vocab=64, ctx=64, dac_f16=dac_f16))
    cfg = model.cfg
    codes = np.random.default_rng(frames).integers(0, cfg.cb_size, (frames, cfg.n_out)).astype(np.uint32)
    pcm64, st64 = _make_golden().torch_dac(model, codes, stages=True)
    o = orc.DacOracle(model, f16_conv=f16_conv)
    assert o.m.f16_conv == (0 if f16_conv == 0 or not dac_f16 else 1)
    pcm, st = o.decode_stages(codes)
    assert len(st) == len(st64) == 2 + len(cfg.strides)
    assert [a.shape[1] for a in st] == [70, 70, 560, 4480, 17920, 35840]
    d = []
    for a, r in zip(st, st64):
        assert a.shape == tuple(r.shape)
        d.append(relerr(a, r.numpy()))
    d_pcm = float(np.abs(pcm - pcm64.numpy()).max())
    print(f"DAC-44k {name} F={frames}: d_ref per stage " + " ".join(f"{x:.2e}" for x in d) + f"  PCM {d_pcm:.2e} (max|pcm64| {np.abs(pcm64.numpy()).max():.3f}, "
          f"median {np.median(np.abs(pcm64.numpy())):.3f})")
    assert max(d) < bar, d
    assert d_pcm < bar * np.abs(pcm64.numpy()).max()


def test_dac_oracle_every_stage_in_one_decode(tiny_f32):
    """decode_stages (stage -2) gives the arrays of one decode per stage, and the same PCM; torch_dac's last_stage the leading stages of a whole decode"""
    g = np.load(GOLD)
    d = orc.DacOracle(tiny_f32)
    pcm, st = d.decode_stages(g["codes"])
    assert np.array_equal(pcm, d.decode(g["codes"])) and len(st) == 2 + len(tiny_f32.cfg.strides)
    for k, a in enumerate(st):
        p2, a2 = d.decode(g["codes"], stage=k)
        assert np.array_equal(p2, pcm) and np.array_equal(a2, a), k
    mg = _make_golden()
    pcm64, st64 = mg.torch_dac(tiny_f32, g["codes"], stages=True)
    assert torch.equal(mg.torch_dac(tiny_f32, g["codes"]), pcm64)
    for k in range(len(st64)):
        part = mg.torch_dac(tiny_f32, g["codes"], last_stage=k)
        assert len(part) == k + 1 and all(torch.equal(a, b) for a, b in zip(part, st64)), k


def test_orpheus_decoder_oracle_matches_torch_golden():
    """orc_orpheus_decode (Llama-3 blocks, src/models/orpheus/model.cpp:186-325 restated with ggml's NEOX rope + frequency
    factors, iterated fp32 theta) against tests/golden/tiny_orpheus.npz (float64 torch with the HF rotary formulation):
    prompt logits, 6 greedy steps through the KV cache, token ids."""
    from tts_cpp_amd import synth as sy
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_orpheus.npz"))
    model = sy.build_orpheus(sy.orpheus_tiny())
    o = orc.OrpheusOracle(model, act_mode=0)
    lg = o.decode(g["prompt"], 0)
    assert np.abs(lg - g["logits"][0]).max() < 5e-6
    pos = len(g["prompt"])
    for s_, t in enumerate(g["tokens"]):
        assert int(lg.argmax()) == int(t)
        lg = o.decode([t], pos)
        pos += 1
        assert np.abs(lg - g["logits"][s_ + 1]).max() < 5e-6
    # prefill in two pieces == one piece (cache semantics)
    o.reset()
    o.decode(g["prompt"][:4], 0)
    lg2 = o.decode(g["prompt"][4:], 4)
    assert np.abs(lg2 - g["logits"][0]).max() < 5e-6
    # Q4_0 weights (BASELINE config 4) run through the integer mul_mat
    q = orc.OrpheusOracle(sy.build_orpheus(sy.orpheus_tiny(weight_type=gguf.Q4_0)))
    assert np.isfinite(q.decode(g["prompt"], 0)).all()


# ---- Dia (src/models/dia/model.cpp) -------------------------------------------------------------------------------
def test_dia_oracle_matches_torch_golden():
    """orc_dia_encode / orc_dia_step (encoder with the real|pad block mask, cross K only for the sentence, GQA self-attention,
    unscaled softmax, NEOX rope base 10000 with iterated fp32 theta, cfg_scale map) against tests/golden/tiny_dia.npz (float64
    torch, batched, HF rotary formulation, boolean masks)."""
    from tts_cpp_amd import synth as sy
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_dia.npz"))
    model = sy.build_dia(sy.dia_tiny())
    o = orc.DiaOracle(model, act_mode=0)
    enc = o.encode(g["tokens"], int(g["sentence_len"]), want_states=True)
    assert np.abs(enc - g["enc"]).max() < 1e-5
    for s_ in range(len(g["ids"])):
        lg, raw = o.step(g["ids"][s_], s_, want_raw=True)
        assert np.abs(raw - g["raw"][s_]).max() < 1e-5
        assert np.abs(lg - g["logits"][s_]).max() < 2e-5
        assert np.array_equal(lg, raw[0] + np.float32(3.0) * (raw[0] - raw[1]))   # util.cpp:194-196, nothing masked
    # the unconditional stream does not depend on the text; the conditional one does
    o2 = orc.DiaOracle(model, act_mode=0)
    toks2, n2 = orc.dia_tokenize("[S2] something else", model.cfg.max_ctx)
    o2.encode(toks2, n2)
    _, raw2 = o2.step(g["ids"][0], 0, want_raw=True)
    assert np.abs(raw2[0] - g["raw"][0][0]).max() > 1e-2
    # pad positions see only pad positions, so the all-zero stream splits the same way: its rows >= n differ between the two texts
    q = orc.DiaOracle(sy.build_dia(sy.dia_tiny(weight_type=gguf.Q8_0)))
    q.encode(g["tokens"], int(g["sentence_len"]))
    assert np.isfinite(q.step(g["ids"][0], 0)).all()


def test_dia_tokenize():
    """tokenize_sentence :661-705"""
    t, n = orc.dia_tokenize("  hello world ", 32)
    assert bytes(t[:n].astype(np.uint8)) == b"\x01 hello world." and (t[n:] == 0).all() and t.size == 32
    t, n = orc.dia_tokenize("[S2] a [S1] b.", 32)
    assert bytes(t[:n].astype(np.uint8)) == b"\x02 a \x01 b."
    t, n = orc.dia_tokenize("[S1]x", 8)
    assert bytes(t[:n].astype(np.uint8)) == b"\x01x."


def test_dia_stopping_and_delay_pattern():
    """check_stopping :767-785 and adjust_output_tokens :787-808 on hand-made sequences"""
    from tts_cpp_amd import synth as sy
    cfg = sy.dia_tiny()
    o = orc.DiaOracle(sy.build_dia(cfg))
    NO, D = cfg.n_out, orc.DIA_DELAY_PATTERN
    # EOS on head 0 at position 5: the next 15 calls force eos / pad per head, the 15th stops
    ids = np.arange(NO, dtype=np.uint32)
    stop, out, d = o.check_stopping(ids, 4, 1000, -1)
    assert not stop and d == -1 and np.array_equal(out, ids)
    ids[0] = cfg.eos
    d = -1
    for k in range(15):
        stop, out, d = o.check_stopping(ids, 5 + k, 1000, d)
        for h in range(NO):
            want = cfg.eos if k == D[h] else (cfg.pad if k > D[h] else ids[h])
            assert out[h] == want, (k, h)
        assert d == 14 - k and stop == (k == 14)
    # the length limit triggers the same countdown at max_generation_size - max_delay
    stop, out, d = o.check_stopping(np.zeros(NO, dtype=np.uint32), 100 - 15, 100, -1)
    assert d == 14 and out[0] == cfg.eos and not stop
    stop, _, d = o.check_stopping(np.zeros(NO, dtype=np.uint32), 100 - 16, 100, -1)
    assert d == -1
    # un-delay: frame i takes head h from step i + delay[h]; a frame with any id >= audio_vocab is dropped; the last
    # max_delay steps only feed earlier frames
    steps = 20
    toks = np.zeros((steps, NO), dtype=np.uint32)
    for s_ in range(steps):
        for h in range(NO):
            toks[s_, h] = (s_ - D[h]) % cfg.audio_vocab if s_ >= D[h] else cfg.bos   # frame index carried by every head
    toks[2 + D[3], 3] = cfg.pad                                                       # spoils frame 2
    frames = o.adjust_output_tokens(toks)
    assert frames.shape == (steps - 15 - 1, NO)
    assert [int(f[0]) for f in frames] == [0, 1, 3, 4] and all((f == f[0]).all() for f in frames)


def test_dia_generate_loop_and_codec():
    """generate_from_batch :810-833 end to end on the oracle: fixed length from the generation limit, 9-head delay pattern,
    DAC on the un-delayed frames"""
    from tts_cpp_amd import synth as sy
    model = sy.build_dia(sy.dia_tiny(), suppress_special=True)
    o = orc.DiaOracle(model)
    outs, frames = o.generate("[S1] Hi there [S2] ok")
    cfg = model.cfg
    assert outs.shape == (cfg.max_gen - 1, cfg.n_out)               # limit hit at max_gen - 15, then 14 more decodes
    assert frames.shape == (cfg.max_gen - 1 - cfg.max_delay, cfg.n_out) and frames.max() < cfg.audio_vocab
    for h, dl in enumerate(orc.DIA_DELAY_PATTERN):
        assert np.array_equal(frames[:, h], outs[dl:dl + len(frames), h])
    outs2, _ = o.generate("[S1] Hi there [S2] ok", max_tokens=24)    # config.max_tokens (:812-818)
    assert outs2.shape == (23, cfg.n_out) and np.array_equal(outs2[:8], outs[:8])
    pcm = orc.DacOracle(model.dac).decode(frames)
    assert pcm.shape == (len(frames) * cfg.hop,) and np.isfinite(pcm).all() and np.abs(pcm).max() <= 1.0


# ---- Kokoro (src/models/kokoro/model.cpp; oracle/kokoro_oracle.c, parity unpinned: see its header) -------------------------
def _kokoro_case(gelu_mode=0):
    """gelu_mode 0: fp32 tanh-GELU like the float64 torch fixture (the product semantics, ggml's fp16 table, is mode 1)"""
    from tts_cpp_amd import synth as sy
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_kokoro.npz"))
    model = sy.build_kokoro(sy.kokoro_tiny())
    o = orc.KokoroOracle(model, gelu_mode=gelu_mode)
    total = int(g["lens"].sum())
    noise = np.random.default_rng(int(g["noise_seed"])).random(9 * 50 * model.cfg.up_sampling_factor, dtype=np.float32)[:o.noise_len(total)]
    return g, model, o, noise


def test_kokoro_duration_graph_matches_torch_golden():
    """ALBERT (one shared layer applied `recurrence` times, eps 1e-12 norms, fixed 0.125 softmax scale), the prosody predictor's
    bidirectional LSTM + AdaLayerNorm stack and the duration head against float64 torch (nn.LSTM, F.layer_norm)."""
    g, model, o, _ = _kokoro_case()
    lens, hid = o.durations(g["tokens"], "af_test")
    assert np.array_equal(lens, g["lens"]) and len(set(lens.tolist())) > 1
    assert np.abs(hid - g["hidden"]).max() < 2e-5
    lens_b, hid_b = o.durations(g["tokens"], "bm_test")           # the voice row (n_tokens - 3) conditions the predictor
    assert np.abs(hid_b - hid).max() > 1e-2


def test_kokoro_generation_graph_matches_torch_golden():
    """alignment, shared LSTM, F0 / N branches (AdaIN residual blocks with the depthwise transposed-conv pool and the nearest-
    neighbour shortcut), text encoder, decoder blocks, harmonic source, STFT conditioning, generator and iSTFT head against float64
    torch (F.instance_norm, F.conv_transpose1d(groups, output_padding), F.interpolate, torch.stft / istft)."""
    g, model, o, noise = _kokoro_case()
    cfg = model.cfg
    pcm, f0, nn_, hs = o.generate(g["tokens"], g["lens"], g["hidden"], "af_test", noise, want_curves=True, hsrc_in=g["hsrc"])
    assert np.abs(f0 - g["f0"]).max() < 1e-4 * np.abs(g["f0"]).max() and np.abs(nn_ - g["n"]).max() < 1e-4
    assert (g["f0"] > 10).any() and (g["f0"] <= 10).any()       # voiced and unvoiced stretches both occur
    # the oracle's own STFT conditioning: fp32 phases of ~1e4 rad limit the source to ~1e-3, compared as complex numbers because the
    # phase channels wrap at +-pi
    nb = cfg.n_fft // 2 + 1
    za, zb = hs[:nb] * np.exp(1j * hs[nb:]), g["hsrc"][:nb] * np.exp(1j * g["hsrc"][nb:])
    assert np.abs(za - zb).max() < 1e-2 * np.abs(zb).max()
    # everything after the conditioning, sample for sample
    assert pcm.shape == g["pcm"].shape == (int(g["lens"].sum()) * cfg.up_sampling_factor,)
    assert np.abs(pcm - g["pcm"]).max() < 5e-5 * np.abs(g["pcm"]).max()


def test_kokoro_albert_gelu_through_the_fp16_table():
    """ggml_gelu on the CPU goes through a table indexed by the fp16 bits of x (kokoro/model.cpp:1000): the default oracle mode follows it —
    close to, but not equal to, the fp32 evaluation"""
    g, model, o0, _ = _kokoro_case(0)
    _, _, o1, _ = _kokoro_case(1)
    l0, h0 = o0.durations(g["tokens"], "af_test")
    l1, h1 = o1.durations(g["tokens"], "af_test")
    d = np.abs(h1 - h0).max()
    assert 0 < d < 5e-3 * np.abs(h0).max()


def test_kokoro_forced_durations_and_noise():
    """BASELINE's Kokoro configuration forces the durations for shape determinism: any integer lengths drive the same graph"""
    g, model, o, _ = _kokoro_case()
    cfg = model.cfg
    lens = np.array([1, 4, 2, 1, 3, 2, 5, 1], dtype=np.float32)
    total = int(lens.sum())
    rng = np.random.default_rng(3)
    n1, n2 = rng.random(o.noise_len(total), dtype=np.float32), rng.random(o.noise_len(total), dtype=np.float32)
    a = o.generate(g["tokens"], lens, g["hidden"], "af_test", n1)
    b = o.generate(g["tokens"], lens, g["hidden"], "af_test", n2)
    assert a.shape == (total * cfg.up_sampling_factor,) and np.isfinite(a).all()
    assert 1e-6 < np.abs(a - b).max()                            # the source noise reaches the audio
    assert np.array_equal(a, o.generate(g["tokens"], lens, g["hidden"], "af_test", n1))


def test_snake_sine_polynomial_is_libm_accurate():
    """csrc/dac_kernels.h snake_sin (4-term Cody-Waite reduction by pi + degree-9 odd polynomial, |x| < 125) restated in numpy float32
    with exact fused multiply-adds: against float64 sin its error stays within 2 ulp / 1.5e-7 absolute — the class of libm's sinf, which
    the reference's snake_1d calls (src/util.cpp:96-101)."""
    f = np.float32

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)

    def snake_sin(x):
        q = np.rint((x * f(0.318309886183790671537767526745028724)).astype(f)).astype(f)
        r = x
        for cst in (-3.140625, -0.0009670257568359375, -6.2771141529083251953e-07, -1.2154201256553420762e-10):
            r = fma(q, np.full_like(x, f(cst)), r)
        s = (r * r).astype(f)
        r = np.where(q.astype(np.int64) & 1, -r, r).astype(f)
        u = np.full_like(x, f(2.6083159809786593541503e-06))
        for cst in (-0.0001981069071916863322258, 0.00833307858556509017944336, -0.166666597127914428710938):
            u = fma(u, s, np.full_like(x, f(cst)))
        return fma(s, (u * r).astype(f), r)

    rng = np.random.default_rng(0)
    for lo, hi in ((-125, 125), (-10, 10), (-1, 1)):
        x = rng.uniform(lo, hi, 1_000_000).astype(f)
        ref = np.sin(x.astype(np.float64))
        err = np.abs(snake_sin(x).astype(np.float64) - ref)
        assert err.max() < 1.5e-7
        assert (err / np.spacing(np.abs(ref).astype(f)).astype(np.float64)).max() < 2.5


def test_device_sampler_key_order_restatement():
    """numpy restatement of smp_key / smp_key_value (csrc/parler_kernels.h, llama_kernels.h): the 64-bit keys the device samplers sort —
    ~monotone(value) << 32 | index — order candidates by value descending, equal values by index ascending (the total order the tests
    hold the reference's std::sort to wherever it is specified), -0 and +0 compare equal, and the value field inverts exactly."""
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(5000) * 7).astype(np.float32)
    v[:50] = np.float32([0.0, -0.0] * 25)
    v[50:60] = v[60:70]                      # exact ties
    v[70], v[71] = np.float32(np.inf), np.float32(-np.inf)
    idx = np.arange(v.size, dtype=np.uint64)

    def key(val, i):
        val = np.where(val == 0.0, np.float32(0.0), val).astype(np.float32)
        u = val.view(np.uint32).astype(np.uint64)
        u = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
        return (((~u) & 0xFFFFFFFF) << np.uint64(32)) | i

    def value(k):
        u = (~(k >> np.uint64(32))) & np.uint64(0xFFFFFFFF)
        bits = np.where(u & 0x80000000, u & 0x7FFFFFFF, (~u) & 0xFFFFFFFF).astype(np.uint32)
        return bits.view(np.float32)

    k = key(v, idx)
    order = np.argsort(k, kind="stable")
    ref = np.lexsort((idx, -np.where(v == 0.0, np.float32(0.0), v).astype(np.float64)))
    assert np.array_equal(order, ref)
    back = value(k)
    assert np.array_equal(back, np.where(v == 0.0, np.float32(0.0), v))


def _bf16_rne(x):
    """float32 -> bf16 (round to nearest even), returned as float32 (what v_cvt_pk_bf16_f32 does)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def _split_bf16x3(x):
    x = np.asarray(x, dtype=np.float32)
    h1 = _bf16_rne(x)
    r1 = x - h1
    h2 = _bf16_rne(r1)
    h3 = _bf16_rne(r1 - h2)
    return h1, h2, h3


def test_bf16x3_split_is_fp32_accurate():
    """The arithmetic of the off-by-default conv1d_mfma_b3_kernel (csrc/dac_kernels.h): fp32 operands as three bf16
    terms, six products, fp32 accumulation per 16-deep MFMA step.  The split itself is exact to 24 bits, the six
    terms leave 1e-8, and the sum's error is that of an fp32 accumulation — not larger than the fp32 MFMA chain's."""
    rng = np.random.default_rng(0)
    K = 7 * 192
    A = (rng.standard_normal((64, K)) * 0.05).astype(np.float32)
    B = rng.standard_normal((K, 128)).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    a, b = _split_bf16x3(A), _split_bf16x3(B)
    assert np.array_equal((a[0].astype(np.float64) + a[1] + a[2]).astype(np.float32), A)
    terms = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]
    exact6 = sum(a[i].astype(np.float64) @ b[j].astype(np.float64) for i, j in terms)
    assert np.abs(exact6 - ref).max() / np.abs(ref).max() < 5e-8
    acc = np.zeros((64, 128), np.float32)
    chain = np.zeros((64, 128), np.float32)
    for k in range(0, K, 16):
        for i, j in terms:      # one 32x32x16 bf16 MFMA each: exact products, fp32 accumulate
            acc = acc + (a[i][:, k:k + 16].astype(np.float64) @ b[j][k:k + 16].astype(np.float64)).astype(np.float32)
    for k in range(0, K, 2):    # the 32x32x2 fp32 MFMA chain of conv1d_mfma_kernel
        chain = chain + (A[:, k:k + 2].astype(np.float64) @ B[k:k + 2].astype(np.float64)).astype(np.float32)
    e_b3 = np.abs(acc - ref).max() / np.abs(ref).max()
    e_f32 = np.abs(chain - ref).max() / np.abs(ref).max()
    assert e_b3 < 2e-6 and e_b3 < 2 * e_f32, (e_b3, e_f32)


def test_fp16_hi_lo_split_three_products_is_near_fp32_accurate():
    """The arithmetic of the codec's default since round 6 (csrc/dac_kernels.h SplitH2): an fp32 operand as h = fp16(x), l = fp16(x - h) — x - h is exact
    in fp32 and, for small x, an fp16 SUBNORMAL that v_mfma_f32_32x32x16_f16 multiplies exactly (profiles/mfma_denorm.hip) —, three products
    h h' + h l' + l h' (each exact in fp32), fp32 accumulation per 16-deep MFMA step.  The operand is represented to 2^-22 relative (or 2^-25 absolute),
    the dropped l l' term is 2^-22 of a product; the sum's error stays that of an fp32 accumulation (VERDICT r5 item 2's decision rule: ~2^-22 per
    product).  fp16's exponent range ends at 2^-14 (2^-24 subnormal), so an operand below 0.25 keeps 2^-25 ABSOLUTE rather than 2^-22 relative: weights
    of the codec's magnitude (0.05) and activations around 1 — the case the kernels meet — and, as the stress case, both spread over five decades."""
    rng = np.random.default_rng(0)
    K = 7 * 192
    A = (rng.standard_normal((64, K)) * 0.05).astype(np.float32)
    B = rng.standard_normal((K, 128)).astype(np.float32)
    As = (A * 10.0 ** rng.uniform(-4, 0, A.shape)).astype(np.float32)
    Bs = (B * 10.0 ** rng.uniform(-4, 1, B.shape)).astype(np.float32)

    def split(x):
        h = x.astype(np.float16)
        l = (x - h.astype(np.float32)).astype(np.float16)
        return h, l
    (sh, sl), (th, tl) = split(As), split(Bs)
    assert (np.abs(sl[np.abs(As) < 1e-3]) < 2.0 ** -14).any() and (sl != 0).any()   # fp16 subnormals are exercised
    stress = np.abs(sum(a.astype(np.float64) @ b.astype(np.float64) for a, b in [(sl, th), (sh, tl), (sh, th)]) - As.astype(np.float64) @ Bs.astype(np.float64)).max()
    e_stress = stress / np.abs(As.astype(np.float64) @ Bs.astype(np.float64)).max()
    assert e_stress < 3e-6, e_stress         # five decades of operand magnitudes: still below the stage bar of the GPU tests (1e-5)
    (ah, al), (bh, bl) = split(A), split(B)
    rep = np.abs((ah.astype(np.float64) + al.astype(np.float64)) - A).max() / np.abs(A).max()
    assert rep < 2.0 ** -21
    ref = A.astype(np.float64) @ B.astype(np.float64)
    terms = [(al, bh), (ah, bl), (ah, bh)]   # smallest first, as SplitH2::ta / tb
    exact3 = sum(a.astype(np.float64) @ b.astype(np.float64) for a, b in terms)
    e3 = np.abs(exact3 - ref).max() / np.abs(ref).max()
    assert e3 < 4e-7, e3                     # the three terms alone
    acc = np.zeros((64, 128), np.float32)
    chain = np.zeros((64, 128), np.float32)
    for k in range(0, K, 16):
        for a, b in terms:      # one 32x32x16 f16 MFMA each: exact products, fp32 accumulate
            acc = acc + (a[:, k:k + 16].astype(np.float64) @ b[k:k + 16].astype(np.float64)).astype(np.float32)
    for k in range(0, K, 2):    # the 32x32x2 fp32 MFMA chain of conv1d_mfma_kernel
        chain = chain + (A[:, k:k + 2].astype(np.float64) @ B[k:k + 2].astype(np.float64)).astype(np.float32)
    e_h2 = np.abs(acc - ref).max() / np.abs(ref).max()
    e_f32 = np.abs(chain - ref).max() / np.abs(ref).max()
    print(f"three-term representation {e3:.2e} (operands over five decades: {e_stress:.2e}); accumulated: fp16 hi+lo {e_h2:.2e}, exact-fp32 chain {e_f32:.2e}")
    assert e_h2 < 2e-6 and e_h2 < 3 * e_f32 + 3e-7, (e_h2, e_f32)


def test_bf16x3_conv_layout_restatement():
    """Index arithmetic of conv1d_mfma_b3_kernel / pack_conv_w_b3_kernel restated in numpy: packed weight image
    [chunk][plane][s][hi][co][8], input image [plane][position][8], half-wave hi takes tap 2s + hi (the eighth tap has
    zero weights and reads tap 6's rows), MFMA fragments A[i = lane & 31][k = 8 hi + e], B[k][j = lane & 31]."""
    rng = np.random.default_rng(1)
    cout, cin, L, dil, CO_T, T_T = 64, 24, 150, 3, 64, 64
    pad = 3 * dil
    w = (rng.standard_normal((cout, cin, 7)) * 0.1).astype(np.float32)
    x = rng.standard_normal((cin, L)).astype(np.float32)
    n_chunks = (cin + 7) // 8
    packed = np.zeros((n_chunks, 3, 4, 2, CO_T, 8), np.float32)       # pack_conv_w_b3_kernel (one co tile)
    for ch in range(n_chunks):
        for st in range(4):
            for hi in range(2):
                tap = 2 * st + hi
                for j in range(8):
                    ci = ch * 8 + j
                    v = w[:, ci, tap] if (ci < cin and tap < 7) else np.zeros(cout, np.float32)
                    for pl, h in enumerate(_split_bf16x3(v)):
                        packed[ch, pl, st, hi, :, j] = h
    xw = T_T + 6 * dil
    out = np.zeros((cout, L), np.float64)
    for t0 in range(0, L, T_T):
        acc = np.zeros((CO_T // 32, T_T // 32, 32, 32), np.float64)
        for ch in range(n_chunks):
            img = np.zeros((3, xw, 8), np.float32)                    # commit(): [plane][position][8 channels]
            for p in range(xw):
                t = t0 + p - pad
                for e in range(8):
                    ci = ch * 8 + e
                    v = x[ci, t] if (ci < cin and 0 <= t < L) else np.float32(0)
                    for pl, h in enumerate(_split_bf16x3(np.array([v], np.float32))):
                        img[pl, p, e] = h[0]
            for st in range(4):
                for i in range(CO_T // 32):
                    for jt in range(T_T // 32):
                        A = np.zeros((3, 32, 16), np.float32)
                        B = np.zeros((3, 16, 32), np.float32)
                        for hi in range(2):
                            tap = min(2 * st + hi, 6)
                            for l31 in range(32):
                                for pl in range(3):
                                    A[pl, l31, 8 * hi:8 * hi + 8] = packed[ch, pl, st, hi, i * 32 + l31]
                                    B[pl, 8 * hi:8 * hi + 8, l31] = img[pl, jt * 32 + l31 + tap * dil]
                        for pa, pb in [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]:
                            acc[i, jt] += A[pa].astype(np.float64) @ B[pb].astype(np.float64)
        for i in range(CO_T // 32):
            for jt in range(T_T // 32):
                t_lo = t0 + jt * 32
                n = max(0, min(32, L - t_lo))
                out[i * 32:(i + 1) * 32, t_lo:t_lo + n] = acc[i, jt][:, :n]
    ref = np.zeros((cout, L), np.float64)
    xp = np.pad(x.astype(np.float64), ((0, 0), (pad, pad)))
    for k in range(7):
        ref += np.einsum("oc,cl->ol", w[:, :, k].astype(np.float64), xp[:, k * dil:k * dil + L])
    assert np.abs(out - ref).max() / np.abs(ref).max() < 1e-7


def test_accumulators_as_b_fragments_restatement():
    """Design check for DESIGN §8 'round 3' item 2 (the k = 1 conv of a 96-channel residual unit inside the k = 7
    kernel's epilogue): with v_mfma_f32_32x32x2_f32 the result D[row][col] of tile i sits in lane (col, hi), register e
    with row = (e & 3) + 8 (e >> 2) + 4 hi; taking the reduction step of the second GEMM as (i, e) and its two k values
    as hi, every lane's own register IS its B fragment (B[k = hi][j = col]) and the weights only need the matching
    permutation.  No cross-lane movement: checked here against a plain matrix product."""
    rng = np.random.default_rng(3)
    C, T = 96, 32
    s1 = rng.standard_normal((C, T)).astype(np.float32)           # snake(conv7 + bias): what the accumulators hold
    w2 = (rng.standard_normal((C, C)) * 0.1).astype(np.float32)   # k = 1 conv weights [co][ci]
    # accumulator image: acc[i][lane = (col, hi)][e]
    acc = np.zeros((C // 32, 32, 2, 16), np.float32)
    for i in range(C // 32):
        for e in range(16):
            for hi in range(2):
                acc[i, :, hi, e] = s1[32 * i + (e & 3) + 8 * (e >> 2) + 4 * hi, :]
    out = np.zeros((C, T), np.float64)
    for i2 in range(C // 32):                                      # output tile of the second GEMM
        D = np.zeros((32, 32), np.float64)
        for i in range(C // 32):
            for e in range(16):                                    # one MFMA: K = 2 (hi = 0, 1)
                A = np.zeros((32, 2), np.float32)
                B = np.zeros((2, 32), np.float32)
                for hi in range(2):
                    ci = 32 * i + (e & 3) + 8 * (e >> 2) + 4 * hi
                    A[:, hi] = w2[32 * i2:32 * i2 + 32, ci]        # lane (row, hi) reads the permuted weight image
                    B[hi, :] = acc[i, :, hi, e]                    # the lane's own register
                D += A.astype(np.float64) @ B.astype(np.float64)
        out[32 * i2:32 * i2 + 32] = D
    ref = w2.astype(np.float64) @ s1.astype(np.float64)
    assert np.abs(out - ref).max() < 1e-12


def test_streaming_integer_gemm_two_blocks_per_mfma_restatement():
    """qgemv_stream_kernel (gemv_stream_kernels.h, round 6) restated in numpy: a lane's 16 bytes are the A operand of v_mfma_i32_16x16x64_i8, whose 64
    columns are TWO Q8_0 blocks (lane groups 0, 1 hold the even block, groups 2, 3 the odd one).  Two MFMAs per span with the other block's lane groups
    reading a row of zeros give the two exact block dots; the LDS image of the rows is XOR-swizzled by the row (16-byte piece p of row r at piece
    p ^ (r & 15)), the last tile of an N that is no multiple of 16 re-reads feature N - 1, K slices leave slabs folded in slab order — and the result is
    ggml_vec_dot_q8_0_q8_0's sum over blocks of (float) sumi * (d_w * d_a), block after block, in fp32."""
    rng = np.random.default_rng(6)
    R, N, K, ks = 7, 37, 1024, 2                      # 7 rows (the 8-row image), 37 features (3 tiles, the last one 5 wide), two K slices of two chunks
    KS, nb, RS = K // ks, K // 32, 8
    W = rng.integers(-127, 128, (N, K)).astype(np.int8)
    wd = (rng.random((N, nb)) * 0.02 + 0.001).astype(np.float16)
    aq = rng.integers(-127, 128, (R, K)).astype(np.int8)
    ad = (rng.random((R, nb)) * 0.05 + 0.001).astype(np.float32)
    # reference: block after block
    ref = np.zeros((R, N), np.float32)
    for b in range(nb):
        sumi = aq[:, b * 32:(b + 1) * 32].astype(np.int32) @ W[:, b * 32:(b + 1) * 32].astype(np.int32).T
        ref = (ref + sumi.astype(np.float32) * (ad[:, b:b + 1] * wd[:, b].astype(np.float32)[None, :]).astype(np.float32)).astype(np.float32)

    def mfma_16x16x64(a_lanes, b_lanes):          # a_lanes / b_lanes [64 lanes][16 bytes]: D[i][j] = sum over lane groups g and the 16 bytes of A[i, g] * B[j, g]
        d = np.zeros((16, 16), np.int64)
        for g in range(4):
            d += a_lanes[g * 16:(g + 1) * 16].astype(np.int64) @ b_lanes[g * 16:(g + 1) * 16].astype(np.int64).T
        return d                                   # lane (li, g) ends with D[4 g + e][li], e = 0 .. 3

    slabs = np.zeros((ks, 16, N), np.float32)
    for kz in range(ks):
        k0 = kz * KS
        # the LDS image of this slice: [RS + 1][KS] bytes, rows >= R repeat row R - 1, row RS zeros, pieces swizzled
        xs = np.zeros((RS + 1, KS), np.int8)
        for r in range(RS):
            src = aq[min(r, R - 1), k0:k0 + KS].reshape(KS // 16, 16)
            for cv in range(KS // 16):
                blk, pc = divmod(cv, 16)
                xs[r, (blk * 16 + (pc ^ (r & 15))) * 16:][:16] = src[cv]
        for t in range((N + 15) // 16):
            acc = np.zeros((16, 16), np.float32)   # [feature of the tile][row li]
            for ch in range(KS // 256):
                for c in range(4):                  # a 64-column span = blocks 2 c and 2 c + 1 of the chunk
                    a_l = np.zeros((64, 16), np.int8); be = np.zeros((64, 16), np.int8); bo = np.zeros((64, 16), np.int8)
                    for lane in range(64):
                        li, g = lane & 15, lane >> 4
                        a_l[lane] = W[min(t * 16 + li, N - 1), k0 + ch * 256 + c * 64 + g * 16:][:16]
                        row = li & (RS - 1)
                        off = ch * 256 + (((c * 4 + g) ^ (row & 15)) << 4)
                        be[lane] = xs[row if g < 2 else RS, off:off + 16]
                        bo[lane] = xs[RS if g < 2 else row, off:off + 16]
                    ze, zo = mfma_16x16x64(a_l, be), mfma_16x16x64(a_l, bo)
                    for which, z in ((0, ze), (1, zo)):
                        b = (k0 >> 5) + ch * 8 + 2 * c + which
                        # the block dot is exact and only this block's
                        feats = np.minimum(t * 16 + np.arange(16), N - 1)
                        want = W[feats, b * 32:(b + 1) * 32].astype(np.int64) @ aq[np.minimum(np.arange(16) & (RS - 1), R - 1), b * 32:(b + 1) * 32].astype(np.int64).T
                        assert np.array_equal(z, want)
                        dw = wd[feats, b].astype(np.float32)[:, None]
                        da = ad[np.minimum(np.arange(16) & (RS - 1), R - 1), b][None, :]
                        acc = (acc + z.astype(np.float32) * (dw * da).astype(np.float32)).astype(np.float32)
            for f in range(16):
                if t * 16 + f < N:
                    slabs[kz, :, t * 16 + f] = acc[f]
    out = slabs[0].copy()
    for kz in range(1, ks):
        out = (out + slabs[kz]).astype(np.float32)
    # two K slices: the same terms in k order inside a slice, associated as (slice 0) + (slice 1): equal up to the fp32 rounding of the partial sums
    # (one slice is ggml's order exactly)
    assert np.abs(out[:R] - ref).max() <= 4e-7 * np.abs(ref).max()


@pytest.mark.parametrize("dims", ["tiny", "dac44k"])
def test_fp16_im2col_reading_of_an_f32_codec_model(dims):
    """upstream ggml_conv_1d always goes through an F16 im2col (general_neural_audio_codec.cpp:142,146, dac_model.cpp:158,164), so
    an F32 codec model can be read two ways: exact fp32 (what the HIP path and oracle reading 0 do) or with the inputs and kernels of the plain convs
    rounded to fp16 (oracle reading 2; transposed convs with an F32 kernel stay exact).  The fork's ggml is absent, so which one it does is unknowable here;
    this test puts the NUMBER on it: max |PCM(0) - PCM(2)| on the same model and codes, at tiny and at DAC-44k dims (DESIGN.md parity table)."""
    if dims == "tiny":
        model = synth.build(synth.tiny(weight_type=gguf.F32))
        frames = 12
    else:
        model = synth.build(synth.tiny(weight_type=gguf.F32, n_out=9, latent=1024, cb_size=1024, c0=1536, strides=(8, 8, 4, 2), layers=1))
        frames = 6
    cfg = model.cfg
    codes = np.random.default_rng(11).integers(0, cfg.cb_size, (frames, cfg.n_out)).astype(np.uint32)
    exact = orc.DacOracle(model, f16_conv=0).decode(codes)
    im2col16 = orc.DacOracle(model, f16_conv=2).decode(codes)
    d = float(np.abs(exact - im2col16).max())
    rms = float(np.sqrt(np.mean((exact - im2col16) ** 2)))
    print(f"{dims}: max |PCM(fp32 reading) - PCM(fp16-im2col reading)| = {d:.3e} (rms {rms:.3e}), max |PCM| = {np.abs(exact).max():.3f}")
    assert d > 1e-6          # the two readings are different functions ...
    assert d < 5e-3, d       # ... about an fp16 rounding per conv apart: the bound DESIGN.md quotes
