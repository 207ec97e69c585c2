"""GPU: the forms of gemm_tile_kernel of which two workgroups fit one CU (tune("tile_pair"), csrc/shim_decoder.hip: launch_tile_shape).
tile_pair = 1: 128 x 128 tiles with two 64-wide LDS buffers (64 KB), 128 x 64 with three (72 KB), the smaller shapes with four (no 128-wide "deep" form);
tile_pair = 2: the same, and a 128 x 128 choice takes 128 x 64 tiles.  A form changes how many k-tiles are in flight and which workgroup owns an output
element, never the element's own sum (32-wide MFMA steps in ascending k): every epilogue must leave the SAME BITS as the current forms.

One GEMM at a time through tts_hip_debug_tile_gemm on random fp16 operands, the tile shape forced (tile_force) so that the small problems take the
big tiles: R = 33, 64, 130, 192 rows (a ragged last row tile at every shape), K = 256, 512 (more k-tiles than buffers: 4 and 8 of 64), N = 128, 192
features (QKV: H = 128, two heads, N = 384; the cross-attention fold: H = N, 2 and 3 heads).  Then a tiny model's greedy loop on two contexts that
share one arena and run side by side: the tokens of the current forms (tile_pair = 0) under every value of the key.

Which forms the default (tile_pair = -1) launches is read back, not inferred from the results (they are the same bits either way): debug_read("tile_pair")
gives the value the launches ran under and the most LDS a tiled launch asked for.  A context alone on its arena keeps today's forms (96 KB deep 64 x 64
tile, 128 KB 128 x 128 tile); a context whose arena another context reads takes the forms of 1 (at most 72 KB); the choice is made at the first tiled
launch and kept until tune("tile_pair") asks again."""
import threading

import numpy as np
import pytest

from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

EPI_STORE, EPI_QKV, EPI_RESID, EPI_GELU, EPI_CROSS = range(5)
ROWS = (33, 64, 130, 192)
KS = (256, 512)
NS = (128, 192)


@pytest.fixture(scope="module")
def model():
    return synth.build(synth.tiny(weight_type=gguf.F16))


@pytest.fixture(scope="module")
def eng(model):
    """one loaded tiny context for every GEMM of this file (the entry uses its stream and its tile keys only)"""
    e = hip.HipEngine(model.cfg, max_seqs=1)
    e.load(model)
    yield e
    e.close()


def _operands(epi, R, K, N):
    rng = np.random.default_rng(epi * 100003 + R * 1009 + K * 7 + N)
    H = 128 if epi == EPI_QKV else N
    n = 3 * H if epi == EPI_QKV else N
    W = (rng.standard_normal((n, K)) / np.sqrt(K)).astype(np.float16)
    A = rng.standard_normal((R, K)).astype(np.float16)
    kw = {}
    if epi == EPI_RESID:
        kw["resid"] = rng.standard_normal((R, n)).astype(np.float32)
    if epi == EPI_CROSS:
        kw["cross_kv"] = rng.standard_normal((2, 27, H)).astype(np.float32)   # 27 voice-prompt positions: past one 16-group of scores
    return W, A, H, kw


def _run(eng, epi, W, A, H, kw, force, deep, pair):
    eng.tune("tile_force", force)
    eng.tune("tile_deep", deep)
    eng.tune("tile_pair", pair)
    out, out2 = eng.debug_tile_gemm(epi, W, A, H, **kw)
    assert np.isfinite(out).all() and np.abs(out).max() > 0
    return out, out2


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        if x is None:
            assert y is None
            continue
        diff = np.flatnonzero(x.view(np.uint8).ravel() != y.view(np.uint8).ravel())
        assert diff.size == 0, f"{what}: {diff.size} bytes differ, first at byte {diff[0]} of an output of shape {x.shape}"


@pytest.mark.parametrize("epi", [EPI_STORE, EPI_QKV, EPI_RESID, EPI_GELU], ids=["store", "qkv", "resid", "gelu"])
def test_two_per_cu_forms_leave_the_same_bits(epi, eng):
    try:
        for R in ROWS:
            for K in KS:
                for N in NS:
                    W, A, H, kw = _operands(epi, R, K, N)
                    ref = _run(eng, epi, W, A, H, kw, 5, 1, 0)                       # 128 x 128, four buffers: today's qkv / fc1 form
                    if epi == EPI_QKV:   # the cache append went to the rows' own positions only
                        kv = ref[1]
                        for r in range(R):
                            assert np.abs(kv[:, r, r % 3]).max() > 0 and not kv[:, r, [p for p in range(3) if p != r % 3]].any()
                    for force, pair in ((5, 1), (5, 2), (4, 0), (4, 1), (4, 2), (3, 0), (3, 1)):
                        got = _run(eng, epi, W, A, H, kw, force, 1, pair)
                        _same_bits(ref, got, f"epi {epi} R={R} K={K} N={N} tile_force={force} tile_pair={pair}")
    finally:
        eng.tune("tile_force", -1); eng.tune("tile_pair", -1); eng.tune("tile_deep", 1)


def test_cross_attention_fold_under_the_two_per_cu_forms(eng):
    """the fold lives in the 64 x 64 tile: 128-wide k-tiles / three buffers today, 64-wide / four buffers under tile_pair (and under tile_deep = 0)"""
    try:
        for R in ROWS:
            for K in KS:
                for N in NS:
                    W, A, H, kw = _operands(EPI_CROSS, R, K, N)
                    ref = _run(eng, EPI_CROSS, W, A, H, kw, 3, 1, 0)
                    for deep, pair in ((0, 0), (1, 1), (1, 2)):
                        got = _run(eng, EPI_CROSS, W, A, H, kw, 3, deep, pair)
                        _same_bits(ref, got, f"cross fold R={R} K={K} H={N} tile_deep={deep} tile_pair={pair}")
    finally:
        eng.tune("tile_force", -1); eng.tune("tile_pair", -1); eng.tune("tile_deep", 1)


def test_only_the_built_forms_are_accepted(eng):
    for v in (-2, 3, 8):
        with pytest.raises(hip.HipError):
            eng.tune("tile_pair", v)
    for v in (2, 1, 0, -1):   # -1, the default: by arena sharing
        eng.tune("tile_pair", v)


KB = 1024


def _forms(e):
    """(tile_pair the tiled launches ran under, most LDS in bytes one of them asked for since tune("tile_pair"))"""
    v = e.debug_read("tile_pair", 2)
    return int(v[0]), int(v[1])


def _one_gemm(e, force):
    W, A, H, kw = _operands(EPI_STORE, 64, 256, 128)
    e.tune("tile_force", force)
    return e.debug_tile_gemm(EPI_STORE, W, A, H, **kw)


def test_the_default_goes_by_arena_sharing(eng, model):
    try:
        eng.tune("tile_deep", 1); eng.tune("tile_pair", -1)
        assert _forms(eng) == (-1, 0)                       # nothing launched yet: nothing decided
        ref3 = _one_gemm(eng, 3)
        assert _forms(eng) == (0, 96 * KB)                  # alone: the deep 64 x 64 form, three 128-wide buffers
        ref5 = _one_gemm(eng, 5)
        assert _forms(eng) == (0, 128 * KB)                 # alone: 128 x 128 with four buffers
        b = hip.HipEngine(model.cfg, max_seqs=1)
        try:
            b.load(model, declare_only=True, external_arena=eng.arena_ptr())
            b.arena_filled()
            assert _forms(b) == (-1, 0)
            _same_bits(ref3, _one_gemm(b, 3), "sharing context, 64 x 64")
            assert _forms(b) == (1, 64 * KB)                # its arena has two readers: four 64-wide buffers
            _same_bits(ref5, _one_gemm(b, 5), "sharing context, 128 x 128")
            assert _forms(b) == (1, 64 * KB)                # two 64-wide buffers
            _one_gemm(b, 4)
            assert _forms(b) == (1, 72 * KB)                # 128 x 64 with three
            _one_gemm(eng, 5)
            assert _forms(eng) == (0, 128 * KB)             # decided before b attached: kept (its captured steps hold those kernels)
            eng.tune("tile_pair", -1)                       # asks again
            _same_bits(ref5, _one_gemm(eng, 5), "owner after the second context attached")
            assert _forms(eng) == (1, 64 * KB)
            eng.tune("tile_pair", 0); _one_gemm(eng, 5)
            assert _forms(eng) == (0, 128 * KB)             # the key forces either choice whatever the arena says
        finally:
            b.close()
        eng.tune("tile_pair", 1); _one_gemm(eng, 5)
        assert _forms(eng) == (1, 64 * KB)
        eng.tune("tile_pair", -1); _one_gemm(eng, 5)
        assert _forms(eng) == (0, 128 * KB)                 # alone again
    finally:
        eng.tune("tile_force", -1); eng.tune("tile_pair", -1); eng.tune("tile_deep", 1)


def _greedy_pair(model, rows, steps, tune):
    """two contexts on one arena, their greedy loops side by side -> the tokens of each, and under "forms" what _forms read from each afterwards"""
    cfg = model.cfg
    a = hip.HipEngine(cfg, max_seqs=rows, kv_positions=8 + steps, tune=tune)
    a.load(model)
    b = hip.HipEngine(cfg, max_seqs=rows, kv_positions=8 + steps, tune=tune)
    b.load(model, declare_only=True, external_arena=a.arena_ptr())
    b.arena_filled()
    out = {}

    def work(key, eng, seed):
        rng = np.random.default_rng(seed)
        prompts = [rng.integers(3, cfg.prompt_vocab, 4).astype(np.uint32) for _ in range(rows)]
        eng.prefill_batch(prompts)
        out[key] = eng.generate_greedy([4] * rows, steps)[0]

    ths = [threading.Thread(target=work, args=(k, e, s)) for k, e, s in (("a", a, 11), ("b", b, 12))]
    for t in ths: t.start()
    for t in ths: t.join()
    out["forms"] = (_forms(a), _forms(b))
    b.close(); a.close()
    assert set(out) == {"a", "b", "forms"}
    return out


@pytest.mark.parametrize("force", [-1, 5], ids=["cost-model-tiles", "128x128-tiles"])
def test_greedy_tokens_of_two_contexts_on_one_arena(force, model):
    rows, steps = 130, 8
    ref = _greedy_pair(model, rows, steps, {"tile_force": force, "tile_pair": 0})
    assert not np.array_equal(ref["a"], ref["b"])   # the two contexts were given different prompts
    assert [f[0] for f in ref["forms"]] == [0, 0]
    if force == 5:
        assert [f[1] for f in ref["forms"]] == [128 * KB] * 2
    for pair in (-1, 1, 2):   # -1, the default: both contexts share the arena before their first launch, so both take the forms of 1
        got = _greedy_pair(model, rows, steps, {"tile_force": force, "tile_pair": pair})
        for k in ("a", "b"):
            assert np.array_equal(ref[k], got[k]), f"context {k}: tile_pair={pair} changed {int((ref[k] != got[k]).sum())} tokens of {ref[k].size}"
        assert [f[0] for f in got["forms"]] == [1 if pair == -1 else pair] * 2, f"tile_pair={pair}: the loops ran under {got['forms']}"
        assert all(0 < f[1] <= 72 * KB for f in got["forms"]), f"tile_pair={pair}: a tiled launch asked for {got['forms']} bytes of LDS"
        if force == 5:
            assert [f[1] for f in got["forms"]] == [(72 if pair == 2 else 64) * KB] * 2


def test_a_context_alone_keeps_the_current_forms_in_its_loop(model):
    """the generation loop of one context on its own arena, default keys but the tile shape: 128 x 128 tiles at 128 KB, as before the key existed"""
    cfg, rows, steps = model.cfg, 130, 4
    e = hip.HipEngine(cfg, max_seqs=rows, kv_positions=8 + steps, tune={"tile_force": 5})
    try:
        e.load(model)
        rng = np.random.default_rng(11)
        e.prefill_batch([rng.integers(3, cfg.prompt_vocab, 4).astype(np.uint32) for _ in range(rows)])
        e.generate_greedy([4] * rows, steps)
        assert _forms(e) == (0, 128 * KB)
    finally:
        e.close()
