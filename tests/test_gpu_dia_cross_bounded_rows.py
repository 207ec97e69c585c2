"""GPU: the finished-row form of Dia's bounded cross-attention, attn_cross_bounded_rows_kernel<3, float> / <4, _Float16> (csrc/dia_cross_kernels.h), the launch of
tune("dia_cross_bounded") where launch_attn_gqa splits no keys: more than 256 (head, row) pairs, or tune("attn_split") 1.  Models, engines and bars are those of
tests/test_gpu_dia_cross_bounded.py and tests/test_gpu_dia_kv_f16.py; the reference is the float64 softmax . V over ALL max_ctx keys of the cache rows read back.
1. the reader at 4 rows, sentence lengths at the edges of the pass loop (a pass is 16 keys, a round U = 3 / 4 passes); 2. 66 rows by default dispatch on the
streaming and the tiled route, against float64 and against the key off; 3. captured = eager loop, and the parked rows, inside the mode.
Measured on MI355X (printed under -s): see DESIGN.md, "Dia cross-attention that reads only the sentence's keys"."""
import dataclasses

import numpy as np
import pytest

import attn_reference as ar
import test_gpu_dia_kv_f16 as kvf
from test_gpu_dia_cross_bounded import BAR, F32_WORST, ON, _bounded_f32
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

NH, HD, A = kvf.NH, kvf.HD, kvf.A
ROWS = {**ON, "attn_split": 1}          # no key split: a step of any row count takes launch_attn_gqa's many-rows branch
KVS = pytest.mark.parametrize("kv", [gguf.F32, gguf.F16], ids=["kv32", "kv16"])


def _encode(eng, S, lens):
    for u, n in enumerate(lens):
        toks = np.zeros(S, dtype=np.uint32)
        toks[:n] = np.random.default_rng(1000 + u).integers(97, 123, n)
        toks[0] = 1 + u % 2          # the speaker tag
        eng.encode_slot(u, toks, n)
    assert eng.debug_read("di_klive", 2 * len(lens)).tolist() == [n for n in lens for _ in range(2)]


def _step(eng, cfg, lens, ids, pos, layers, sharp=False):
    """one step -> (the layers' (cross rows, folded queries), worst kernel / float32 restatement distance from float64 of max|ref|, least shift without the pad term or
    key n - 1, the query's slab count)"""
    S, R, theta = cfg.max_ctx, 2 * len(lens), kvf._powf(10000.0, -2.0 / HD)
    eng.step_batch(ids, pos)
    outs, w = [], dict(kernel=0.0, f32=0.0, sharp=np.inf)
    for layer in layers:
        meta = eng.debug_read(f"di_attn:{layer}:cross:meta", 4 + 3 * R)
        n_parts, stride, ld = (int(v) for v in meta[:3])
        assert int(meta[3]) == R and meta[4 + R: 4 + 2 * R].tolist() == [S] * R
        qbuf = eng.debug_read(f"di_attn:{layer}:cross:q", (n_parts - 1) * stride + R * ld + 1)
        outs.append((eng.debug_read(f"di_attn:{layer}:cross:out", R * A).reshape(R, A), np.stack([ar.fold_slabs(qbuf, n_parts, stride, r, ld, A) for r in range(R)])))
        for r in range(R):
            n, (K, V) = lens[r // 2], kvf._cross(eng, layer, r, S)
            assert not K[n:].any() and V[n:].any(axis=1).all()
            q = ar.rope_neox(outs[-1][1][r], pos[r // 2], theta, NH)
            ref = ar.attention_rows(q[None], K, V, [S], 1.0, NH, NH)[0]
            scale = np.abs(ref).max()
            w["kernel"] = max(w["kernel"], float(np.abs(outs[-1][0][r] - ref).max() / scale))
            w["f32"] = max(w["f32"], float(np.abs(_bounded_f32(q.astype(np.float32), K, V, n) - ref).max() / scale))
            if sharp and r % 2 == 0:   # the conditional rows (the unconditional ones read V rows that are copies of one another)
                shifts = list(ar.drop_shifts(q[None], K, V, [S], 1.0, NH, NH, lambda i, T: [n - 1])[0].values())
                if n < S:
                    shifts.append(float(np.abs(ar.attention_rows(q[None], K, V, [n], 1.0, NH, NH)[0] - ref).max() / scale))
                w["sharp"] = min(w["sharp"], *shifts)
    return outs, w, n_parts


@pytest.mark.parametrize("wtype", [gguf.F16, gguf.F32], ids=["w16", "w32"])
@KVS
@pytest.mark.parametrize("S", [256, 1024])
def test_rows_reader_against_float64_over_all_keys(S, kv, wtype):
    base, U = kvf._model(wtype), 3 if kv == gguf.F32 else 4          # KVRow<KV>::EXT_SLOTS
    cfg = dataclasses.replace(base.cfg, max_ctx=S)
    eng = kvf._engine(base, cfg=cfg, kv=kv, tune=ROWS)
    eng.set_debug(True)
    ids = np.random.default_rng(0xB0D).integers(0, cfg.audio_vocab, (2, cfg.n_out)).astype(np.uint32)
    worst = dict(kernel=0.0, f32=0.0, sharp=np.inf)
    for pair in [(15, 16), (17, 16 * U - 1), (16 * U + 1, S - 1), (S, S // 5)]:
        _encode(eng, S, pair)
        for pos in ([0, 0], [37, 5]):
            _, w, n_parts = _step(eng, cfg, pair, ids, pos, range(cfg.dec_layers), sharp=True)
            assert int(eng.debug_read("di_cross_bounded", 1)[0]) == cfg.dec_layers and (n_parts > 1) == (wtype == gguf.F16)
            worst = dict(kernel=max(worst["kernel"], w["kernel"]), f32=max(worst["f32"], w["f32"]), sharp=min(worst["sharp"], w["sharp"]))
    eng.close()
    print(f"[dia cross bounded rows] ctx {S} kv {kv} w {wtype}: kernel {worst['kernel']:.2e}  float32 association {worst['f32']:.2e}  least shift {worst['sharp']:.2e}  bar {BAR:.2e}")
    assert worst["f32"] <= F32_WORST and worst["sharp"] >= 10 * BAR and worst["kernel"] < BAR


@pytest.mark.parametrize("tile_min", [0, 17])
@KVS
def test_66_rows_by_default_dispatch_on_both_routes(kv, tile_min):
    model = kvf._model(gguf.F16)
    cfg, n = model.cfg, 33          # 66 rows x 4 heads > 256: no key split
    lens = [[1, 15, 16, 17, 47, 49, 63, 65, 200, 255, 256][u % 11] for u in range(n)]
    eng = kvf._engine(model, kv=kv, n=n, tune={**ON, "dia_tile_min_rows": tile_min})
    eng.set_debug(True)
    _encode(eng, cfg.max_ctx, lens)
    ids = np.random.default_rng(0xB0E).integers(0, cfg.audio_vocab, (n, cfg.n_out)).astype(np.uint32)
    pos, layers = [(7 * u) % 41 for u in range(n)], (0, cfg.dec_layers - 1)
    on, w, _ = _step(eng, cfg, lens, ids, pos, layers)
    assert int(eng.debug_read("di_cross_bounded", 1)[0]) == cfg.dec_layers and (int(eng.debug_read("di_tiled", 1)[0]) > 0) == (tile_min > 0)
    eng.tune("dia_cross_bounded", 0)
    off, w_off, _ = _step(eng, cfg, lens, ids, pos, layers)
    assert int(eng.debug_read("di_cross_bounded", 1)[0]) == 0
    eng.close()
    # on against off, row by row, where both read the same query bits: every row of layer 0.  Behind layer 0 the rows pass through fp16 (the out projection's
    # input), a last-bit difference there flips a rounding here and there, and the last layer's queries differ by up to 1.9e-4 of max|q| in a few rows (measured;
    # those rows then differ by as much, 3.3e-5 .. 2.2e-4, under either kernel): such a row is held to float64 from its own query instead, on and off alike
    same = [np.array([kvf._same_bits(qa[r], qb[r]) for r in range(2 * n)]) for (_, qa), (_, qb) in zip(on, off)]
    dist = max(float(np.abs(a[r] - b[r]).max() / np.abs(b[r]).max()) for (a, _), (b, _), m in zip(on, off, same) for r in np.flatnonzero(m))
    print(f"[dia cross bounded rows] 66 rows kv {kv} tile_min {tile_min}: kernel {w['kernel']:.2e} (key off {w_off['kernel']:.2e})  float32 association {w['f32']:.2e}  "
          f"on against off {dist:.2e} over {[int(m.sum()) for m in same]} rows  bar {BAR:.2e}")
    assert w["f32"] <= F32_WORST and w["kernel"] < BAR and w_off["kernel"] < BAR
    assert same[0].all() and dist < BAR


@KVS
def test_captured_loop_equals_the_eager_loop_in_the_mode(kv):
    model = synth.build_dia(synth.dia_tiny(max_gen=1024, max_ctx=256, weight_type=gguf.F16), suppress_special=True)
    cfg, got = model.cfg, []
    uni = np.random.default_rng(3).random((40, 2, cfg.n_out), dtype=np.float32)
    for flags in (0, hip.FLAG_NO_GRAPH):
        eng = kvf._engine(model, kv=kv, tune=ROWS, flags=flags)
        for u in range(2):
            eng.encode_slot(u, *kvf.orc.dia_tokenize(kvf.TEXTS[u], cfg.max_ctx))
        got.append(eng.generate(2, 40, **kvf._args(cfg)) + eng.generate(2, 40, uniforms=uni, **kvf.SAMPLING, **kvf._args(cfg)))
        assert int(eng.debug_read("di_cross_bounded", 1)[0]) == cfg.dec_layers
        eng.close()
    assert all(len(a) > 1 and np.array_equal(a, b) for a, b in zip(*got)) and not np.array_equal(got[0][0], got[0][2])


@KVS
def test_parked_rows_leave_their_one_v_row(kv):
    """the first step of an eager session, slot 0 live, slot 1 encoded but parked, slot 2 never encoded (its one key cleared): kend = [S, S, 1, 1, 1, 1]"""
    model = synth.build_dia(synth.dia_tiny(max_ctx=256, weight_type=gguf.F16), suppress_special=True)
    cfg = model.cfg
    S, W = cfg.max_ctx, cfg.dec_heads * HD
    utt, other = (kvf.orc.dia_tokenize(t, S) for t in kvf.TEXTS[:2])
    eng = kvf._engine(model, kv=kv, n=3, tune=ROWS, flags=hip.FLAG_NO_GRAPH)
    eng.set_debug(True)
    eng.encode_slot(1, *other)
    outs = []
    for key in (1, 0):
        eng.tune("dia_cross_bounded", key)
        eng.stream_begin(3, cfg.max_gen, **kvf._args(cfg))
        eng.stream_admit([0], [utt[0]], [utt[1]])
        eng.stream_run(1)
        assert int(eng.debug_read("di_cross_bounded", 1)[0]) == key * cfg.dec_layers
        assert all(eng.debug_read(f"di_attn:{l}:cross:meta", 64)[10:16].tolist() == [S, S, 1, 1, 1, 1] for l in range(cfg.dec_layers))
        outs.append([eng.debug_read(f"di_attn:{l}:cross:out", 6 * W).reshape(6, W) for l in range(cfg.dec_layers)])
        eng.stream_end()
    v0 = [np.stack([eng.debug_read(f"di_cv:{l}:{r}", W) for r in range(2, 6)]) for l in range(cfg.dec_layers)]
    eng.close()
    for on, off, v in zip(*outs, v0):
        assert np.array_equal(on[2:], v) and np.array_equal(on[2:], off[2:]) and on[2:4].any(axis=1).all() and not on[4:].any()
        assert np.abs(on[:2] - off[:2]).max() < BAR * np.abs(off[:2]).max() and on[:2].any(axis=1).all()
