"""GPU: attn_rows_f8_kernel (csrc/parler_kernels.h), the row-major self-attention reader over Parler's e4m3 K/V cache (tune "kv_f8"; run_attn takes it from
max(attn_rows_min, attn_rows_f8_min) = 256 rows).  A lane owns 16 channels, H / 16 lanes a key row, NKL = 4096 / H key lanes a workgroup; key lane kl reads keys
kl, kl + NKL, ... of its slice, U = 2 in flight: passes of P = NKL U keys, merged through LDS.  The attention rows against the float64 softmax . V of what the
launch read back, through the checker of tests/test_gpu_parler_attention.py (its bars: 7.16e-6 of max|ref| on `att`, the fp16 rounding of that on `att16`, a
dropped boundary key moves the reference by ten times the bar, `part:4` holds -inf exactly on the empty slices) with this kernel's edges."""
import numpy as np
import pytest

import test_gpu_parler_attention as pa
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

U = 2
F8 = {"kv_f8": 1}


def _ragged(eng, monkeypatch, Ts, H, NH, f16w, tag):
    """pa._rows_case with this kernel's geometry: slot r behind a prompt of Ts[r] - 1 ids (one batched prefill), then one step of every slot: row r reads Ts[r] keys"""
    n, nkl = len(Ts), 4096 // H
    monkeypatch.setattr(pa, "H", H)
    monkeypatch.setattr(pa, "NH", NH)
    monkeypatch.setattr(pa, "_edges", lambda kernel, nz, T: (nkl - 1, nkl, nkl * U - 1, nkl * U, -(-T // nz) - 1, -(-T // nz)))
    assert eng.debug_read("kv_elem", 1)[0] == 1
    ids, audio = pa._ids(n)
    eng.prefill_batch([ids[s, :T - 1] for s, T in enumerate(Ts)])
    lg = eng.step(audio[:n], [T - 1 for T in Ts], list(range(n)))
    assert np.isfinite(lg).all()
    log, failures = [], []
    pa._fetch_and_check(eng, tag, ("rows_f8", 1 if n >= 1024 else 4, "att16" if f16w else "att"), [T - 1 for T in Ts], list(range(n)), log, failures)
    assert not failures, "\n".join(failures)
    return log[0]


P = 16 * U                                                                            # the test model: 16 key lanes
T256 = (1, 2, 3, 4, 5, 4 * 16 - 1, 4 * 16, 4 * 16 + 1, 4 * P - 1, 4 * P, 4 * P + 1)   # empty slices, fewer keys than key lanes, a slice of one pass and a key
LONG256 = {5: 1040, 77: 1041, 200: 1040, 255: 1041}                                   # slices of 260 and of 261 / 260 keys
T1024 = (1, 15, 16, 17, P - 1, P, P + 1, 2 * P + 1, 129)


@pytest.mark.parametrize("n,wtype", [(256, gguf.F32), (256, gguf.F16), (1024, gguf.F16)], ids=["256rows-4slices-att", "256rows-4slices-att16", "1024rows-1slice-att16"])
def test_rows_f8_kernel_against_float64(n, wtype, monkeypatch):
    """256 rows: four slices + attn_combine_kernel (no partials exist there without the reader: attn_kernel runs unsplit); 1024 rows: one slice"""
    Ts = [LONG256.get(r, T256[r % len(T256)]) for r in range(256)] if n == 256 else [T1024[(r + r // len(T1024)) % len(T1024)] for r in range(1024)]
    eng = pa._engine(wtype, gguf.F32, n, kv_positions=pa.CTX if n == 256 else 136, monkeypatch=monkeypatch, tune=F8)
    worst = _ragged(eng, monkeypatch, Ts, 256, 4, wtype == gguf.F16, f"e4m3 rows{n}")
    assert worst["keys"] == (1, max(Ts))
    eng.tune("attn_rows_f8_min", 0)      # the key exists
    eng.close()


def test_rows_f8_kernel_one_wave_per_key_lane(monkeypatch):
    """hidden 1024, 16 heads: 64 lanes per key row, every wave one key lane, NKL = 4 (Parler-Mini's lane shape); 256 rows, `att`"""
    m = synth.build(synth.tiny(hidden=1024, heads=16, layers=1, ctx=136, prompt_vocab=pa.PV, weight_type=gguf.F32))
    t = m.by_name["decoder.embed_prompts"]      # pa._model's table, a hundred times as large
    t2 = gguf.Tensor.from_array(t.name, (t.to_f32().reshape(pa.PV, 1024) * np.float32(100.0)).astype(np.float32), t.type)
    m.tensors[[x.name for x in m.tensors].index(t.name)] = t2
    m.by_name[t.name] = t2
    monkeypatch.delenv("TTS_HIP_ATTN_ROWS", raising=False)
    monkeypatch.delenv("TTS_HIP_ATTN_NSPLIT", raising=False)
    eng = hip.HipEngine(m.cfg, max_seqs=256, use_cross_attn=False, kv_positions=136, tune=F8)
    eng.load(m)
    T = (1, 3, 4, 5, 4 * U - 1, 4 * U, 4 * U + 1, 130)
    worst = _ragged(eng, monkeypatch, [T[(r + r // len(T)) % len(T)] for r in range(256)], 1024, 16, False, "e4m3 hidden 1024 rows256")
    eng.close()
    assert worst["keys"] == (1, 130)


Q8_BAR = 4 * 8.03e-3      # 4 x the fp16-cache distance below


def test_quantised_out_projection_reads_the_readers_blocks(monkeypatch):
    """Q8_0 matrices, 256 rows: the combine behind the reader writes the out projection's Q8_0 blocks.  Logits of one step against the same engine under
    attn_rows_f8_min = 0 (attn_kernel): the two differ by summation order in front of a Q8_0 rounding, so the bar is measured, not derived: 4 x the same
    distance between TTS_HIP_ATTN_ROWS=0 and the default over the fp16 cache on the parent commit, max|a - b| / max|b| on MI355X:
      fp16 cache, attn_kernel against attn_rows_kernel + combine (parent)   8.03e-3   -> bar 3.21e-2
      e4m3 cache, attn_kernel against attn_rows_f8_kernel + combine         8.72e-3"""
    Ts = [T256[r % len(T256)] + 1 for r in range(256)]
    ids, audio = pa._ids(256)
    model = synth.build(synth.tiny(ctx=264, prompt_vocab=pa.PV, weight_type=gguf.Q8_0))
    monkeypatch.delenv("TTS_HIP_ATTN_ROWS", raising=False)
    monkeypatch.delenv("TTS_HIP_ATTN_NSPLIT", raising=False)
    lg = []
    for f8_min in (256, 0):
        eng = hip.HipEngine(model.cfg, max_seqs=256, use_cross_attn=False, kv_positions=264, tune=dict(F8, attn_rows_f8_min=f8_min))
        eng.load(model)
        eng.prefill_batch([ids[s, :T - 1] for s, T in enumerate(Ts)])
        lg.append(eng.step(audio[:256], [T - 1 for T in Ts], list(range(256))))
        eng.close()
    d = float(np.abs(lg[0] - lg[1]).max() / np.abs(lg[1]).max())
    print(f"[kv_f8 rows] Q8_0 logits, reader against attn_kernel: {d:.3e}")
    assert np.isfinite(lg[0]).all() and 0.0 < d < Q8_BAR, d


def test_session_of_256_slots_equals_the_eager_step_loop(monkeypatch):
    """stream_begin / stream_admit / stream_run: the launch captured once and replayed while the histories grow, against FLAG_NO_GRAPH steps"""
    n, n_steps = 256, 6
    ids, _ = pa._ids(n)
    prompts = [ids[s, :1 + s % 7] for s in range(n)]
    cfg = pa._model(gguf.F16).cfg
    monkeypatch.delenv("TTS_HIP_ATTN_ROWS", raising=False)
    monkeypatch.delenv("TTS_HIP_ATTN_NSPLIT", raising=False)
    eager = hip.HipEngine(cfg, max_seqs=n, use_cross_attn=False, kv_positions=24, tune=F8, flags=hip.FLAG_NO_GRAPH)
    eager.load(pa._model(gguf.F16))
    eager.prefill_batch(prompts)
    cur, want = np.full((n, cfg.n_out), cfg.bos, dtype=np.uint32), []
    for st in range(n_steps):
        tok = eager.step(cur, [len(p) + st for p in prompts], list(range(n))).argmax(-1).astype(np.uint32)
        want.append(tok)
        cur = np.where(np.arange(cfg.n_out)[None, :] <= st, tok, cfg.bos).astype(np.uint32)
    eager.close()
    want = np.stack(want)
    eng = pa._engine(gguf.F16, gguf.F32, n + 1, kv_positions=24, monkeypatch=monkeypatch, tune=F8)      # (a session wants a spare cache slot)
    eng.stream_begin(n, n_steps)
    eng.stream_admit(list(range(n)), prompts)
    done = dict(eng.stream_run(n_steps))
    for s in range(n):
        steps = done.get(s, n_steps)
        assert np.array_equal(eng.stream_collect(s, steps), want[:steps, s]), s
    eng.stream_end()
    eng.close()
