"""GPU: attn_rows_kernel<U> at U = 2, 4 and 8 keys in flight per lane (tune("attn_rows_u"), csrc/parler_kernels.h).  U changes how many K / V rows a lane
has requested before it folds the first of them, never the arithmetic or the key order: the attention rows, the logits and with them the greedy tokens
must be the SAME BITS under the three values, and U = 8 (the only instantiation until the key existed) must stay inside the float64 bar of
tests/test_gpu_parler_attention.py, whose model, ids, engine set-up and checker are used here unchanged.

One context per U runs the same batched prefill and three steps, every row on its own cache slot with its own history (a ragged forward):
  256 rows  (fp32 matrices, `att`):   four key slices per row + attn_combine_kernel
  1024 rows (fp16 matrices, `att16`): one slice per row
Histories of the first step T = 1, 2, 3, 4, 5, 7, 8, 9, 17 (below U, at U and one past a multiple of every U; at 256 rows also slices with no key at
all), then T + 1 and T + 2; fp32 and fp16 cache."""
import numpy as np
import pytest

import test_gpu_parler_attention as pa
from tts_cpp_amd import gguf, hip

pytestmark = pytest.mark.gpu

T_FIRST = (1, 2, 3, 4, 5, 7, 8, 9, 17)
STEPS = 3
US = (8, 4, 2)


def _run(U, n, wtype, kv, Ts, monkeypatch, tag):
    """-> per step (attention rows of the last layer, logits); U = 8: every step's launch through the float64 checker as well"""
    f16w = wtype == gguf.F16
    eng = pa._engine(wtype, kv, n, kv_positions=136, monkeypatch=monkeypatch, tune={"attn_rows_u": U})
    ids, audio = pa._ids(n)
    eng.prefill_batch([ids[s, :T - 1] for s, T in enumerate(Ts)])
    plan = pa._plan(n, f16w)
    assert plan == ("rows", 1 if n >= 1024 else 4, "att16" if f16w else "att")
    seqs, cur, out, log, failures = list(range(n)), audio[:n], [], [], []
    for k in range(STEPS):
        pos = [T - 1 + k for T in Ts]
        lg = eng.step(cur, pos, seqs)
        att = eng.debug_read(plan[2], n * pa.H).copy()
        if U == 8:
            pa._fetch_and_check(eng, f"{tag} U=8 step {k}", plan, pos, seqs, log, failures)
        out.append((att, lg))
        cur = lg.argmax(-1).astype(np.uint32)
    eng.close()
    assert not failures, "\n".join(failures)
    if U == 8:
        assert len(log) == STEPS and log[0]["keys"] == (1, 17) and log[-1]["keys"] == (STEPS, 16 + STEPS)
    return out


@pytest.mark.parametrize("kv", [gguf.F32, gguf.F16], ids=pa.KV_IDS.get)
@pytest.mark.parametrize("n,wtype", [(256, gguf.F32), (1024, gguf.F16)], ids=["256rows-4slices", "1024rows-1slice"])
def test_keys_in_flight_do_not_change_a_bit(n, wtype, kv, monkeypatch):
    Ts = [T_FIRST[(r + r // len(T_FIRST)) % len(T_FIRST)] for r in range(n)]   # neighbouring rows differ; every T next to every other
    assert set(Ts) == set(T_FIRST)
    tag = f"{'f16' if wtype == gguf.F16 else 'f32'} {pa.KV_IDS[kv]} rows{n}"
    ref = _run(8, n, wtype, kv, Ts, monkeypatch, tag)
    for U in US[1:]:
        got = _run(U, n, wtype, kv, Ts, monkeypatch, tag)
        for k, ((att0, lg0), (att1, lg1)) in enumerate(zip(ref, got)):
            assert np.isfinite(att1).all() and np.isfinite(lg1).all()
            diff = np.flatnonzero(att0.view(np.uint32) != att1.view(np.uint32))
            assert diff.size == 0, f"{tag} step {k}: U={U} differs from U=8 in {diff.size} attention values, first at row {diff[0] // pa.H} (T={Ts[diff[0] // pa.H] + k})"
            assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32)), f"{tag} step {k}: logits of U={U} differ from U=8"
            assert np.array_equal(lg0.argmax(-1), lg1.argmax(-1))


def test_only_the_built_instantiations_are_accepted(monkeypatch):
    eng = pa._engine(gguf.F32, gguf.F32, 1, kv_positions=136, monkeypatch=monkeypatch)
    for v in (0, 1, 3, 6, 16):
        with pytest.raises(hip.HipError):
            eng.tune("attn_rows_u", v)
    for v in US:
        eng.tune("attn_rows_u", v)
    eng.close()
