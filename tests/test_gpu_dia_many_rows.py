"""GPU: Dia decoder steps of more than 16 rows on the tiled MFMA GEMM (dia_forward_tiled, csrc/shim_llama.hip), and contexts of up to 128 utterance slots.

A step takes the tiled route when it has more than 16 rows, every decoder matrix and the heads are F16 with K % 128 == 0 and N % 16 == 0, the context does
not carry TTS_HIP_FLAG_VALU_GEMM, and tune("dia_tile_min_rows") is non-zero and at most the row count: 0 by default on contexts of at most 64 slots (they
launch what they always launched), 17 on larger ones.  debug_read("di_tiled") counts the gemm_tile_kernel launches of the last forward, "di_pending_max" the
most K-slice slabs a GEMM left for the next rms norm.

Bars: the project's own for fp16 matrices (tests/test_gpu_dia.py): 2e-3 of max|oracle| on the raw logits, 8e-3 on the guided ones; F32 2e-4 / 8e-4, Q8_0
3e-2 / 12e-2.  The oracle is DiaOracle(act_mode=1): activations rounded to fp16 in front of an F16 matrix, what the producers of the route store."""
import functools

import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

RAW, GUIDED = 2e-3, 8e-3
STEPS = 3
LATE = 2                      # this utterance of a step's order joins at the second step, one position behind the others
SAMPLING = dict(top_k=8, repetition_penalty=1.3)
SAMPLING_B = dict(top_k=20, top_p=0.9, temperature=0.8, repetition_penalty=1.1)


def relerr(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _args(cfg):
    return dict(delay_pattern=[0, 8, 9, 10, 11, 12, 13, 14, 15], bos=cfg.bos, eos=cfg.eos, pad=cfg.pad, max_delay=cfg.max_delay)


@functools.lru_cache(maxsize=None)
def _model(wtype=gguf.F16, dec_ffn=512, max_gen=48, enc_hidden=128, suppress=False):
    return synth.build_dia(synth.dia_tiny(weight_type=wtype, dec_ffn=dec_ffn, max_gen=max_gen, enc_hidden=enc_hidden), suppress_special=suppress)


def _text(u):
    return "[S%d] utt %d %s." % (u % 2 + 1, u, "abcdefgh"[: u % 7])       # at most 24 bytes once the tag is one byte: the tiny text context


def _engine(model, n, tune=None, **kw):
    eng = hip.DiaEngine(model.cfg, max_utterances=n, **kw)
    for k, v in (tune or {}).items():
        eng.tune(k, v)
    eng.load(model)
    return eng


def _checked(n):
    """six utterances of a step of n: the first, the last, those whose rows sit on either side of rows 63 | 64 and 127 | 128 (utterances 31 | 32, 63 | 64),
    where the step has them; filled up from the front otherwise; and the late one"""
    want = [u for u in (0, n - 1, 31, 32, 63, 64) if 0 <= u < n]
    for u in range(n):
        if len(set(want)) >= 6:
            break
        want.append(u)
    return sorted(set(want) | {LATE})


def _plan(n, seed=5):
    """slots in a shuffled order, ids of every utterance and step"""
    rng = np.random.default_rng(seed + n)
    return rng.permutation(n), rng.integers(0, 64, (STEPS, n, 9)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle_rows(n, dec_ffn=512, wtype=gguf.F16, enc_hidden=128):
    """per checked utterance u: the raw and the guided logits of its steps, from an oracle of its own -> {u: [(step, raw, guided)]}"""
    model = _model(wtype, dec_ffn, enc_hidden=enc_hidden)
    cfg = model.cfg
    _, ids = _plan(n)
    out = {}
    for u in _checked(n):
        o = orc.DiaOracle(model, act_mode=1)
        o.encode(*orc.dia_tokenize(_text(u), cfg.max_ctx))
        rows, pos = [], 0
        for s in range(STEPS):
            if u == LATE and s == 0:
                continue
            ref, ref_raw = o.step(ids[s, u], pos, want_raw=True)
            rows.append((s, np.array(ref_raw, copy=True), np.array(ref, copy=True)))
            pos += 1
        out[u] = rows
    return out


def _encode_all(eng, n, slots):
    for u in range(n):
        eng.encode_slot(int(slots[u]), *orc.dia_tokenize(_text(u), eng.cfg.max_ctx))


def _run_steps(eng, n):
    """the three steps of the plan on an engine whose slots are encoded -> per step (order, raw, guided, di_tiled, di_pending_max)"""
    slots, ids = _plan(n)
    res = []
    for s in range(STEPS):
        order = [u for u in range(n) if not (u == LATE and s == 0)]
        pos = [s - 1 if u == LATE else s for u in order]
        lg, raw = eng.step_batch(ids[s, order], pos, slots=[int(slots[u]) for u in order], want_raw=True)
        res.append((order, raw.copy(), lg.copy(), int(eng.debug_read("di_tiled", 1)[0]), int(eng.debug_read("di_pending_max", 1)[0])))
    return res


def _against_oracle(res, refs, raw_bar, guided_bar, tag):
    worst_raw = worst_guided = 0.0
    for u, rows in refs.items():
        for s, ref_raw, ref in rows:
            order, raw, lg = res[s][:3]
            k = order.index(u)
            worst_raw, worst_guided = max(worst_raw, relerr(raw[k], ref_raw)), max(worst_guided, relerr(lg[k], ref))
    print(f"[dia many rows] {tag}: raw {worst_raw:.2e} (bar {raw_bar:.0e}), guided {worst_guided:.2e} (bar {guided_bar:.0e})")
    assert worst_raw < raw_bar, tag
    assert worst_guided < guided_bar, tag


@functools.lru_cache(maxsize=None)
def _steps_of(n, kv=gguf.F32, key=None, slots_ctx=None):
    """the plan's three steps on a context of slots_ctx (default n) slots; key: tune("dia_tile_min_rows"), None = the context's default"""
    model = _model()
    eng = _engine(model, slots_ctx or n, tune=None if key is None else {"dia_tile_min_rows": key}, kv_type=kv)
    _encode_all(eng, n, _plan(n)[0])
    res = _run_steps(eng, n)
    eng.close()
    return res


# ---- 1. the cap ---------------------------------------------------------------------------------------------------------------------------
def test_128_slots_are_created_and_129_refused():
    cfg = _model().cfg
    eng = hip.DiaEngine(cfg, max_utterances=128)
    eng.close()
    with pytest.raises(hip.HipError, match=r"tts_hip_dia_create.*max_utterances"):
        hip.DiaEngine(cfg, max_utterances=129)


def test_a_65_slot_context_encodes_slot_64_and_steps_65_utterances():
    model = _model()
    cfg = model.cfg
    eng = _engine(model, 65)
    for u in range(65):
        eng.encode_slot(u, *orc.dia_tokenize(_text(u), cfg.max_ctx))
    lg = eng.step_batch(np.full((65, cfg.n_out), cfg.bos, dtype=np.uint32), np.zeros(65, dtype=np.uint32))
    assert lg.shape == (65, cfg.n_out, cfg.out_vocab) and np.isfinite(lg).all()
    assert int(eng.debug_read("di_tiled", 1)[0]) > 0
    with pytest.raises(hip.HipError):
        eng.encode_slot(65, *orc.dia_tokenize(_text(0), cfg.max_ctx))
    eng.close()


# ---- 2. steps against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kv", [(9, gguf.F32), (32, gguf.F32), (33, gguf.F32), (33, gguf.F16), (65, gguf.F32), (128, gguf.F32)],
                         ids=["9", "32", "33", "33-kvf16", "65", "128"])
def test_tiled_steps_against_the_oracle(n, kv):
    """18 rows (the smallest tiled step), 64 and 66 rows (the 64-row tile edge), 130 and 256 rows (the cap); contexts of at most 64 slots opt in"""
    res = _steps_of(n, kv, 17 if n <= 64 else None)
    assert all((r[3] > 0) == (2 * len(r[0]) > 16) for r in res), [(len(r[0]), r[3]) for r in res]      # 9 utterances: 16 rows before the late one joins
    _against_oracle(res, _oracle_rows(n), RAW, GUIDED, f"{n} utterances, {'fp16' if kv == gguf.F16 else 'fp32'} cache")


# ---- 3. tiled against untiled ---------------------------------------------------------------------------------------------------------------
def test_tiled_against_untiled_at_33_utterances():
    tiled, plain = _steps_of(33, gguf.F32, 17), _steps_of(33, gguf.F32, 0)
    assert all(r[3] > 0 for r in tiled) and all(r[3] == 0 for r in plain)
    worst_raw = worst_guided = 0.0
    for (order, raw_t, lg_t, _, _), (_, raw_p, lg_p, _, _) in zip(tiled, plain):
        for k in range(len(order)):
            worst_raw = max(worst_raw, relerr(raw_t[k], raw_p[k]), relerr(raw_p[k], raw_t[k]))
            worst_guided = max(worst_guided, relerr(lg_t[k], lg_p[k]), relerr(lg_p[k], lg_t[k]))
    print(f"[dia many rows] tiled against untiled, 33 utterances: raw {worst_raw:.2e} (bar {2 * RAW:.0e}), guided {worst_guided:.2e} (bar {2 * GUIDED:.0e})")
    assert worst_raw < 2 * RAW and worst_guided < 2 * GUIDED
    _against_oracle(plain, _oracle_rows(33), RAW, GUIDED, "33 utterances, 16-feature kernel")


# ---- 4. slabs and shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [1, 2, 4, 8])
def test_every_tile_shape_and_k_slice_count_at_66_rows(ks):
    """dec_ffn 2048: `out` (K = 2048) takes 1, 2, 4, 8 K slices, so / co (K = 256) at most 2; the slabs are folded by the next rms_fold_rows_f16_kernel"""
    n = 33
    model = _model(dec_ffn=2048)
    eng = _engine(model, n, tune={"dia_tile_min_rows": 17, "tile_ks": ks})
    _encode_all(eng, n, _plan(n)[0])
    refs = _oracle_rows(n, 2048)
    for shape in range(6):
        eng.tune("tile_force", shape)
        res = _run_steps(eng, n)
        assert all(r[3] > 0 for r in res)
        assert all(r[4] == (ks if ks > 1 else 0) for r in res), (shape, [r[4] for r in res])
        _against_oracle(res, refs, RAW, GUIDED, f"66 rows, tile shape {shape}, {ks} K slices")
    eng.close()


# ---- 5. unchanged contexts ------------------------------------------------------------------------------------------------------------------
def test_a_9_slot_context_stays_untiled_by_default():
    a, b = _steps_of(9, gguf.F32, None), _steps_of(9, gguf.F32, 0)
    assert all(r[3] == 0 for r in a) and all(r[3] == 0 for r in b)
    for ra, rb in zip(a, b):
        assert np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    assert not np.array_equal(a[2][1], _steps_of(9, gguf.F32, 17)[2][1])          # the key reaches the route


def test_the_key_turned_on_after_load_reaches_the_route():
    """a small context allocates the route's fp16 rows only once the key is above 0: tune after load allocates them then, and the steps equal those of a
    context that had the key before load"""
    n = 9
    eng = _engine(_model(), n)
    _encode_all(eng, n, _plan(n)[0])
    plain = _run_steps(eng, n)
    assert all(r[3] == 0 for r in plain)
    eng.tune("dia_tile_min_rows", 17)
    late = _run_steps(eng, n)
    eng.close()
    early = _steps_of(n, gguf.F32, 17)
    for a, b in zip(late, early):
        assert a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert late[2][3] > 0


def test_7_utterances_on_a_128_slot_context_equal_a_7_slot_context():
    a, b = _steps_of(7, gguf.F32, None, 128), _steps_of(7, gguf.F32, None, 7)
    assert all(r[3] == 0 for r in a) and all(r[3] == 0 for r in b)                # 14 rows: the streaming route on every context
    for ra, rb in zip(a, b):
        assert np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])


@pytest.mark.parametrize("wtype,tol", [(gguf.F32, 2e-4), (gguf.Q8_0, 3e-2)], ids=["f32", "q8_0"])
def test_f32_and_q8_0_matrices_stay_on_their_kernels_at_18_rows(wtype, tol):
    eh = 256 if wtype == gguf.Q8_0 else 128          # as tests/test_gpu_dia.py: the integer path wants rows of multiples of 256
    model = _model(wtype, enc_hidden=eh)
    eng = _engine(model, 9, tune={"dia_tile_min_rows": 17})
    _encode_all(eng, 9, _plan(9)[0])
    res = _run_steps(eng, 9)
    eng.close()
    assert all(r[3] == 0 for r in res)
    _against_oracle(res, _oracle_rows(9, 512, wtype, eh), tol, 4 * tol, f"18 rows, matrix type {wtype}")


# ---- 6. loops -------------------------------------------------------------------------------------------------------------------------------
LOOP_N = 20
EXTRA = tuple(2 + (7 * i) % 17 for i in range(30))          # budgets max_delay + 2 .. 18


def _loop_model():
    # max_gen 1024: the eager step's key-split count (max_gen / 128) is the captured step's fixed one, so both run the same launches
    return _model(max_gen=1024, suppress=True)


def _loop_engine(n_ctx=65, flags=0, n_enc=LOOP_N):
    model = _loop_model()
    eng = _engine(model, n_ctx, flags=flags)
    for u in range(n_enc):
        eng.encode_slot(u, *orc.dia_tokenize(_text(u), model.cfg.max_ctx))
    return eng


def test_captured_loop_equals_the_eager_loop_on_the_tiled_route():
    cfg = _loop_model().cfg
    budget = cfg.max_delay + 18
    uni = np.random.default_rng(3).random((budget, LOOP_N, cfg.n_out), dtype=np.float32)
    got = []
    for flags in (0, hip.FLAG_NO_GRAPH):
        eng = _loop_engine(flags=flags)
        got.append(eng.generate(LOOP_N, budget, **_args(cfg)) + eng.generate(LOOP_N, budget, uniforms=uni, **SAMPLING, **_args(cfg)))
        assert int(eng.debug_read("di_tiled", 1)[0]) > 0
        eng.close()
    assert len(got[0]) == 2 * LOOP_N and all(len(a) == budget - 1 for a in got[0])
    assert all(np.array_equal(a, b) for a, b in zip(*got))
    assert not np.array_equal(got[0][0], got[0][LOOP_N])


def test_generate_equals_the_gen_pieces_on_the_tiled_route():
    cfg = _loop_model().cfg
    eng = _loop_engine()
    budget = cfg.max_delay + 9
    want = eng.generate(LOOP_N, budget, **_args(cfg))
    for piece in (1, 5, 64):
        eng.gen_begin(LOOP_N, budget, **_args(cfg))
        for _ in range(budget + 2):
            eng.gen_launch(piece)
            out, steps, done, _ = eng.gen_wait()
            if done.all():
                break
        assert done.all() and steps.tolist() == [len(w) for w in want]
        for u in range(LOOP_N):
            assert np.array_equal(out[u, :steps[u]], want[u]), (piece, u)
    assert int(eng.debug_read("di_tiled", 1)[0]) > 0
    eng.close()


def _session(eng, n_slots, utts, budgets, uniforms=None, settings=None, run=4, **sampling):
    """utts through one session: the first n_slots at once, the rest as slots free up (tests/test_gpu_dia_kv_f16.py); settings: a mixed session
    -> (ids per utterance, slot per utterance, admissions beside live slots, look-ins that found a parked slot beside a live one)"""
    cfg = eng.cfg
    if settings is not None:
        eng.stream_begin_mixed(n_slots, cfg.max_gen, **_args(cfg))
    else:
        eng.stream_begin(n_slots, cfg.max_gen, sampled=uniforms is not None, **sampling, **_args(cfg))
    out, slot_of, in_slot = [None] * len(utts), [None] * len(utts), {}
    free, nxt, refills, parked_beside_live = list(range(n_slots)), 0, 0, 0

    def admit():
        nonlocal nxt
        take = []
        while free and nxt < len(utts):
            take.append((free.pop(0), nxt))
            nxt += 1
        if take:
            sl, tk, ln, bd = [s for s, _ in take], [utts[u][0] for _, u in take], [utts[u][1] for _, u in take], [budgets[u] for _, u in take]
            un = None if uniforms is None else np.stack([uniforms[u] for _, u in take])
            if settings is not None:
                eng.stream_admit_mixed(sl, tk, ln, [settings[u] for _, u in take], budgets=bd, uniforms=un)
            else:
                eng.stream_admit(sl, tk, ln, budgets=bd, uniforms=un)
            for s, u in take:
                in_slot[s], slot_of[u] = u, s
        return len(take)

    admit()
    for _ in range(400):
        if not in_slot:
            break
        for s, steps in eng.stream_run(run):
            out[in_slot.pop(s)] = eng.stream_collect(s, steps)
            free.append(s)
        free.sort()
        live = len(in_slot)
        if admit() and live:
            refills += 1
        if free and in_slot:
            parked_beside_live += 1
    assert not in_slot and nxt == len(utts)
    eng.stream_end()
    return out, slot_of, refills, parked_beside_live


def _reference(eng, n_slots, slot, utt, budget, uniforms=None, **sampling):
    """tts_hip_dia_generate over n_slots slots of the same context: the utterance in `slot`, whatever sentence the others hold"""
    cfg = eng.cfg
    eng.encode_slot(slot, *utt)
    if uniforms is None:
        return eng.generate(n_slots, budget, **_args(cfg))[slot]
    u = np.random.default_rng(99).random((budget, n_slots, cfg.n_out), dtype=np.float32)
    u[:, slot, :] = uniforms[:budget]
    return eng.generate(n_slots, budget, uniforms=u, **sampling, **_args(cfg))[slot]


def test_sessions_of_20_slots_over_30_utterances_equal_generate():
    """refills, a parked slot beside live ones; uniform greedy, uniform sampled, and mixed with two samplers and greedy utterances"""
    cfg = _loop_model().cfg
    utts = [orc.dia_tokenize(_text(100 + u), cfg.max_ctx) for u in range(30)]
    budgets = [cfg.max_delay + e for e in EXTRA]
    uni = np.random.default_rng(5).random((30, cfg.max_gen, cfg.n_out), dtype=np.float32)
    settings = [(SAMPLING, SAMPLING_B, None)[u % 3] for u in range(30)]
    eng = _loop_engine()
    greedy, slots, refills, parked = _session(eng, LOOP_N, utts, budgets)
    assert int(eng.debug_read("di_tiled", 1)[0]) > 0
    assert refills >= 1 and parked >= 1
    sampled, slots_s, _, _ = _session(eng, LOOP_N, utts, budgets, uniforms=uni, **SAMPLING)
    mixed, slots_m, _, _ = _session(eng, LOOP_N, utts, budgets, uniforms=uni, settings=settings)
    assert slots_s == slots and slots_m == slots
    for u in range(30):
        ref_g = _reference(eng, LOOP_N, slots[u], utts[u], budgets[u])
        ref_s = _reference(eng, LOOP_N, slots[u], utts[u], budgets[u], uniforms=uni[u], **SAMPLING)
        assert greedy[u].shape == ref_g.shape and np.array_equal(greedy[u], ref_g), (u, slots[u])
        assert sampled[u].shape == ref_s.shape and np.array_equal(sampled[u], ref_s), (u, slots[u])
        ref_m = ref_g if settings[u] is None else ref_s if settings[u] is SAMPLING else _reference(eng, LOOP_N, slots[u], utts[u], budgets[u], uniforms=uni[u], **SAMPLING_B)
        assert mixed[u].shape == ref_m.shape and np.array_equal(mixed[u], ref_m), (u, slots[u])
    assert not np.array_equal(sampled[0], greedy[0])
    eng.close()


def test_a_session_of_66_slots_with_70_short_utterances():
    """both workgroups of the loop's pre- and post-step (64 slots each) hold live and finishing slots; a dropped slot beside them"""
    cfg = _loop_model().cfg
    n = 66
    utts = [orc.dia_tokenize(_text(200 + u), cfg.max_ctx) for u in range(70)]
    budgets = [cfg.max_delay + 2 + (5 * u) % 6 for u in range(70)]
    eng = _loop_engine(n_ctx=n, n_enc=0)          # no slot encoded: begin clears position 0 of all 66, the slots beyond the clear kernel's 64-bit mask in a launch of their own
    got, slots, refills, _ = _session(eng, n, utts, budgets, run=3)
    assert refills >= 1 and max(slots) == 65 and int(eng.debug_read("di_tiled", 1)[0]) > 0
    for u in (0, 1, 31, 32, 63, 64, 65, 66, 67, 68, 69):
        ref = _reference(eng, n, slots[u], utts[u], budgets[u])
        assert got[u].shape == ref.shape == (budgets[u] - 1, cfg.n_out) and np.array_equal(got[u], ref), (u, slots[u])
    # launch / wait and drop with slots of both workgroups live
    eng.stream_begin(n, cfg.max_gen, **_args(cfg))
    eng.stream_admit(list(range(n)), [utts[u][0] for u in range(n)], [utts[u][1] for u in range(n)], budgets=[cfg.max_delay + 6] * n)
    eng.stream_launch(3)
    _, steps, done, fin = eng.stream_wait()
    assert steps.tolist() == [3] * n and not done.any() and not fin
    eng.stream_drop([1, 65])
    fin = []
    for _ in range(40):
        fin += eng.stream_run(4)
        if len(fin) == n - 2:
            break
    assert sorted(s for s, _ in fin) == [s for s in range(n) if s not in (1, 65)] and all(st == cfg.max_delay + 5 for _, st in fin)
    eng.stream_end()
    eng.close()


# ---- 7. the runner --------------------------------------------------------------------------------------------------------------------------
def test_runner_with_20_slots_and_the_clamp_at_128(tmp_path, capfd):
    """F32 matrices, as in the runner equalities of tests/test_gpu_dia.py and test_gpu_dia_kv_f16.py: a 20-slot runner is a context of at most 64 slots, so
    generate() (2 rows, the streaming kernels) and generate_batch (40 rows, the 16-feature GEMM) run the kernels they ran before this route existed, and
    only fp32 matrices give both the same rows.  With fp16 matrices the two kernels sum in different orders: measured on MI355X, 19 of the 20 greedy
    id streams were equal and utterance 7's was not."""
    from tts_cpp_amd import runner
    model = synth.build_dia(synth.dia_tiny(max_gen=64), suppress_special=True)
    path = model.write_gguf(str(tmp_path / "dia.gguf"))
    texts = [_text(u) for u in range(20)]
    kw = dict(sample=0, max_tokens=30)
    r = runner.Runner(path, sample=0, max_seqs=20)
    assert r.stream_capacity() == 20
    singles, ids = [], []
    for t in texts:
        singles.append(r.generate(t, **kw))
        ids.append(r.last_tokens(1).copy())
    batch = r.generate_batch(texts, **kw)
    for i in range(20):
        assert ids[i].size > 0 and np.array_equal(r.last_tokens(16 + i), ids[i]), i
        assert batch[i].shape == singles[i].shape and np.abs(batch[i] - singles[i]).max() < 1e-5, i
    stream = r.generate_stream(texts, **kw)
    assert len(stream) == 20
    for i in range(20):
        assert np.array_equal(r.last_tokens(16 + i), ids[i]), i
        assert stream[i].shape == singles[i].shape and np.abs(stream[i] - singles[i]).max() < 1e-5, i
    r.close()
    capfd.readouterr()
    big = runner.Runner(path, sample=0, max_seqs=200)
    err = capfd.readouterr().err
    assert big.stream_capacity() == 128
    lines = [ln for ln in err.splitlines() if "max_seqs" in ln]
    assert len(lines) == 1 and "200" in lines[0] and "128" in lines[0], err
    big.close()


def test_runner_with_65_slots_runs_the_tiled_route_on_fp16_matrices(tmp_path):
    """a runner of more than 64 slots on the issue's fp16 model: generate_batch (the fixed batch of 65, 130 rows) and generate_stream (the session of 65 slots)
    both step on the tiled route, at the same slot count, so an utterance's rows see the same launches: ids equal, audio within 1e-5"""
    from tts_cpp_amd import runner
    model = synth.build_dia(synth.dia_tiny(weight_type=gguf.F16, max_gen=64), suppress_special=True)
    path = model.write_gguf(str(tmp_path / "dia.gguf"))
    texts = [_text(u) for u in range(65)]
    kw = dict(sample=0, max_tokens=26)
    r = runner.Runner(path, sample=0, max_seqs=65)
    assert r.stream_capacity() == 65
    batch = r.generate_batch(texts, **kw)
    ids = [r.last_tokens(16 + i).copy() for i in range(65)]
    stream = r.generate_stream(texts, **kw)
    assert len(batch) == len(stream) == 65
    for i in range(65):
        assert ids[i].size > 0 and np.array_equal(r.last_tokens(16 + i), ids[i]), i
        assert stream[i].shape == batch[i].shape and batch[i].size > 0 and np.abs(stream[i] - batch[i]).max() < 1e-5, i
    r.close()


# ---- 8. the profiler ------------------------------------------------------------------------------------------------------------------------
def test_profile_times_the_tiled_route_by_class():
    """tts_hip_profile on an eager tiled step: one launch per layer of every GEMM class, the heads once, both attentions, the row producers under 'ln';
    the logits are those of the unprofiled step"""
    n = 9
    model = _model()
    L = model.cfg.dec_layers
    eng = _engine(model, n, tune={"dia_tile_min_rows": 17})
    _encode_all(eng, n, np.arange(n))
    ids = _plan(n)[1][0]
    pos = np.zeros(n, dtype=np.uint32)
    want = eng.step_batch(ids, pos)
    hip.engine_profile(eng, 1)
    got = eng.step_batch(ids, pos)
    st = hip.engine_profile_get(eng)
    hip.engine_profile(eng, 0)
    assert int(eng.debug_read("di_tiled", 1)[0]) == 6 * L + 1
    assert np.array_equal(got, want)
    for k in ("gemm_qkv", "gemm_attn_out", "gemm_cross_q", "gemm_cross_out", "gemm_fc1", "gemm_fc2", "attn_self", "attn_cross"):
        assert st[k]["launches"] == L and st[k]["ms_total"] > 0, (k, st[k])
    assert st["gemm_heads"]["launches"] == 1 and st["gemm_other"]["launches"] == 0
    assert st["ln"]["launches"] == 7 * L + 1          # per layer: three norms, two rows -> fp16, rope, silu; the final norm
    eng.close()
