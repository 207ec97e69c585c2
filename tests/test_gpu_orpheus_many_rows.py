"""Orpheus contexts of 65 .. 256 cache slots: lock-step forwards of more than 64 rows on GGUF-quantised matrices run on the LDS-tiled integer GEMM
(qgemm_tile_kernel), their activations quantised with transposed block scales by rms_fold_rows_q8t_kernel, silu_mul_q8t_kernel and
quant_rows_q8t_kernel; the o / down projections leave split-K slabs that the next rms norm folds; the LM head (5001 -> 5008 features) is the first
matrix on that kernel whose width is no multiple of the tile.  Logits against the oracle with the activation-flip bound of tests/test_gpu_orpheus.py
(3e-2 of max|ref|), the tiled path against the 16-feature kernel, every tile shape and slab count, the generation loop and the continuous session
above 64 rows, and contexts of at most 64 slots, which are unchanged."""
import functools

import numpy as np
import pytest

import oracle as orc
from tts_cpp_amd import gguf, hip, synth

pytestmark = pytest.mark.gpu

TOL_Q = 3e-2          # quantised matrices: one flipped Q8_0 activation code (tests/test_gpu_orpheus.py)
VOCAB = 5001          # 312 x 16 + 9: padded to 5008 = 78 x 64 + 16, a ragged last tile for every tile width


def relerr(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _prompt(u, vocab=VOCAB):
    """utterance u's prompt: 2-6 ids, the same in every test (the oracle's rows are shared)"""
    return np.random.default_rng(1000 + u).integers(0, vocab, 2 + (u % 5)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _model(wtype, layers):
    return synth.build_orpheus(synth.orpheus_3b(layers=layers, vocab=VOCAB, ctx=128, weight_type=wtype))


@functools.lru_cache(maxsize=None)
def _oracle(wtype, layers):
    return orc.OrpheusOracle(_model(wtype, layers), act_mode=1)


@functools.lru_cache(maxsize=None)
def _ref_step(wtype, layers, u):
    """(the first greedy id after utterance u's prompt, the logits of the step that feeds it back) from the oracle"""
    o = _oracle(wtype, layers)
    p = _prompt(u)
    first = int(o.decode(p, 0).argmax())
    return first, o.decode([first], len(p)).copy()


def _filled(eng, B):
    """B utterances' prompts into slots 0 .. B-1 -> the step's (slots, ids, positions): every utterance's first id at the position behind its prompt"""
    prompts = [_prompt(u) for u in range(B)]
    first = eng.generate_batch(prompts, 1, stop_id=VOCAB + 5)
    return list(range(B)), [int(f[0]) for f in first], [len(p) for p in prompts]


def _check_rows_against_oracle(wtype, layers, lg, ids, rows, what):
    for u in rows:
        first, ref = _ref_step(wtype, layers, u)
        if ids[u] != first:   # the engine's prompt pass took another id inside the flip bound: the oracle follows the engine's id
            o = _oracle(wtype, layers)
            o.decode(_prompt(u), 0)
            ref = o.decode([ids[u]], len(_prompt(u)))
        err = relerr(lg[u], ref)
        print(f"{what} row {u}: rel err {err:.3e}")
        assert err < TOL_Q, (what, u, err)


def test_creation_accepts_256_slots_and_refuses_257():
    cfg = synth.orpheus_tiny()
    eng = hip.OrpheusEngine(cfg, max_seqs=256)
    eng.close()
    with pytest.raises(hip.HipError, match="max_seqs.*256"):
        hip.OrpheusEngine(cfg, max_seqs=257)


@pytest.mark.parametrize("wtype", [gguf.Q4_0, gguf.Q8_0])
def test_step_logits_of_65_129_and_256_rows_match_the_oracle(wtype):
    """One step of B rows at the 3B widths (two layers): 65 = a full 64-row tile and a 1-row tile, 129 = the same for the 128-row shapes, 256 = RMAX.
    Rows 0, 63, 64 and B - 1 against the oracle fed that utterance's history, and the selected ids are the logits' arg-max.  B = 129 once more over an
    fp16 K/V cache."""
    model = _model(wtype, 2)
    eng = hip.OrpheusEngine(model.cfg, max_seqs=256)
    eng.load(model)
    assert eng.debug_read("l_tile_tables", 1)[0] == 2 * 4 + 1
    for B in (65, 129, 256):
        slots, ids, pos = _filled(eng, B)
        lg, tok = eng.step_batch(slots, ids, pos)
        assert lg.shape == (B, VOCAB)
        _check_rows_against_oracle(wtype, 2, lg, ids, (0, 63, 64, B - 1), f"B={B}")
        assert tok.tolist() == lg.argmax(1).tolist()
    eng.close()
    eng = hip.OrpheusEngine(model.cfg, max_seqs=129, flags=hip.FLAG_KV_F16)
    eng.load(model)
    assert eng.debug_read("l_kv_elem", 1)[0] == 2
    slots, ids, pos = _filled(eng, 129)
    lg, tok = eng.step_batch(slots, ids, pos)
    _check_rows_against_oracle(wtype, 2, lg, ids, (0, 63, 64, 128), "B=129 fp16 cache")
    assert tok.tolist() == lg.argmax(1).tolist()
    eng.close()


def test_tiled_path_against_the_16_feature_kernel():
    """The same 200 rows (Q5_0, 3B widths, two layers) through qgemm_tile_kernel and, with tune("qtile_min_rows") = 0, through qgemm16_kernel: a row
    without a flipped activation code differs only in summation order (median row error < 1e-5 of the row's range), a row with one stays inside the
    flip bound (max < 3e-2).  Measured on MI355X: 0.645 of the 200 rows below 1e-5 (129 rows), median 2.6e-7, max 1.1e-2."""
    model = _model(gguf.Q5_0, 2)
    B = 200
    eng = hip.OrpheusEngine(model.cfg, max_seqs=B)
    eng.load(model)
    slots, ids, pos = _filled(eng, B)
    tiled, _ = eng.step_batch(slots, ids, pos)
    eng.tune("qtile_min_rows", 0)
    plain, _ = eng.step_batch(slots, ids, pos)     # the step rewrites the cache rows it appended: the same inputs
    eng.close()
    err = np.abs(tiled - plain).max(1) / np.abs(plain).max(1)
    share = float((err < 1e-5).mean())
    print(f"tiled against 16-feature kernel, 200 rows: {share:.3f} of the rows below 1e-5, median {np.median(err):.3e}, max {err.max():.3e}")
    assert err.max() < TOL_Q
    assert np.median(err) < 1e-5


def test_every_tile_shape_and_slab_count():
    """B = 200 on one layer at the 3B widths (Q4_0): every tile shape 0 .. 4 forced with 1 / 2 / 4 / 8 K slices of the o (K = 3072) and down (K = 8192)
    projections — 8 slabs are what l_parts holds.  Rows 0, 63, 64 and 199 against the oracle; the 5001-feature head is the ragged last tile for every
    tile width: a store of row 63's last tile behind column 5008 would land in row 64's first logits, which the comparison of the consecutive rows 63
    and 64 sees."""
    model = _model(gguf.Q4_0, 1)
    B = 200
    eng = hip.OrpheusEngine(model.cfg, max_seqs=B)
    eng.load(model)
    slots, ids, pos = _filled(eng, B)
    for shape in range(5):
        for ks in (1, 2, 4, 8):
            eng.tune("qtile_shape", shape)
            eng.tune("qtile_ks", ks)
            lg, tok = eng.step_batch(slots, ids, pos)
            _check_rows_against_oracle(gguf.Q4_0, 1, lg, ids, (0, 63, 64, 199), f"shape {shape} ks {ks}")
            assert tok.tolist() == lg.argmax(1).tolist(), (shape, ks)
    eng.close()


def test_attention_width_that_is_no_multiple_of_256():
    """9 query heads: the o projection has K = 1152 = 4 x 256 + 128.  The upload keeps integer codes only for matrices whose K is a multiple of 256, so
    this o projection is fp32 and has no scale table: inside one layer qkv, gate | up and down run on the tiled GEMM and o on the 16-feature path, which
    reads the attention's fp32 rows and adds into the residual stream itself.  Rows 0, 64 and 69 of a 70-row step against the oracle."""
    model = synth.build_orpheus(synth.orpheus_tiny(heads=9, kv_heads=3, weight_type=gguf.Q4_0))
    cfg = model.cfg
    B = 70
    prompts = [_prompt(u, cfg.vocab) for u in range(B)]
    eng = hip.OrpheusEngine(cfg, max_seqs=B)
    eng.load(model)
    assert eng.debug_read("l_tile_tables", 1)[0] == cfg.layers * 3 + 1       # no table for o
    first = eng.generate_batch(prompts, 1, stop_id=cfg.vocab + 5)
    lg, tok = eng.step_batch(list(range(B)), [int(f[0]) for f in first], [len(p) for p in prompts])
    o = orc.OrpheusOracle(model, act_mode=1)
    for u in (0, 64, 69):
        o.decode(prompts[u], 0)
        ref = o.decode([int(first[u][0])], len(prompts[u]))
        err = relerr(lg[u], ref)
        print(f"9 heads, row {u}: rel err {err:.3e}")
        assert err < TOL_Q, (u, err)
    assert tok.tolist() == lg.argmax(1).tolist()
    eng.close()


def _teacher_forced(o, prompt, ids, tol):
    """every id of `ids` inside the oracle's flip bound when the oracle is fed the same history -> whether every margin exceeded the bound"""
    ref = o.decode(prompt, 0)
    clear = True
    for s, t in enumerate(ids):
        bound = 2 * tol * np.abs(ref).max()
        assert ref[t] >= ref.max() - bound, (s, t, int(ref.argmax()))
        top2 = np.partition(ref, -2)[-2:]
        clear = clear and (top2[1] - top2[0] > bound)
        if s + 1 < len(ids):
            ref = o.decode([t], len(prompt) + s)
    return clear


@pytest.mark.parametrize("wtype,tol", [(gguf.Q4_0, TOL_Q), (gguf.F32, 2e-4)])
def test_generation_loop_at_70_utterances(wtype, tol):
    """tts_hip_orpheus_generate_batch with 70 utterances: ragged prompts, a stop id that rows meet at different steps, so the live count crosses 64
    downwards inside the generation (the tiled GEMM, then the streaming one; F32 matrices stay on the 16-feature path above 64 rows).  Every id is the
    oracle's arg-max up to the bound when the oracle is teacher-forced with the utterance's ids; where every margin exceeds the bound the ids are
    those of the one-sequence generate_greedy."""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=wtype))
    cfg = model.cfg
    n_utt, max_new, never = 70, 12, cfg.vocab + 5
    prompts = [_prompt(u, cfg.vocab) for u in range(n_utt)]
    eng = hip.OrpheusEngine(cfg, max_seqs=n_utt)
    eng.load(model)
    free = eng.generate_batch(prompts, max_new, stop_id=never)
    # the id that ends the most utterances early while at least one runs on: rows leave at different steps
    best, stop = -1, 0
    for t in range(cfg.vocab):
        ends = [g.tolist().index(t) for g in free if t in g.tolist()[:-1]]
        if len(ends) < n_utt and len(ends) > best and len(set(ends)) > 1:
            best, stop = len(ends), t
    assert best >= 7, "no stop id takes the live count from 70 to 64 or fewer: other prompts"
    got = eng.generate_batch(prompts, max_new, stop_id=stop)
    lens = sorted(len(g) for g in got)
    assert lens[6] < lens[-1] and len(set(lens)) > 2, lens      # at least seven rows are gone while others still generate
    o = orc.OrpheusOracle(model, act_mode=1)
    compared = 0
    for u in range(n_utt):
        assert len(got[u]) == max_new or got[u][-1] == stop
        assert stop not in got[u][:-1].tolist()
        if _teacher_forced(o, prompts[u], got[u].tolist(), tol):
            assert got[u].tolist() == eng.generate_greedy(prompts[u], max_new, stop_id=stop).tolist(), u
            compared += 1
    print(f"{compared} of {n_utt} utterances with every margin above the bound: equal to generate_greedy")
    assert compared >= 1
    eng.close()


def test_continuous_session_of_70_slots_and_100_requests():
    """A mixed session of 70 slots (Q4_0): 100 requests, so freed slots are refilled; steps are enqueued in chunks (stream_launch / stream_wait);
    one live slot is dropped.  Every request but the dropped one comes back exactly once; six greedy utterances — the first, the last, two refills,
    the neighbour of the dropped slot and the one that finishes first — pass the teacher-forced check."""
    model = synth.build_orpheus(synth.orpheus_tiny(weight_type=gguf.Q4_0))
    cfg = model.cfg
    n_slots, n_req, max_new = 70, 100, 10
    rng = np.random.default_rng(5)
    prompts = [_prompt(u, cfg.vocab) for u in range(n_req)]
    uni = rng.random((n_req, max_new), dtype=np.float32)
    settings = [dict(top_k=8, temperature=0.9, repetition_penalty=1.1, top_p=0.9) if u % 7 == 3 else None for u in range(n_req)]
    eng = hip.OrpheusEngine(cfg, max_seqs=n_slots)
    eng.load(model)
    free0 = eng.generate_batch(prompts[:n_slots], max_new, stop_id=cfg.vocab + 5)
    stop = int(free0[10][3])                      # utterance 10 (greedy) ends with its fourth id; others meet it elsewhere or never
    eng.stream_begin_mixed(n_slots, max_new, stop)
    slot_req, out, nxt, dropped = {}, {}, 0, None
    free = list(range(n_slots))
    first_done = None
    for _ in range(200):
        take = min(len(free), n_req - nxt)
        if take:
            sl = [free.pop(0) for _ in range(take)]
            eng.stream_admit_mixed(sl, prompts[nxt:nxt + take], settings[nxt:nxt + take], uni[nxt:nxt + take])
            for i, s in enumerate(sl):
                slot_req[s] = nxt + i
            nxt += take
        if dropped is None and nxt >= n_slots:
            dropped = slot_req.pop(20)
            eng.stream_drop([20])
            free.append(20)
            continue
        if not slot_req:
            break
        eng.stream_launch(2)
        toks, cnt, done, fin = eng.stream_wait()
        for s, n in fin:
            r = slot_req.pop(s)
            assert r not in out
            out[r] = eng.stream_collect(s, n).tolist()
            assert out[r] == toks[s, :n].tolist()
            if first_done is None:
                first_done = r
            free.append(s)
    eng.stream_end()
    assert sorted(out) == [r for r in range(n_req) if r != dropped]
    greedy = [r for r in out if settings[r] is None]
    refills = [r for r in greedy if r >= n_slots]
    first_greedy = first_done if settings[first_done] is None else greedy[0]
    checked = {greedy[0], max(greedy), refills[0], refills[-2], 21 if settings[21] is None else 19, first_greedy}
    o = orc.OrpheusOracle(model, act_mode=1)
    for r in sorted(checked):
        assert len(out[r]) == max_new or out[r][-1] == stop
        _teacher_forced(o, prompts[r], out[r], TOL_Q)
    eng.close()


def test_mixed_selection_of_129_rows_equals_the_one_row_sampler():
    """tts_hip_orpheus_sample_logits_rows_mixed at 129 rows (a context of 129 slots): greedy rows, sampled rows and rows with top_p < 1 together,
    each against tts_hip_orpheus_sample_logits with that row's setting (pinned to the reference sampler by tests/test_gpu_orpheus.py)."""
    cfg = synth.orpheus_tiny(vocab=VOCAB)
    eng = hip.OrpheusEngine(cfg, max_seqs=129)
    eng.load(synth.build_orpheus(cfg))
    rng = np.random.default_rng(129)
    n = 129
    kinds = [None, dict(top_k=50, temperature=1.0, repetition_penalty=1.0, top_p=1.0), dict(top_k=7, temperature=0.9, repetition_penalty=1.5, top_p=1.0),
             dict(top_k=50, temperature=0.8, repetition_penalty=1.1, top_p=0.9)]
    settings = [kinds[r % 4] for r in range(n)]
    lg = (rng.standard_normal((n, VOCAB)) * 3.0).astype(np.float32)
    last = rng.integers(0, VOCAB, n).astype(np.int32)
    cnt = rng.integers(1, 5, n).astype(np.uint32)
    u = rng.random(n, dtype=np.float32)
    tok, last2, cnt2 = eng.sample_logits_rows_mixed(lg, settings, u, last_id=last, rep_count=cnt)
    for r, s in enumerate(settings):
        if s is None:
            want, state = int(lg[r].argmax()), (int(last[r]), int(cnt[r]))
        else:
            want, l, c = eng.sample_logits(lg[r], float(u[r]), last_id=int(last[r]), rep_count=int(cnt[r]), **s)
            state = (l, c) if s["repetition_penalty"] != 1.0 else (int(last[r]), int(cnt[r]))
        assert int(tok[r]) == want, (r, s)
        assert (int(last2[r]), int(cnt2[r])) == state, (r, s)
    eng.close()


def test_contexts_of_at_most_64_slots_are_unchanged():
    """A context of 8 slots plans no transposed scale table (one of 65 slots plans one per quantised matrix), and its 6-row step does not depend on
    tune("qtile_min_rows"): bit-equal logits at the default and at 0."""
    model = _model(gguf.Q4_0, 1)
    eng = hip.OrpheusEngine(model.cfg, max_seqs=8)
    eng.load(model)
    assert eng.debug_read("l_tile_tables", 1)[0] == 0
    slots, ids, pos = _filled(eng, 6)
    a, _ = eng.step_batch(slots, ids, pos)
    eng.tune("qtile_min_rows", 0)
    b, _ = eng.step_batch(slots, ids, pos)
    assert np.array_equal(a, b)
    eng.close()
    big = hip.OrpheusEngine(model.cfg, max_seqs=65)
    big.load(model)
    assert big.debug_read("l_tile_tables", 1)[0] == 5
    big.close()
