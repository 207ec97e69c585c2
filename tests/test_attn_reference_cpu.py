"""Pins tests/attn_reference.py (the numpy float64 reference of tests/test_gpu_llama_attention.py) to torch float64 on random data."""
import numpy as np
import torch

import attn_reference as ar

HD = ar.HD


def _case(seed, NH, NKV, T, ctx):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(NH * HD).astype(np.float32)
    K = rng.standard_normal((ctx, NKV * HD)).astype(np.float32)
    V = rng.standard_normal((ctx, NKV * HD)).astype(np.float32)
    return q, K, V


def _torch_attention(q, K, V, T, scale, NH, NKV, keep=None):
    q = torch.from_numpy(q).double().reshape(NH, HD)
    K = torch.from_numpy(K[:T]).double().reshape(T, NKV, HD)
    V = torch.from_numpy(V[:T]).double().reshape(T, NKV, HD)
    if keep is not None:
        K, V = K[keep], V[keep]
    rep = NH // NKV
    out = []
    for h in range(NH):
        kh = h // rep
        p = torch.softmax(K[:, kh, :] @ q[h] * scale, dim=0)
        out.append(p @ V[:, kh, :])
    return torch.cat(out).numpy()


def test_attention_matches_torch_float64_with_gqa_mapping():
    for seed, (NH, NKV, T, ctx) in enumerate([(4, 2, 601, 700), (4, 1, 1, 8), (4, 4, 129, 129), (16, 4, 65, 80)]):
        q, K, V = _case(seed, NH, NKV, T, ctx)
        for scale in (1.0 / np.sqrt(HD), 0.05):
            got = ar.attention(q, K, V, T, scale, NH, NKV)
            ref = _torch_attention(q, K, V, T, scale, NH, NKV)
            assert got.dtype == np.float64 and np.abs(got - ref).max() < 1e-13 * max(1.0, np.abs(ref).max())
    # the k/v head of a query head: neither the identity nor constant at 4 heads on 2 groups; rows beyond T take no part
    assert [ar.kv_head(h, 4, 2) for h in range(4)] == [0, 0, 1, 1]
    q, K, V = _case(9, 4, 2, 50, 64)
    a = ar.attention(q, K, V, 50, 0.1, 4, 2)
    K[50:], V[50:] = 7.0, -3.0
    assert np.array_equal(a, ar.attention(q, K, V, 50, 0.1, 4, 2))
    K2 = K.copy()
    K2[:, HD:] = 0.0                       # zero the second k/v head's keys: only heads 2 and 3 may move
    b = ar.attention(q, K2, V, 50, 0.1, 4, 2)
    assert np.array_equal(a[:2 * HD], b[:2 * HD]) and np.abs(a[2 * HD:] - b[2 * HD:]).max() > 1e-3


def test_attention_rows_is_attention_per_row():
    rng = np.random.default_rng(2)
    Q = rng.standard_normal((5, 4 * HD)).astype(np.float32)
    _, K, V = _case(2, 4, 2, 130, 140)
    Ts = [1, 64, 65, 130, 17]
    got = ar.attention_rows(Q, K, V, Ts, 0.09, 4, 2)
    for r, T in enumerate(Ts):
        assert np.abs(got[r] - ar.attention(Q[r], K, V, T, 0.09, 4, 2)).max() < 1e-13
        assert np.abs(got[r] - _torch_attention(Q[r], K, V, T, 0.09, 4, 2)).max() < 1e-13


def test_drop_key_and_its_closed_form():
    q, K, V = _case(3, 4, 2, 300, 300)
    s = 1.0 / np.sqrt(HD)
    full = ar.attention(q, K, V, 300, s, 4, 2)
    keys = [0, 15, 16, 63, 64, 255, 256, 299]
    shifts = ar.drop_shifts(q[None], K, V, [300], s, 4, 2, lambda r, T: keys)[0]
    for j in keys:
        keep = torch.ones(300, dtype=torch.bool)
        keep[j] = False
        ref = _torch_attention(q, K, V, 300, s, 4, 2, keep=keep)
        got = ar.drop_key(q, K, V, 300, s, 4, 2, j)
        assert np.abs(got - ref).max() < 1e-13
        direct = np.abs(got - full).max() / np.abs(full).max()
        assert abs(shifts[j] - direct) < 1e-9 * direct + 1e-15
        assert direct > 1e-5               # N(0,1) data: one key in 300 is far above the rounding of a float32 kernel
    assert ar.boundary_keys(3, 1) == [0, 1, 2] and ar.boundary_keys(1061, 512) == [0, 15, 16, 63, 64, 511, 512, 1060]
    assert ar.boundary_keys(16, 64) == [0, 15]


def test_float32_evaluation_is_the_yardstick_scale():
    """the same formula in float32 stays near 1e-6 of float64 at the key counts of the GPU file (the tolerance there is 4x the largest such distance)"""
    worst = 0.0
    for seed, T in enumerate([513, 1061, 3000]):
        q, K, V = _case(20 + seed, 4, 2, T, T)
        s = 1.0 / np.sqrt(HD)
        ref = ar.attention(q, K, V, T, s, 4, 2)
        f32 = ar.attention(q, K, V, T, s, 4, 2, dtype=np.float32)
        assert f32.dtype == np.float32
        worst = max(worst, float(np.abs(f32 - ref).max() / np.abs(ref).max()))
    assert 1e-8 < worst < 2.5e-6


def test_fold_slabs_sums_in_slab_order_in_float32():
    rng = np.random.default_rng(5)
    ld, width, rows, n_parts, stride = 512, 512, 4, 5, 16 * 512
    buf = (rng.standard_normal(n_parts * stride) * 100).astype(np.float32)
    for r in (0, 3):
        want = buf[r * ld: r * ld + width].copy()
        for p in range(1, n_parts):
            want = (want + buf[p * stride + r * ld: p * stride + r * ld + width]).astype(np.float32)
        got = ar.fold_slabs(buf, n_parts, stride, r, ld, width)
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(ar.fold_slabs(buf, 1, 0, 2, ld, width), buf[2 * ld: 3 * ld])


def _torch_rope(q, pos, theta_scale, NH):
    """ggml_rope NEOX restated in torch: theta iterated in float32 tensors, rotation in float64"""
    th = torch.empty(HD // 2, dtype=torch.float32)
    t, sc = torch.tensor(float(pos), dtype=torch.float32), torch.tensor(theta_scale, dtype=torch.float32)
    for i in range(HD // 2):
        th[i] = t
        t = t * sc
    th = th.double()
    x = torch.from_numpy(np.asarray(q)).double().reshape(NH, HD)
    x0, x1 = x[:, :HD // 2], x[:, HD // 2:]
    return torch.cat([x0 * th.cos() - x1 * th.sin(), x0 * th.sin() + x1 * th.cos()], dim=1).reshape(-1).numpy()


def test_rope_neox_iterates_theta_in_float32():
    """the oracle exposes no rope of its own, so the pin is torch; positions 0 (no rotation), 1 and 300 (Dia's cross query at a late step)"""
    rng = np.random.default_rng(8)
    q = rng.standard_normal(4 * HD).astype(np.float32)
    ts = float(np.float32(10000.0) ** np.float32(-2.0 / HD))
    assert np.array_equal(ar.rope_neox(q, 0, ts, 4), q.astype(np.float64))
    for pos in (1, 300, 3000):
        got = ar.rope_neox(q, pos, ts, 4)
        assert np.abs(got - _torch_rope(q, pos, ts, 4)).max() < 1e-12
        assert abs(np.linalg.norm(got) - np.linalg.norm(q.astype(np.float64))) < 1e-9      # a rotation
    # the iterated float32 theta is NOT the closed form: at position 3000 they are up to ~1e-2 rad apart, which is the reference's semantics
    closed = 3000.0 * (10000.0 ** (-2.0 * np.arange(HD // 2) / HD))
    gap = np.abs(ar.rope_thetas(3000, ts).astype(np.float64) - closed).max()
    assert 1e-5 < gap < 5e-2
    assert np.abs(ar.rope_thetas(1, ts).astype(np.float64) - closed / 3000.0).max() < 1e-5


# ---- head width 64, NKV == NH: Parler's attention (tests/test_gpu_parler_attention.py) -----------------------------------------------------
def _case64(seed, NH, T, rows):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, NH * 64)).astype(np.float32), rng.standard_normal((T, NH * 64)).astype(np.float32),
            rng.standard_normal((T, NH * 64)).astype(np.float32))


def _torch_attention64(q, K, V, T, scale, NH, keep=None):
    q = torch.from_numpy(q).double().reshape(NH, 64)
    K = torch.from_numpy(K[:T]).double().reshape(T, NH, 64)
    V = torch.from_numpy(V[:T]).double().reshape(T, NH, 64)
    if keep is not None:
        K, V = K[keep], V[keep]
    return torch.cat([torch.softmax(K[:, h, :] @ q[h] * scale, dim=0) @ V[:, h, :] for h in range(NH)]).numpy()


def test_head_width_64_attention_rows_match_torch_float64():
    Q, K, V = _case64(31, 4, 1041, 6)
    Ts = [1, 2, 64, 65, 1040, 1041]
    got = ar.attention_rows(Q, K, V, Ts, 0.125, 4, 4, hd=64)
    assert got.shape == (6, 256) and got.dtype == np.float64
    for r, T in enumerate(Ts):
        ref = _torch_attention64(Q[r], K, V, T, 0.125, 4)
        assert np.abs(got[r] - ref).max() < 1e-13
        assert np.abs(ar.attention(Q[r], K, V, T, 0.125, 4, 4, hd=64) - ref).max() < 1e-13
    assert np.abs(got[0] - V[0]).max() == 0.0                   # one key: the row is V[0]
    f32 = ar.attention_rows(Q, K, V, Ts, 0.125, 4, 4, dtype=np.float32, hd=64)
    assert f32.dtype == np.float32 and 1e-9 < np.abs(f32 - got).max() / np.abs(got).max() < 2.5e-6
    # the default width is untouched: the same buffers read as 2 heads of 128 give other rows
    assert np.abs(ar.attention_rows(Q, K, V, Ts, 0.125, 2, 2)[3] - got[3]).max() > 1e-3


def test_head_width_64_drop_shifts_equal_drop_key():
    Q, K, V = _case64(32, 4, 300, 2)
    Ts = [300, 66]
    keys = lambda r, T: ar.edge_keys(T, (15, 16, 63, 64, 74, 75))
    assert keys(0, 300) == [0, 15, 16, 63, 64, 74, 75, 299] and keys(1, 66) == [0, 15, 16, 63, 64, 65] and ar.edge_keys(1, (0, 1)) == [0]
    shifts = ar.drop_shifts(Q, K, V, Ts, 0.125, 4, 4, keys, hd=64)
    for r, T in enumerate(Ts):
        full = ar.attention(Q[r], K, V, T, 0.125, 4, 4, hd=64)
        for j in keys(r, T):
            keep = torch.ones(T, dtype=torch.bool)
            keep[j] = False
            got = ar.drop_key(Q[r], K, V, T, 0.125, 4, 4, j, hd=64)
            assert np.abs(got - _torch_attention64(Q[r], K, V, T, 0.125, 4, keep=keep)).max() < 1e-13
            direct = np.abs(got - full).max() / np.abs(full).max()
            assert abs(shifts[r][j] - direct) < 1e-9 * direct + 1e-15 and direct > 1e-5


def test_fold_partials_of_any_cut_is_the_uncut_row():
    """slices of an arbitrary cut of the keys, empty ones among them (with rubbish in their sum and channels: -inf alone marks them), fold to the uncut row"""
    Q, K, V = _case64(33, 4, 130, 1)
    scale = 0.125
    for T, cuts in [(130, [0, 17, 17, 64, 65, 130, 130, 130]), (3, [0, 1, 2, 3, 3, 3, 3, 3, 3]), (1, [0, 1, 1, 1, 1]), (9, [0, 0, 9]),
                    (128, list(range(0, 129, 8)))]:
        ref = ar.attention(Q[0], K, V, T, scale, 4, 4, hd=64)
        for h in range(4):
            sl = slice(h * 64, (h + 1) * 64)
            parts = [ar.slice_partials(Q[0, sl], K[:, sl], V[:, sl], a, b, scale) for a, b in zip(cuts[:-1], cuts[1:])]
            m, s, o = [p[0] for p in parts], [p[1] for p in parts], np.stack([p[2] for p in parts])
            empty = [i for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])) if a == b]
            assert all(m[i] == -np.inf for i in empty) and (len(empty) > 0 or T == 128)
            for i in empty:
                s[i], o[i] = 7.0, 1e30
            got = ar.fold_partials(m, s, o)
            assert got.dtype == np.float64 and np.abs(got - ref[sl]).max() < 1e-13 * max(1.0, np.abs(ref).max())
    # a lost slice is not forgiven
    parts = [ar.slice_partials(Q[0, :64], K[:, :64], V[:, :64], a, b, scale) for a, b in [(0, 65), (65, 130)]]
    one = ar.fold_partials([parts[0][0]], [parts[0][1]], parts[0][2][None])
    assert np.abs(one - ar.attention(Q[0], K, V, 130, scale, 4, 4, hd=64)[:64]).max() > 1e-3


def test_parler_seeds_keep_every_boundary_key_visible():
    """the sharpness condition of tests/test_gpu_parler_attention.py on the CPU: the oracle's last-layer cache rows of that file's model and ids, queries of the
    same scale (cache rows of another head: W_q and W_k are drawn alike).  Dropping any boundary key of any kernel form moves the float64 row by more than
    the fp16 rows' threshold, the larger of the two (the GPU file asserts the condition again on the device's own tensors)."""
    import oracle as orc
    import test_gpu_parler_attention as tpa
    from tts_cpp_amd import gguf
    model = tpa._model(gguf.F32)
    ids, _ = tpa._ids(16)
    T_all = 1041
    o = orc.ParlerOracle(model, act_mode=1, gelu_mode=1, use_cross=False)
    o.decode(ids[0, :T_all], 0, audio=False, want_logits=False)
    K, V = o.get_kv(model.cfg.layers - 1, T_all)
    Ts = [2, 7, 8, 9, 16, 17, 63, 64, 65, 128, 129, 136, 137, 255, 256, 257, 512, 513, 520, 521, 1040, 1041]
    Q = np.stack([np.roll(K[(37 * i + 11) % T], tpa.HD) for i, T in enumerate(Ts)])
    assert tpa.SHARP16 > tpa.SHARP32
    least = np.inf
    for kernel, nz in [("attn256", 1), ("attn1024", 1), ("fused", 8), ("fused", 4), ("fused", 16), ("rows", 4), ("rows", 1)]:
        shifts = ar.drop_shifts(Q, K, V, Ts, tpa.SCALE, tpa.NH, tpa.NH, lambda r, T: ar.edge_keys(T, tpa._edges(kernel, nz, T)), hd=tpa.HD)
        for T, d in zip(Ts, shifts):
            assert len(d) >= 2 and min(d.values()) >= tpa.SHARP16, (kernel, nz, T, d)
            least = min(least, min(d.values()))
    print(f"least boundary-key shift on the oracle's cache rows: {least:.2e}")
    assert tpa._edges("fused", 8, 1040)[-2:] == (129, 130) and tpa._edges("rows", 4, 33) == (7, 8, 8, 9) and tpa._edges("attn1024", 1, 300)[:4] == (63, 64, 255, 256)
