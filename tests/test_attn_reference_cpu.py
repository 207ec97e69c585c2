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
