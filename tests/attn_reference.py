"""Plain numpy float64 restatement of what one launch of the Llama / Dia attention kernels computes (csrc/llama_kernels.h): the reference of
tests/test_gpu_llama_attention.py, and of the Parler attention kernels (csrc/parler_kernels.h, tests/test_gpu_parler_attention.py: head width 64,
NKV == NH), pinned to torch by tests/test_attn_reference_cpu.py.  One query row, all heads; K / V are cache rows [keys][NKV * hd]; hd is the
head width (HD = 128 by default)."""
import numpy as np

HD = 128


def kv_head(h, NH, NKV):
    """the k/v head a query head reads (grouped-query attention)"""
    return h // (NH // NKV)


def _softmax_rows(Q, K, V, Ts, scale, NH, NKV, dtype, hd=HD):
    """rows r with Ts[r] keys each of one cache: per head the probabilities [R][Tmax] (zero beyond a row's keys), the values [Tmax][HD] and the rows [R][HD]"""
    Q = np.asarray(Q, dtype=dtype).reshape(-1, NH, hd)
    Ts = np.asarray(Ts, dtype=np.int64).reshape(-1)
    Tmax = int(Ts.max())
    K = np.asarray(K[:Tmax], dtype=dtype).reshape(Tmax, NKV, hd)
    V = np.asarray(V[:Tmax], dtype=dtype).reshape(Tmax, NKV, hd)
    live = np.arange(Tmax)[None, :] < Ts[:, None]
    P, Vh, O = [], [], []
    for h in range(NH):
        kh = kv_head(h, NH, NKV)
        s = np.where(live, (Q[:, h, :] @ K[:, kh, :].T) * dtype(scale), dtype(-np.inf))
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p = p / p.sum(axis=1, keepdims=True, dtype=dtype)
        P.append(p); Vh.append(V[:, kh, :]); O.append(p @ V[:, kh, :])
    return P, Vh, O


def attention_rows(Q, K, V, Ts, scale, NH, NKV, dtype=np.float64, hd=HD):
    """attention() for rows [R][NH * hd] that read the same cache, row r over keys [0, Ts[r]) -> [R][NH * hd]"""
    _, _, O = _softmax_rows(Q, K, V, Ts, scale, NH, NKV, dtype, hd)
    return np.concatenate(O, axis=1)


def attention(q, K, V, T, scale, NH, NKV, dtype=np.float64, hd=HD):
    """softmax over keys [0, T) of q . K * scale, times V, query head h on k/v head kv_head(h) -> [NH * HD].
    dtype=np.float32 evaluates the same formula in float32 (the yardstick of the tolerance, not a model of any kernel's summation order)."""
    return attention_rows(np.asarray(q).reshape(1, -1), K, V, [T], scale, NH, NKV, dtype, hd)[0]


def drop_key(q, K, V, T, scale, NH, NKV, j, hd=HD):
    """attention() without key j"""
    keep = np.ones(T, dtype=bool)
    keep[j] = False
    return attention(q, np.asarray(K[:T])[keep], np.asarray(V[:T])[keep], T - 1, scale, NH, NKV, hd=hd)


def drop_shifts(Q, K, V, Ts, scale, NH, NKV, keys_of, hd=HD):
    """per row r: {j: max|attention - drop_key(j)| / max|attention|} for j in keys_of(r, Ts[r]), from one softmax: without key j the row is
    (o - p_j v_j) / (1 - p_j), so it moves by p_j (o - v_j) / (1 - p_j).  Equal to drop_key() (test_attn_reference_cpu.py)."""
    P, Vh, O = _softmax_rows(Q, K, V, Ts, scale, NH, NKV, np.float64, hd)
    ref = np.concatenate(O, axis=1)
    out = []
    for r, T in enumerate(np.asarray(Ts).reshape(-1)):
        d = {}
        for j in keys_of(r, int(T)):
            d[j] = max(float(np.abs(P[h][r, j] * (O[h][r] - Vh[h][j]) / (1.0 - P[h][r, j])).max()) for h in range(NH)) / float(np.abs(ref[r]).max())
        out.append(d)
    return out


def fold_partials(m, s, o):
    """the float64 merge of key slices: m [nz] the slices' maxima (-inf: an empty slice, skipped whatever its s and o hold), s [nz] their sums of
    exp(score - m), o [nz][hd] their unnormalised rows sum exp(score - m) v -> the row [hd]"""
    m, s, o = np.asarray(m, dtype=np.float64), np.asarray(s, dtype=np.float64), np.asarray(o, dtype=np.float64)
    live = m != -np.inf
    f = np.exp(m[live] - m[live].max())
    return (f[:, None] * o[live]).sum(axis=0) / (f * s[live]).sum()


def slice_partials(q, K, V, t0, t1, scale, dtype=np.float64):
    """one head's partial over keys [t0, t1) as the kernels leave it: (max, sum, unnormalised row); (-inf, 0, 0) for an empty slice.  q [hd], K / V [keys][hd]"""
    q = np.asarray(q, dtype=dtype)
    if t1 <= t0:
        return -np.inf, 0.0, np.zeros(q.shape[0], dtype=dtype)
    sc = (np.asarray(K[t0:t1], dtype=dtype) @ q) * dtype(scale)
    p = np.exp(sc - sc.max())
    return sc.max(), p.sum(), p @ np.asarray(V[t0:t1], dtype=dtype)


def fold_slabs(buf, n_parts, part_stride, row, ld, width):
    """the query row of a projection that left n_parts K-slice slabs part_stride floats apart: summed in slab order, in float32 as the kernels do"""
    buf = np.asarray(buf, dtype=np.float32)
    x = buf[row * ld: row * ld + width].copy()
    for p in range(1, n_parts):
        x += buf[p * part_stride + row * ld: p * part_stride + row * ld + width]
    return x


def rope_thetas(pos, theta_scale, n=HD // 2):
    """ggml's angles: theta_0 = float32(pos), theta_{i+1} = theta_i * theta_scale, every product rounded to float32"""
    t = np.empty(n, dtype=np.float32)
    th, sc = np.float32(pos), np.float32(theta_scale)
    for i in range(n):
        t[i] = th
        th = np.float32(th * sc)
    return t


def rope_neox(q, pos, theta_scale, NH):
    """ggml_rope NEOX on every head of a row: pairs (i, i + HD/2); the angles iterated in float32 (rope_thetas), cos / sin and the rotation in float64"""
    q = np.asarray(q, dtype=np.float64).reshape(NH, HD)
    th = rope_thetas(pos, theta_scale).astype(np.float64)
    cs, sn = np.cos(th), np.sin(th)
    x0, x1 = q[:, :HD // 2], q[:, HD // 2:]
    return np.concatenate([x0 * cs - x1 * sn, x0 * sn + x1 * cs], axis=1).reshape(NH * HD)


def boundary_keys(T, Rd):
    """the keys next to a batch, pass, round or chunk edge of a row of T keys (Rd: its round or chunk size)"""
    return sorted({j for j in (0, 15, 16, 63, 64, Rd - 1, Rd, T - 1) if 0 <= j < T})


def edge_keys(T, edges):
    """boundary_keys() for a kernel with its own geometry: keys 0 and T - 1 and those of `edges` that exist in a row of T keys"""
    return sorted({j for j in (0, *edges, T - 1) if 0 <= j < T})
