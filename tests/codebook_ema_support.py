"""EMA-maintained codebooks — the fp64 reference of the rule and the seeded case table shared by the host and GPU
tests. No import of the product package.

The rule (include/rqvae_hip.h, modules/codebook_ema.py), restated independently. One forward with level inputs
res (L, B, D) and ids (B, L) accumulates n[l][k] += #{b : ids[b][l] == k} and s[l][k] += sum of those rows (ids
outside [0, K) skipped); the update with decay g and smoothing eps is

    N' = g N + (1 - g) n;  S' = g S + (1 - g) s;  T[l] = sum_k N'[l][k]
    N~ = (N' + eps) / (T + K eps) * T;  W[l][k][:] = S'[l][k][:] / N~[l][k]

Bounds, from fp32 rounding with u = 2^-24 (none is tuned):
  * a sum of m fp32 rows in any order: |err| <= m u sum|x| per element, plus u |s| for the add into the accumulator;
  * N', S' from the same fp32 inputs: |err| <= 4 u (|g old| + |(1 - g) new|) (g and 1 - g rounded to fp32, two
    products, one sum);
  * W against the rule evaluated in fp64 on the implementation's own fp32 N', S': relative (K + 8) u (the sum T of K
    positive terms, then a handful of roundings).
"""
import numpy as np

U = 2.0 ** -24

# (name, B, D, K, L, kind)
STATS_CASES = [
    ("ml32m", 1000, 32, 256, 3, "random"),        # the LDS form at the ML-32M dims, ragged last chunk
    ("k5", 300, 8, 5, 1, "random"),               # K not a multiple of the waves' code ranges
    ("collapsed", 5000, 64, 256, 2, "one"),       # every row on one code per level: the longest fixed-order chain
    ("sparse", 5000, 64, 256, 2, "few"),          # codes nothing selects: untouched rows of s
    ("tiled", 2000, 64, 4096, 1, "random"),       # above the LDS bound
    ("wide", 40, 1024, 8, 1, "random"),           # the widest row
    ("empty", 0, 32, 256, 3, "random"),           # B = 0: no-op
    ("skip", 300, 16, 32, 2, "skip"),             # ids of -1 and K are skipped
    ("second", 1000, 32, 256, 3, "random"),       # a second batch at ml32m's shape: two calls in a row
    ("chunks", 2500, 32, 256, 3, "random"),       # three row chunks, the last ragged
    ("subblocks", 2500, 512, 4096, 1, "random"),  # a chunk longer than one 1024-row sub-block
]
_CACHE = {}


def stats_ref(res, ids, K):
    """-> n (L, K) int64, s (L, K, D) float64 batch sums, a (L, K, D) float64 sums of |x| (for the bound)."""
    L, B, D = res.shape
    n = np.zeros((L, K), np.int64)
    s = np.zeros((L, K, D), np.float64)
    a = np.zeros((L, K, D), np.float64)
    for l in range(L):
        col = ids[:, l]
        ok = (col >= 0) & (col < K)
        np.add.at(n[l], col[ok], 1)
        x = res[l][ok].astype(np.float64)
        np.add.at(s[l], col[ok], x)
        np.add.at(a[l], col[ok], np.abs(x))
    return n, s, a


def stats_case(name):
    """Inputs of a case and the reference, computed once and shared (read-only): dict(B, D, K, L, res (L,B,D) fp32,
    ids (B,L) int64, n0 (L,K) int64 and s0 (L,K,D) fp32 — what the accumulators hold before the call — n, s, a from
    stats_ref)."""
    if name in _CACHE:
        return _CACHE[name]
    _, B, D, K, L, kind = next(c for c in STATS_CASES if c[0] == name)
    g = np.random.Generator(np.random.PCG64(sum(map(ord, name)) + 7919 * K + D))
    res = g.standard_normal((L, B, D), dtype=np.float32)
    if kind == "one":
        ids = np.tile(g.integers(0, K, size=(1, L)), (B, 1))
    elif kind == "few":
        ids = g.choice(g.permutation(K)[:40], size=(B, L))
    else:
        ids = g.integers(0, K, size=(B, L))
    ids = ids.astype(np.int64)
    if kind == "skip":
        ids[::7, 0] = -1
        ids[3::5, 1] = K
        ids[1::11, 0] = K + 3
    n0 = g.integers(0, 1000, size=(L, K)).astype(np.int64)
    s0 = g.standard_normal((L, K, D), dtype=np.float32)
    n, s, a = stats_ref(res, ids, K)
    case = dict(B=B, D=D, K=K, L=L, res=res, ids=ids, n0=n0, s0=s0, n=n, s=s, a=a)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[name] = case
    return case


def check_stats(case, n_got, s_got, n0=None, s0=None):
    """Assert accumulators that held n0, s0 (default: the case's) hold the reference afterwards: n exactly, s within
    m u sum|x| + u |s|; rows of s no id selected keep their bits."""
    n0 = case["n0"] if n0 is None else n0
    s0 = case["s0"] if s0 is None else s0
    assert np.array_equal(np.asarray(n_got, np.int64), n0 + case["n"])
    want = s0.astype(np.float64) + case["s"]
    bound = case["n"][:, :, None] * U * case["a"] + U * np.abs(want)
    err = np.abs(np.asarray(s_got, np.float64) - want)
    assert (err <= bound).all(), float((err - bound).max())
    idle = case["n"] == 0
    got = np.ascontiguousarray(s_got, np.float32)
    assert np.array_equal(got[idle].view(np.uint32), np.ascontiguousarray(s0[idle]).view(np.uint32))


def apply_ref(N, S, n, s, decay, eps):
    """The update in fp64 -> (N', S', W, bound_N, bound_S); inputs are taken as data (cast to fp64)."""
    N, S, n, s = (np.asarray(t, np.float64) for t in (N, S, n, s))
    K = N.shape[1]
    Np = decay * N + (1.0 - decay) * n
    Sp = decay * S + (1.0 - decay) * s
    bN = 4 * U * (np.abs(decay * N) + np.abs((1.0 - decay) * n))
    bS = 4 * U * (np.abs(decay * S) + np.abs((1.0 - decay) * s))
    return Np, Sp, weights_ref(Np, Sp, eps, K), bN, bS


def weights_ref(Np, Sp, eps, K):
    """W of the rule in fp64 from N' (L, K) and S' (L, K, D) taken as data."""
    Np, Sp = np.asarray(Np, np.float64), np.asarray(Sp, np.float64)
    T = Np.sum(1, keepdims=True)
    nt = (Np + eps) / (T + K * eps) * T
    return Sp / nt[:, :, None]


def check_apply(N0, S0, n, s, decay, eps, N_got, S_got, W_got, n_after, s_after):
    """Assert one update's results (numpy; W_got (L, K, D)) against the fp64 rule within the module's bounds."""
    K = N0.shape[1]
    Np, Sp, _, bN, bS = apply_ref(N0, S0, n, s, decay, eps)
    eN = np.abs(np.asarray(N_got, np.float64) - Np)
    eS = np.abs(np.asarray(S_got, np.float64) - Sp)
    assert (eN <= bN).all(), float((eN - bN).max())
    assert (eS <= bS).all(), float((eS - bS).max())
    W = weights_ref(N_got, S_got, eps, K)
    eW = np.abs(np.asarray(W_got, np.float64) - W)
    assert (eW <= (K + 8) * U * np.abs(W)).all(), float((eW / np.maximum(np.abs(W), 1e-300)).max() / U)
    assert not np.asarray(n_after).any() and not np.asarray(s_after).any()


# (name, stats case the statistics come from, decay, eps)
APPLY_CASES = [("ml32m", "ml32m", 0.99, 1e-5), ("k5", "k5", 0.9, 1e-5), ("collapsed", "collapsed", 0.99, 1e-5),
               ("tiled", "tiled", 0.999, 1e-3), ("wide", "wide", 0.5, 1e-5), ("nodecay", "skip", 0.0, 1e-5)]


def apply_case(name):
    """dict(decay, eps, N0 (L,K) fp32 > 0, S0 (L,K,D) fp32, n (L,K) int64, s (L,K,D) fp32): a state and accumulated
    statistics (the stats case's batch sums rounded to fp32). Shared, read-only."""
    key = ("apply", name)
    if key in _CACHE:
        return _CACHE[key]
    _, src, decay, eps = next(c for c in APPLY_CASES if c[0] == name)
    c = stats_case(src)
    g = np.random.Generator(np.random.PCG64(sum(map(ord, name)) + 31))
    N0 = (g.random((c["L"], c["K"]), dtype=np.float32) * 8 + np.float32(0.01)).astype(np.float32)
    S0 = g.standard_normal((c["L"], c["K"], c["D"]), dtype=np.float32)
    case = dict(decay=decay, eps=eps, N0=N0, S0=S0, n=c["n"].copy(), s=c["s"].astype(np.float32), L=c["L"], K=c["K"],
                D=c["D"])
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = case
    return case
