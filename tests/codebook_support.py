"""Dead-code revival and usage counting — numpy restatement of the rule and the shared test cases.

The rule (include/rqvae_hip.h rq_codebook_revive, modules/codebook_revival.py), restated independently:
level l's dead codes are {k : counts[l][k] < min_count} in ascending k; the j-th takes donor row
(s_l + j) mod B of res[l] with s_l = splitmix64(seed, l) mod B (unsigned 64-bit, oracle.dropout.splitmix64);
the codeword becomes a bit copy of the donor, its rows of both moments +0.0. No import of the product package.
"""
import numpy as np

from oracle.dropout import splitmix64


def usage_ref(ids, K, counts=None):
    """counts (L, K) int64 += the per-level histogram of ids (B, L); ids outside [0, K) are skipped."""
    ids = np.asarray(ids, np.int64)
    L = ids.shape[1]
    out = np.zeros((L, K), np.int64) if counts is None else np.array(counts, np.int64)
    for l in range(L):
        col = ids[:, l]
        np.add.at(out[l], col[(col >= 0) & (col < K)], 1)
    return out


def donor_rows(seed, level, n_dead, B):
    """Donor rows of a level's dead codes, in the order of the codes."""
    s = int(splitmix64(seed, level)[0]) % B
    return (s + np.arange(n_dead, dtype=np.int64)) % B


def revive_ref(weights, counts, res, min_count, seed, exp_avg=None, exp_avg_sq=None):
    """-> dict(weights (L, K, D), exp_avg, exp_avg_sq (or None), revived (L, K) bool, n_revived (L,) int64); the
    inputs are not modified."""
    w = np.array(weights, np.float32)
    m = None if exp_avg is None else np.array(exp_avg, np.float32)
    v = None if exp_avg_sq is None else np.array(exp_avg_sq, np.float32)
    L, K, _ = w.shape
    B = res.shape[1]
    assert B >= K
    revived = np.zeros((L, K), bool)
    for l in range(L):
        dead = np.flatnonzero(np.asarray(counts[l]) < min_count)
        rows = donor_rows(seed, l, dead.size, B)
        w[l, dead] = res[l, rows]
        revived[l, dead] = True
        if m is not None:
            m[l, dead] = 0.0
            v[l, dead] = 0.0
    return dict(weights=w, exp_avg=m, exp_avg_sq=v, revived=revived, n_revived=revived.sum(1).astype(np.int64))


def bits(a):
    """fp32 array as its uint32 bit patterns (a bitwise comparison also sees -0.0, NaN payloads, denormals)."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# (name, L, K, D, B, min_count, with_moments)
REVIVE_CASES = [
    ("one", 1, 1, 8, 1, 1, True),
    ("wrap", 3, 32, 16, 32, 1, True),          # level 0 all dead (n_dead = K = B: wraps), level 1 none, level 2 mixed
    ("chunk", 2, 300, 64, 1000, 1, True),      # dead codes on both sides of k = 256
    ("many", 1, 5000, 8, 5000, 1, True),       # many 256-code chunks
    ("min3", 3, 32, 16, 32, 3, True),          # min_count = 3
    ("nomoments", 2, 300, 64, 1000, 1, False),
]
_CACHE = {}


def revive_case(name):
    """Inputs of a case and the restatement's result, computed once and shared (read-only):
    dict(L, K, D, B, min_count, seed, weights (L,K,D), counts (L,K), res (L,B,D), exp_avg, exp_avg_sq, ref)."""
    if name in _CACHE:
        return _CACHE[name]
    _, L, K, D, B, min_count, with_m = next(c for c in REVIVE_CASES if c[0] == name)
    g = np.random.Generator(np.random.PCG64(sum(map(ord, name)) + 1000 * K))
    w = g.standard_normal((L, K, D), dtype=np.float32)
    res = g.standard_normal((L, B, D), dtype=np.float32)
    # bit patterns an arithmetic "copy" would change: -0.0, a denormal, a NaN with a payload
    special = np.array([0x80000000, 0x00000001, 0x7FC01234], np.uint32).view(np.float32)
    res.reshape(-1)[: min(3, res.size)] = special[: min(3, res.size)]
    res[:, :, D - 1] = np.where(g.random((L, B)) < 0.1, np.float32(-0.0), res[:, :, D - 1])
    m = g.standard_normal((L, K, D), dtype=np.float32) if with_m else None
    v = (g.random((L, K, D), dtype=np.float32) + np.float32(0.5)) if with_m else None
    counts = g.integers(0, 6, size=(L, K)).astype(np.int64)
    if name in ("wrap", "min3"):
        counts[0] = 0
        counts[1] = 5
    if name in ("chunk", "nomoments"):
        counts[:, [3, 255, 256, 257, 299]] = 0
        counts[:, [0, 254, 258]] = 2
    if name == "one":
        counts[:] = 0
    seed = 0x9E3779B97F4A7C15 ^ (K * 1315423911 + L)   # above 2^63: the unsigned reading matters
    case = dict(L=L, K=K, D=D, B=B, min_count=min_count, seed=seed, weights=w, counts=counts, res=res, exp_avg=m,
                exp_avg_sq=v, ref=revive_ref(w, counts, res, min_count, seed, m, v))
    for a in (w, counts, res, m, v):
        if a is not None:
            a.setflags(write=False)
    _CACHE[name] = case
    return case


def check_revived(case, weights, exp_avg, exp_avg_sq, revived, n_revived):
    """Assert a result (numpy arrays; weights (L,K,D)) equals the restatement bit for bit, and that live rows and their
    moments are the inputs' bits."""
    ref = case["ref"]
    assert np.array_equal(np.asarray(n_revived, np.int64), ref["n_revived"])
    if revived is not None:
        assert np.array_equal(np.asarray(revived).astype(bool), ref["revived"])
    assert np.array_equal(bits(weights), bits(ref["weights"]))
    live = ~ref["revived"]
    assert np.array_equal(bits(np.asarray(weights)[live]), bits(case["weights"][live]))
    if case["exp_avg"] is not None:
        for got, key in ((exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            assert np.array_equal(bits(got), bits(ref[key]))
            assert np.array_equal(bits(np.asarray(got)[live]), bits(case[key][live]))
            assert not bits(np.asarray(got)[ref["revived"]]).any()   # +0.0 exactly
