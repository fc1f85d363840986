"""Shared by the beam-quantize tests (no test file imports another): the fp64 numpy reference of the beam rule, the
plain-Python reference of the collision-resolution rule, and the seeded cases.

The rule (include/rqvae_hip.h, modules/beam_quantize.py): level 0 starts from one beam with residual x; at level l
beam w and code k have the key (|r_w|^2 + |c_k|^2) - 2 r_w.c_k — the expression of oracle.quantize.l2_dist, here
in fp64; the W smallest (key, w, k) survive in that order (a stable argsort of the keys flattened as w K + k); a
survivor's residual is r_w - c_k and its path is its parent's plus k.
"""
import numpy as np

import gen_inputs as gi

SAFE_GAP = 1e-5        # an item is safe when consecutive gaps among its first W + 1 sorted keys exceed
#                        SAFE_GAP (max_w |r_w|^2 + max_k |c_k|^2) at every level: fp32 keys cannot reorder them
MIN_SAFE_SHARE = 0.85

# (B, D, K, L, W, kind, seed)
GPU_CASES = [
    (129, 16, 40, 2, 3, "random", 101),
    (257, 64, 256, 3, 8, "random", 102),
    (64, 32, 256, 3, 16, "random", 103),
    (1, 64, 256, 3, 4, "random", 104),
    (96, 8, 7, 3, 7, "random", 105),       # W = K, K no multiple of anything
    (300, 64, 256, 4, 32, "random", 106),
    (200, 16, 32, 3, 6, "integer", 107),
    (70, 64, 256, 3, 32, "integer", 108),
]


def case_id(c):
    return "%s-B%d-D%d-K%d-L%d-W%d" % (c[5], c[0], c[1], c[2], c[3], c[4])


def make_inputs(B, D, K, L, kind, seed):
    """random: normal values scaled by 1 / sqrt(D), level l's codebook by 0.6 ** l. integer: x in [-3, 3], codebooks
    in [-2, 2] — every key is exact in fp32 and ties are frequent."""
    g = gi.rng(seed)
    if kind == "integer":
        x = g.integers(-3, 4, size=(B, D)).astype(np.float32)
        cbs = g.integers(-2, 3, size=(L, K, D)).astype(np.float32)
    else:
        s = np.float32(1.0 / np.sqrt(D))
        x = g.standard_normal((B, D), dtype=np.float32) * s
        cbs = g.standard_normal((L, K, D), dtype=np.float32) * s
        cbs *= (np.float32(0.6) ** np.arange(L, dtype=np.float32))[:, None, None]
    return x.astype(np.float32), cbs.astype(np.float32)


def beam_ref(x, cbs, W):
    """fp64 reference -> dict(paths (B, W, L) int64, err (B, W) f64, residual (B, W, D) f64, safe (B,) bool,
    scale (B,) f64 = the last level's max_w |r_w|^2 + max_k |c_k|^2)."""
    x = x.astype(np.float64)
    cbs = cbs.astype(np.float64)
    (B, D), (L, K, _) = x.shape, cbs.shape
    res = x[:, None, :]
    paths = np.zeros((B, 1, 0), np.int64)
    safe = np.ones(B, bool)
    rows = np.arange(B)[:, None]
    for l in range(L):
        cb = cbs[l]
        r2 = (res * res).sum(-1, keepdims=True)
        c2 = (cb * cb).sum(-1)
        keys = (r2 + c2[None, None, :]) - (2.0 * res) @ cb.T             # oracle.quantize.l2_dist's expression
        flat = keys.reshape(B, -1)
        order = np.argsort(flat, axis=1, kind="stable")
        head = np.take_along_axis(flat, order[:, :W + 1], 1)
        scale = r2.max(axis=(1, 2)) + c2.max()
        safe &= (np.diff(head, axis=1) > SAFE_GAP * scale[:, None]).all(1)
        top = order[:, :W]
        parent, code = top // K, top % K
        err = np.take_along_axis(flat, top, 1)
        res = res[rows, parent] - cb[code]
        paths = np.concatenate([paths[rows, parent], code[:, :, None]], 2)
    return dict(paths=paths, err=err, residual=res, safe=safe, scale=scale)


_CASES = {}


def case(c):
    """(x, cbs, reference) of one GPU_CASES entry, computed once and shared."""
    if c not in _CASES:
        B, D, K, L, W, kind, seed = c
        x, cbs = make_inputs(B, D, K, L, kind, seed)
        _CASES[c] = (x, cbs, beam_ref(x, cbs, W))
    return _CASES[c]


def path_residual(x, cbs, paths):
    """x - sum_l c of every path, fp64: (B, W, D)."""
    res = np.repeat(x.astype(np.float64)[:, None, :], paths.shape[1], 1)
    for l in range(paths.shape[2]):
        res = res - cbs[l].astype(np.float64)[paths[:, :, l]]
    return res


def check_invariants(x, cbs, paths, err, residual, scale):
    """What holds for every case, W = 32 included: sorted beams, distinct paths, residual and err of the item's own
    paths (fp64 recomputation)."""
    B, W, L = paths.shape
    assert paths.min() >= 0 and paths.max() < cbs.shape[1]
    assert (np.diff(err.astype(np.float64), axis=1) >= 0).all(), "err non-decreasing along the beams"
    for b in range(B):
        assert len({tuple(p) for p in paths[b].tolist()}) == W, f"item {b}: duplicate paths"
    want = path_residual(x, cbs, paths)
    if residual is not None:
        np.testing.assert_allclose(residual.astype(np.float64), want, rtol=0, atol=1e-5)
    gap = np.abs(err.astype(np.float64) - (want * want).sum(-1))
    assert (gap <= 1e-5 * scale[:, None]).all(), gap.max()


# ---------------------------------------------------------------------------------------------- collisions
def resolve_ref(paths):
    """The resolution rule as a dict loop over plain Python tuples -> (ids (N, L), choice (N,))."""
    N, W, L = paths.shape
    rows = [[tuple(int(v) for v in paths[i, r]) for r in range(W)] for i in range(N)]
    owner, choice = {}, [None] * N
    for r in range(W):
        for i in range(N):            # ascending index: the lowest proposer of a free tuple takes it
            if choice[i] is None and rows[i][r] not in owner:
                owner[rows[i][r]] = i
                choice[i] = r
    choice = [0 if c is None else c for c in choice]
    ids = np.array([rows[i][choice[i]] for i in range(N)], np.int64).reshape(N, L)
    return ids, np.array(choice, np.int64)


def n_collided(ids):
    """#items whose dedup rank is > 0: items that share their tuple with a lower-index item."""
    seen, n = set(), 0
    for t in map(tuple, np.asarray(ids).tolist()):
        n += t in seen
        seen.add(t)
    return n


def duplicate_vectors(D, seed, n_vec=8, copies=8):
    """n_vec distinct rows, each `copies` times, copies interleaved (row i = vector i % n_vec)."""
    v = gi.residual_rows(n_vec, D, seed)
    return np.tile(v, (copies, 1))


def collision_fixtures():
    """name -> paths (N, W, L) int64 for collisions.resolve."""
    out = {}
    x = duplicate_vectors(16, 201)
    _, cbs = make_inputs(1, 16, 32, 3, "random", 202)
    out["duplicates"] = beam_ref(x, cbs, 8)["paths"]                     # 8 vectors x 8 copies, W = 8
    g = gi.rng(203)
    out["disjoint"] = np.stack([np.arange(160) // 100, (np.arange(160) // 10) % 10, np.arange(160) % 10], 1).reshape(40, 4, 3)
    # round-r proposals hit owned tuples: few distinct tuples, so later rounds mostly propose what is taken, some
    # items are never placed, and equal proposals meet within a round
    out["crowded"] = g.integers(0, 4, size=(30, 5, 2)).astype(np.int64)
    return out
