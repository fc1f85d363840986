"""The dropout mask generator, stated once on the host (oracle/dropout.py), and the key schedule of
ops.next_seed — CPU only.

* the restatement is SplitMix64 (published sequence) and its flat (keep1) and float4 (keep4) forms agree;
* rq_dropout_params (the library's threshold / scale) equals the restatement's rules, edges included;
* the masks behave like independent fair draws where the model needs them to: per float4 position, along a
  stream at the lags of float4 neighbours and of column neighbours at the model's row widths, and between
  the keys the model really draws (consecutive keys, data-parallel ranks, graph epochs, adjacent base seeds);
* no two keys the model can draw are within 2^32 counters of each other. The streams of keys a and b are
  shifted copies of one sequence, key_distance(a, b) counters apart; 2^32 counters are 2^33 elements (32 GiB
  of fp32), above anything the model allocates (its largest dropout tensor is 11,600 x 1,024).

Every statistical bound is 6 sigma of the binomial (test_fused_decoder_gpu._check_rate's convention). Inputs
are fixed, so these are deterministic comparisons. A stream's agreement with itself at lag L has overlapping
pairs (element i + L sits in two of them), which at p = 0.1 makes its true sigma 1.33x the binomial's; the
binomial bound is kept, and is then the tighter one.

tests/test_dropout_mask_gpu.py pins every kernel that draws a mask to this restatement, bit for bit.
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from oracle import dropout as D

N = 1 << 20
PS = (0.1, 0.5)
LAGS_SELF = (1, 2, 3, 4, 64, 256, 512, 1024)
LAGS_PAIR = range(-8, 9)
BOUND = 1 << 32   # counters


def _ops():
    from rqvae_hip import ops
    return ops


@pytest.fixture
def seeded():
    """Tests below call torch.manual_seed: put torch's CPU generator and the key counter back afterwards."""
    ops = _ops()
    s0, state, saved = torch.initial_seed(), torch.get_rng_state(), dict(ops._SEED)
    yield ops
    torch.manual_seed(s0)
    torch.set_rng_state(state)
    ops._SEED.update(saved)


def _keys(ops, base, n):
    """The first n keys under torch.manual_seed(base). The key counter restarts when torch.initial_seed()
    changes, so another seed is bound first."""
    torch.manual_seed(base ^ 1)
    ops.next_seed()
    torch.manual_seed(base)
    return [ops.next_seed() for _ in range(n)]


def _with_rank(monkeypatch, ops, rank):
    monkeypatch.setattr(ops, "_dist", types.SimpleNamespace(is_available=lambda: True, is_initialized=lambda: True,
                                                            get_rank=lambda: rank))


def _sigma6(q, n):
    return 6 * np.sqrt(q * (1 - q) / n)


def _agreement(a, b, lag):
    """Fraction of i with a[i] == b[i + lag] over the overlap, and the overlap's length."""
    if lag < 0:
        return _agreement(b, a, -lag)
    n = len(a) - lag
    return float(np.mean(a[:n] == b[lag:])), n


def _check_pair_independent(ka, kb, what, epochs=(0, 0)):
    for p in PS:
        a, b = D.keep_mask(ka, N, p, epochs[0]), D.keep_mask(kb, N, p, epochs[1])
        q = (1 - p) ** 2 + p ** 2
        for lag in LAGS_PAIR:
            agree, n = _agreement(a, b, lag)
            assert abs(agree - q) < _sigma6(q, n), (what, p, lag, agree, q)


# ------------------------------------------------------------------------------- the restatement
def test_splitmix64_published_sequence():
    ref = [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]
    assert D.splitmix64(1234567, np.arange(5)).tolist() == ref
    assert int(D.splitmix64(1234567, 3)[0]) == ref[3]
    assert (D.G * D.G_INV) % (1 << 64) == 1


def test_flat_and_float4_forms_agree():
    for seed, epoch in ((0, 0), (1234567, 0), ((1 << 64) - 1, 0), (42, 3), (42, (1 << 33) + 5)):
        flat = D.mask_words(seed, 0, 4 * 1000, epoch)
        assert np.array_equal(flat.reshape(-1, 4), D.mask_words4(seed, 0, 1000, epoch))
        # an unaligned window of the same stream
        assert np.array_equal(D.mask_words(seed, 4 * 250 + 3, 777, epoch), flat[1003:1780])
    # word 0 is the LOW half of the 64-bit draw, element index row-major
    m = D.splitmix64(7, np.arange(2))
    assert D.mask_words(7, 0, 4).tolist() == [int(m[0]) & 0xFFFFFFFF, int(m[0]) >> 32, int(m[1]) & 0xFFFFFFFF, int(m[1]) >> 32]
    assert np.array_equal(D.keep_mask(7, (3, 8), 0.3).reshape(-1), D.mask_words(7, 0, 24) >= D.threshold(0.3))
    assert int(D.epoch_key((1 << 64) - 1, 2)) == ((1 << 64) - 1 + 2 * D.E) % (1 << 64)


def test_key_distance_is_a_stream_shift():
    """Keys k and k + d G draw the same sequence, d counters apart."""
    k = 0x0123456789ABCDEF
    for d in (1, -1, 5, -(1 << 40)):
        k2 = (k + d * D.G) % (1 << 64)
        assert D.key_distance(k2, k) == d and D.key_distance(k, k2) == -d
        assert D.key_distance(np.array([k2], dtype=np.uint64), np.array([k], dtype=np.uint64)).tolist() == [d]
    assert np.array_equal(D.splitmix64((k + 5 * D.G) % (1 << 64), np.arange(100)), D.splitmix64(k, np.arange(5, 105)))


# ------------------------------------------------------------------------ the library's parameters
def _lib():
    from rqvae_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _lib.load()


@pytest.mark.parametrize("p", [0.0, -1.0, float("nan"), 1e-10, 0.1, 0.3, 0.5, 1 - 2.0 ** -24, 1.0, 2.0])
def test_dropout_params_match_restatement(p):
    lib = _lib()
    thr, scale = ctypes.c_uint32(), ctypes.c_float()
    assert lib.rq_dropout_params(ctypes.c_float(p), ctypes.byref(thr), ctypes.byref(scale)) == 0
    assert thr.value == D.threshold(p), (p, thr.value, D.threshold(p))
    assert np.float32(scale.value).tobytes() == D.scale(p).tobytes(), (p, scale.value, D.scale(p))
    if p == 0.5:
        assert thr.value == 1 << 31
    if p == 1 - 2.0 ** -24:   # the largest fp32 below 1: thr = 2^32 - 256, not wrapped to a small value
        assert thr.value == (1 << 32) - 256 and scale.value == 2.0 ** 24
    if not p > 0:
        assert (thr.value, scale.value) == (0, 1.0)
    if p >= 1:
        assert (thr.value, scale.value) == (0xFFFFFFFF, 0.0)


# --------------------------------------------------------------------- statistics of the restatement
@pytest.mark.parametrize("p", PS)
def test_stream_rate_and_self_agreement(seeded, p):
    ops = seeded
    for key in _keys(ops, 1234, 3):
        m = D.keep_mask(key, N, p)
        for j in range(4):   # each float4 position on its own
            keep = float(np.mean(m[j::4]))
            assert abs(keep - (1 - p)) < _sigma6(p, N // 4), (key, p, j, keep)
        q = (1 - p) ** 2 + p ** 2
        for lag in LAGS_SELF:
            agree, n = _agreement(m, m, lag)
            assert abs(agree - q) < _sigma6(q, n), (key, p, lag, agree, q)


def test_consecutive_keys_are_independent(seeded):
    ops = seeded
    ks = _keys(ops, 1234, 5)
    for a, b in zip(ks, ks[1:]):
        _check_pair_independent(a, b, ("consecutive", a, b))


def test_rank_keys_are_independent(seeded, monkeypatch):
    ops = seeded
    per_rank = []
    for r in range(4):
        _with_rank(monkeypatch, ops, r)
        per_rank.append(_keys(ops, 1234, 2))
    for r in range(3):
        for n in range(2):
            _check_pair_independent(per_rank[r][n], per_rank[r + 1][n], ("rank", r, n))


def test_epoch_keys_are_independent(seeded):
    ops = seeded
    key = _keys(ops, 1234, 1)[0]
    for e in (0, 1, 1000, (1 << 33) + 5):
        _check_pair_independent(key, key, ("epoch", e), epochs=(e, e + 1))


@pytest.mark.parametrize("s", [0, 100, (1 << 31) - 1])
def test_adjacent_base_seeds_are_independent(seeded, s):
    """The n-th mask under torch.manual_seed(s) against the n-th under manual_seed(s + 1): a seed sweep over
    adjacent seeds must see independent dropout noise. (With keys linear in the base seed, base + 1 moved the
    stream by exactly one counter: agreement 1.0 at lag 2 for about half of the keys.)"""
    ops = seeded
    ka, kb = _keys(ops, s, 8), _keys(ops, s + 1, 8)
    for n, (a, b) in enumerate(zip(ka, kb), 1):
        _check_pair_independent(a, b, ("base", s, n))


# ------------------------------------------------------------------------------- the key schedule
BASES = (0, 1, 2, 100, 101, (1 << 31) - 1, 1 << 31, (1 << 63) - 1)


def _schedule(ops, monkeypatch):
    """{(base, rank, n): key} for the bases above, ranks 0..3, n = 1..64."""
    keys = {}
    for base in BASES:
        for r in range(4):
            _with_rank(monkeypatch, ops, r)
            for n, k in enumerate(_keys(ops, base, 64), 1):
                keys[(base, r, n)] = k
    return keys


def _abs_distance(d):
    """|d| of wrapped uint64 differences, as uint64 (2^63 maps to itself)."""
    with np.errstate(over="ignore"):
        return np.minimum(d, ~d + np.uint64(1))


def test_no_two_keys_within_2_32_counters(seeded, monkeypatch):
    ops = seeded
    keys = _schedule(ops, monkeypatch)
    ids = list(keys)
    k = np.array([keys[i] for i in ids], dtype=np.uint64)
    assert len(k) == len(BASES) * 4 * 64
    with np.errstate(over="ignore"):
        c = k * np.uint64(D.G_INV)                       # counter coordinate: distance(a, b) = c_a - c_b
        d = _abs_distance(c[:, None] - c[None, :])
    d[np.arange(len(k)), np.arange(len(k))] = np.uint64(1 << 63)   # a key against itself
    i, j = np.unravel_index(np.argmin(d), d.shape)
    assert int(d[i, j]) >= BOUND, (ids[i], ids[j], D.key_distance(int(k[i]), int(k[j])))
    assert len(set(k.tolist())) == len(k)


def test_no_two_epoch_keys_within_2_32_counters(seeded, monkeypatch):
    """epoch_key(k_i, e) against epoch_key(k_j, e') for e - e' = +-1..1024, i = j included (one layer's masks
    at different replays of a captured step)."""
    ops = seeded
    keys = _schedule(ops, monkeypatch)
    ids = [i for i in keys if i[2] <= 2][:64]   # 8 bases x 4 ranks x the first two keys
    k = np.array([keys[i] for i in ids], dtype=np.uint64)
    assert len(k) == 64
    delta = np.concatenate([np.arange(-1024, 0), np.arange(1, 1025)])
    with np.errstate(over="ignore"):
        c = k * np.uint64(D.G_INV)
        step = D._u64(delta) * np.uint64((D.E * D.G_INV) % (1 << 64))    # counters per epoch delta
        for i in range(len(k)):
            d = _abs_distance((c[i] - c)[:, None] + step[None, :])       # (j, delta)
            assert int(d.min()) >= BOUND, (ids[i], [(ids[j], int(delta[t])) for j, t in zip(*np.where(d < BOUND))][:4])
    # the vectorised coordinate is key_distance: one spot check through the public function
    want = (int(c[3]) - int(c[5]) + int(step[1024 + 4])) % (1 << 64)     # delta[1024 + 4] == 5
    assert D.key_distance(int(D.epoch_key(int(k[3]), 7)), int(D.epoch_key(int(k[5]), 2))) % (1 << 64) == want


def test_next_seed_contract(seeded, monkeypatch):
    ops = seeded
    a = _keys(ops, 77, 16)
    assert all(isinstance(k, int) and 0 <= k < (1 << 63) for k in a)           # fits int64
    assert len(set(a)) == 16
    torch.manual_seed(78)                                                       # the counter restarts with the base
    b = [ops.next_seed() for _ in range(4)]
    assert not set(a) & set(b)
    torch.manual_seed(77)                                                       # manual_seed replays the sequence
    assert [ops.next_seed() for _ in range(16)] == a
    assert ops.next_seed() not in a                                             # and goes on from there
    _with_rank(monkeypatch, ops, 1)
    assert not set(_keys(ops, 77, 16)) & set(a)                                 # ranks sharing a seed: other keys
    for base in ((1 << 63) - 1, 1 << 63, (1 << 64) - 1):
        assert all(0 <= k < (1 << 63) for k in _keys(ops, base, 4))
