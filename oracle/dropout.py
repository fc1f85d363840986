"""Counter-based dropout mask — exact integer restatement on the host. Test infrastructure only.

Restates rq-vae-recommender_amd/csrc/common.h (splitmix64, epoch_seed, keep4 / keep1) and
csrc/dropout.hip (dropout_params), the one generator behind every dropout of the decoder path
(dropout.hip, rowwise.hip, the GEMM epilogues of linear.hip). Not a restatement of the reference: the
reference draws its masks from torch's generator and stores them; the kernels here regenerate the mask in
the backward from (seed, epoch, element index):

  counter c under key k:   z = k + (c + 1) G;  z = (z ^ z >> 30) M1;  z = (z ^ z >> 27) M2;  z ^ z >> 31
  key of (seed, epoch):    seed + epoch E                       (all arithmetic mod 2^64)
  element e of a tensor:   32-bit word (e & 1) of counter (e >> 1) — low word first — row-major e
  kept iff word >= thr,    thr = round(p 2^32) (saturated), kept values scaled by fp32 1 / (1 - p)

uint64 numpy throughout; no import of the product package.
"""
import numpy as np

G = 0x9E3779B97F4A7C15      # SplitMix64's increment (the golden-ratio constant): one counter step
M1 = 0xBF58476D1CE4E5B9     # the finaliser's multipliers
M2 = 0x94D049BB133111EB
E = 0xD6E8FEB86659FD93      # key step of one dropout epoch (common.h epoch_seed)
G_INV = pow(G, -1, 1 << 64)
_MASK64 = (1 << 64) - 1


def _u64(v):
    """A python int (any sign / size) or integer array as uint64, mod 2^64."""
    if isinstance(v, (int, np.integer)):
        return np.uint64(int(v) & _MASK64)
    a = np.asarray(v)
    return a if a.dtype == np.uint64 else a.astype(np.int64).view(np.uint64)   # signed values wrap


def splitmix64(seed, c):
    """SplitMix64 output of counter(s) c under key seed (common.h splitmix64); uint64, the shape of c."""
    c = np.atleast_1d(_u64(c))
    with np.errstate(over="ignore"):
        z = _u64(seed) + (c + np.uint64(1)) * np.uint64(G)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
        return z ^ (z >> np.uint64(31))


def epoch_key(seed, epoch):
    """Key the kernels draw from at a dropout epoch: seed + epoch E mod 2^64 (common.h epoch_seed). seed and
    epoch may be python ints or broadcastable integer arrays; returns uint64 (a numpy scalar for two ints)."""
    with np.errstate(over="ignore"):
        return _u64(seed) + _u64(epoch) * np.uint64(E)


def threshold(p) -> int:
    """thr of dropout_params (dropout.hip) for the fp32 probability p: 0 = no dropout."""
    p = np.float32(p)
    if not p > 0:
        return 0
    if p >= 1:
        return 0xFFFFFFFF
    t = float(p) * 4294967296.0          # exact: an fp32 times 2^32 in double
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t + 0.5)


def scale(p) -> np.float32:
    """Multiplier of the kept values, fp32 1 / (1 - p) (dropout_params)."""
    p = np.float32(p)
    if not p > 0:
        return np.float32(1.0)
    if p >= 1:
        return np.float32(0.0)
    return np.float32(1.0) / (np.float32(1.0) - p)


def mask_words(seed, start: int, n: int, epoch=0):
    """The 32-bit words of elements start .. start + n - 1 (uint32): element e takes word e & 1 (0 = the
    low half) of counter e >> 1 (common.h keep1)."""
    e = np.arange(int(start), int(start) + int(n), dtype=np.uint64)
    m = splitmix64(epoch_key(seed, epoch), e >> np.uint64(1))
    return (m >> (np.uint64(32) * (e & np.uint64(1)))).astype(np.uint32)


def mask_words4(seed, q0: int, nq: int, epoch=0):
    """The same words in the kernels' float4 form (common.h keep4): (nq, 4) uint32, quad q = q0 + i holds
    (lo, hi) of counter 2q, then (lo, hi) of counter 2q + 1."""
    q = np.arange(int(q0), int(q0) + int(nq), dtype=np.uint64)
    k = epoch_key(seed, epoch)
    a, b = splitmix64(k, np.uint64(2) * q), splitmix64(k, np.uint64(2) * q + np.uint64(1))
    lo32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    return np.stack([a & lo32, a >> s32, b & lo32, b >> s32], axis=1).astype(np.uint32)


def keep_mask(seed, shape, p, epoch=0):
    """bool mask of a tensor of `shape` under Dropout(p): True = kept; row-major element index."""
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    n = int(np.prod(shape, dtype=np.int64))
    thr = threshold(p)
    if thr == 0:
        return np.ones(shape, dtype=bool)
    return (mask_words(seed, 0, n, epoch) >= np.uint32(thr)).reshape(shape)


def key_distance(a, b):
    """(a - b) G^-1 mod 2^64 as a signed integer: how many counters apart the streams of keys a and b are
    (stream a at counter c equals stream b at counter c + distance). int for two ints, else an int64 array."""
    if isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer)):
        d = ((int(a) - int(b)) * G_INV) & _MASK64
        return d - (1 << 64) if d >> 63 else d
    with np.errstate(over="ignore"):
        return ((_u64(a) - _u64(b)) * np.uint64(G_INV)).view(np.int64)
