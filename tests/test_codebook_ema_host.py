"""EMA-maintained codebooks on the host: the plain-torch CPU path of modules.codebook_ema against the fp64 reference
(codebook_ema_support: the rule and its bounds), RqVae.use_ema_codebooks' refusals and state contract, the revival
tie-in, the declared C entry points and the plan, and the two-rank protocol over gloo."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch

import codebook_ema_support as S
from conftest import ROOT


def _t(a):
    return torch.from_numpy(np.array(a))


# ------------------------------------------------------------------------------- the torch restatement
@pytest.mark.parametrize("name", [c[0] for c in S.STATS_CASES])
def test_cpu_stats_match_reference(name):
    from modules.codebook_ema import ema_stats_
    c = S.stats_case(name)
    n, s = _t(c["n0"]), _t(c["s0"])
    ema_stats_(_t(c["res"]), _t(c["ids"]), n, s)
    S.check_stats(c, n.numpy(), s.numpy())


def test_cpu_stats_accumulate_two_batches():
    from modules.codebook_ema import ema_stats_
    a, b = S.stats_case("ml32m"), S.stats_case("second")
    n, s = _t(a["n0"]), _t(a["s0"])
    ema_stats_(_t(a["res"]), _t(a["ids"]), n, s)
    mid = s.numpy().copy()
    ema_stats_(_t(b["res"]), _t(b["ids"]), n, s)
    S.check_stats(b, n.numpy(), s.numpy(), n0=a["n0"] + a["n"], s0=mid)
    want = a["s0"].astype(np.float64) + a["s"] + b["s"]   # the fp64 sum of both batches
    bound = S.U * (a["n"][:, :, None] * a["a"] + b["n"][:, :, None] * b["a"] + np.abs(mid) + np.abs(want))
    assert (np.abs(s.numpy().astype(np.float64) - want) <= bound).all()


@pytest.mark.parametrize("name", [c[0] for c in S.APPLY_CASES])
def test_cpu_apply_matches_reference(name):
    from modules.codebook_ema import ema_apply_
    c = S.apply_case(name)
    w = [torch.zeros(c["K"], c["D"]) for _ in range(c["L"])]
    N, Sx, n, s = _t(c["N0"]), _t(c["S0"]), _t(c["n"]), _t(c["s"])
    ema_apply_(w, N, Sx, n, s, decay=c["decay"], eps=c["eps"])
    S.check_apply(c["N0"], c["S0"], c["n"], c["s"], c["decay"], c["eps"], N.numpy(), Sx.numpy(),
                  np.stack([x.numpy() for x in w]), n.numpy(), s.numpy())


def test_case_table_covers_the_edges():
    assert (S.stats_case("collapsed")["n"] > 0).sum(1).tolist() == [1, 1]
    assert (S.stats_case("sparse")["n"] == 0).sum() >= 2 * (256 - 40)
    sk = S.stats_case("skip")
    assert (sk["ids"] == -1).any() and (sk["ids"] >= sk["K"]).any() and sk["n"].sum() < sk["ids"].size
    assert S.stats_case("empty")["n"].sum() == 0


def test_argument_errors():
    from modules.codebook_ema import ema_apply_, ema_stats_

    def state(L, K, D):
        return ([torch.zeros(K, D) for _ in range(L)], torch.ones(L, K), torch.zeros(L, K, D),
                torch.zeros(L, K, dtype=torch.int64), torch.zeros(L, K, D))
    for kw, match in ((dict(decay=1.0), "decay"), (dict(decay=-0.1), "decay"), (dict(eps=0.0), "eps")):
        with pytest.raises(ValueError, match=match):
            ema_apply_(*state(1, 4, 8), **kw)
    with pytest.raises(ValueError, match="D % 4"):
        ema_apply_(*state(1, 4, 6))
    with pytest.raises(ValueError, match="K <= 4096"):
        ema_apply_(*state(1, 4097, 4))
    with pytest.raises(ValueError, match="L <= 16"):
        ema_stats_(torch.zeros(17, 2, 4), torch.zeros(2, 17, dtype=torch.int64), torch.zeros(17, 2, dtype=torch.int64),
                   torch.zeros(17, 2, 4))
    with pytest.raises(ValueError, match="res"):
        ema_stats_(torch.zeros(1, 2, 4), torch.zeros(3, 1, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int64),
                   torch.zeros(1, 2, 4))


def test_ops_refuse_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.codebook_ema_stats(torch.zeros(1, 2, 4), torch.zeros(2, 1, dtype=torch.int64),
                               torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, 4))
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.codebook_ema_apply([torch.zeros(2, 4)], torch.ones(1, 2), torch.zeros(1, 2, 4),
                               torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, 4), 0.99, 1e-5)


# ------------------------------------------------------------------------------------------- the model
def _model(**kw):
    from modules.quantize import QuantizeForwardMode
    from modules.rqvae import RqVae
    cfg = dict(input_dim=24, embed_dim=8, hidden_dims=[16], codebook_size=4, codebook_kmeans_init=False,
               codebook_mode=QuantizeForwardMode.ROTATION_TRICK, n_layers=2, n_cat_features=0)
    cfg.update(kw)
    return RqVae(**cfg)


def test_use_ema_codebooks_refusals():
    from modules.quantize import QuantizeDistance, QuantizeForwardMode
    for kw in (dict(codebook_sim_vq=True), dict(codebook_normalize=True)):
        with pytest.raises(ValueError, match="out_proj"):
            _model(**kw).use_ema_codebooks()
    with pytest.raises(ValueError, match="k-means"):
        _model(codebook_kmeans_init=True).use_ema_codebooks()
    with pytest.raises(ValueError, match="STE or ROTATION_TRICK"):
        _model(codebook_mode=QuantizeForwardMode.GUMBEL_SOFTMAX).use_ema_codebooks()
    m = _model()
    m.layers[1].distance_mode = QuantizeDistance.COSINE
    with pytest.raises(ValueError, match="L2"):
        m.use_ema_codebooks()
    for kw in (dict(decay=1.0), dict(decay=-1e-3), dict(eps=0.0)):
        with pytest.raises(ValueError):
            _model().use_ema_codebooks(**kw)
    m = _model()
    for what in (m.ema_update, m.ema_state_dict, m.ema_discard_stats):
        with pytest.raises(ValueError, match="use_ema_codebooks"):
            what()
    with pytest.raises(ValueError, match="use_ema_codebooks"):
        m.revive_dead_codes(torch.zeros(4, 24), seed=0, ema_min_count=0.5)
    assert m.ema is None and all(l.embedding.weight.requires_grad for l in m.layers)   # refusals change nothing
    _model(codebook_mode=QuantizeForwardMode.STE).use_ema_codebooks()


def test_state_contract_and_checkpoint_round_trip():
    m = _model()
    keys = list(m.state_dict().keys())
    m.use_ema_codebooks(decay=0.9, eps=1e-4)
    assert list(m.state_dict().keys()) == keys and not list(m.named_buffers())
    assert not any(l.embedding.weight.requires_grad for l in m.layers)
    assert all(p.requires_grad for p in list(m.encoder.parameters()) + list(m.decoder.parameters()))
    e = m.ema
    W = torch.stack([l.embedding.weight.detach() for l in m.layers])
    assert e["N"].shape == (2, 4) and e["N"].dtype == torch.float32 and bool((e["N"] == 1).all())   # N = 1, S = W
    assert torch.equal(e["S"], W) and e["S"].data_ptr() != m.layers[0].embedding.weight.data_ptr()
    assert e["n"].dtype == torch.int64 and not e["n"].any() and not e["s"].any()
    e["N"].mul_(3.0)
    e["S"].add_(1.0)
    sd = m.ema_state_dict()
    assert sorted(sd) == ["N", "S", "decay", "eps"] and sd["decay"] == 0.9 and sd["eps"] == 1e-4
    m2 = _model()
    m2.load_state_dict(m.state_dict())
    m2.use_ema_codebooks()
    m2.ema["n"] += 1
    m2.load_ema_state_dict(sd)
    assert m2.ema["decay"] == 0.9 and m2.ema["eps"] == 1e-4 and not m2.ema["n"].any()
    assert torch.equal(m2.ema["N"], e["N"]) and torch.equal(m2.ema["S"], e["S"])
    sd["N"].zero_()   # the state dict holds copies
    assert bool((e["N"] == 3).all())
    with pytest.raises(ValueError, match="N / S"):
        m2.load_ema_state_dict({"decay": 0.9, "eps": 1e-4, "N": torch.ones(2, 5), "S": sd["S"]})


def test_revival_tie_in_dead_set_and_reseated_state():
    """The dead set from ema_min_count and the re-seated rows' N, S (CPU model: torch paths of revival and quantize
    are not needed — revive_ is given the residuals through a stubbed quantize_levels)."""
    import codebook_support as R
    m = _model(codebook_size=4)
    m.use_ema_codebooks()
    g = torch.Generator().manual_seed(3)
    res = torch.randn(2, 6, 8, generator=g)
    m.encode = lambda x: x
    m.quantize_levels = lambda r0, t, with_norms=False: (None, res, None, None, None)
    m.ema["N"].copy_(torch.tensor([[0.2, 1.5, 0.49, 0.5], [2.0, 0.0, 3.0, 0.1]]))
    N0, S0 = m.ema["N"].clone(), m.ema["S"].clone()
    W0 = torch.stack([l.embedding.weight.detach().clone() for l in m.layers])
    n_rev = m.revive_dead_codes(torch.zeros(6, 24), seed=11, ema_min_count=0.5)   # no track_usage() needed
    dead = N0 < 0.5
    assert n_rev.tolist() == [2, 2] and dead.tolist() == [[True, False, True, False], [False, True, False, True]]
    W = torch.stack([l.embedding.weight.detach() for l in m.layers])
    ref = R.revive_ref(W0.numpy(), (~dead).numpy().astype(np.int64), res.numpy(), 1, 11)
    assert np.array_equal(R.bits(W.numpy()), R.bits(ref["weights"]))
    assert torch.equal(m.ema["N"], torch.where(dead, torch.ones_like(N0), N0))
    assert torch.equal(m.ema["S"], torch.where(dead[:, :, None], W, S0))
    # the window counters still work with EMA on, and re-seat N, S the same way
    m.track_usage()
    m.code_usage.copy_(torch.tensor([[1, 0, 2, 3], [1, 1, 1, 1]]))
    m.ema["N"].fill_(7.0)
    assert m.revive_dead_codes(torch.zeros(6, 24), seed=5).tolist() == [1, 0]
    assert m.ema["N"].tolist() == [[7.0, 1.0, 7.0, 7.0], [7.0] * 4] and not m.code_usage.any()
    assert torch.equal(m.ema["S"][0, 1], m.layers[0].embedding.weight.detach()[1])
    # without EMA and without the new argument nothing changed
    with pytest.raises(ValueError, match="track_usage"):
        _model().revive_dead_codes(torch.zeros(4, 24), seed=0)


# ----------------------------------------------------------------------------------- the C entry points
def test_entry_points_declared_and_typed():
    from rqvae_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rqvae_hip.h")).read(), flags=re.S)
    for name, nargs in (("rq_codebook_ema_stats_plan", 5), ("rq_codebook_ema_stats_workspace", 4),
                        ("rq_codebook_ema_stats", 11), ("rq_codebook_ema_apply", 11)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib._SIGS and name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGS[name][0]) == nargs
    import train_rqvae
    assert train_rqvae.CODEBOOK_EMA_DECAY == 0 and train_rqvae.CODEBOOK_EMA_EPS == 1e-5   # off by default
    assert train_rqvae.REVIVE_EMA_MIN_COUNT is None


def _lib_or_skip():
    from rqvae_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _lib, _lib.load()


def test_plan_forms_and_host_checks():
    _lib, lib = _lib_or_skip()
    assert lib.rq_abi_version() == 4
    f = _lib.EmaStatsForm()
    forms = {}
    for name, B, D, K, L, _ in S.STATS_CASES:
        assert lib.rq_codebook_ema_stats_plan(B, D, K, L, ctypes.byref(f)) == 0
        forms[name] = (f.form, f.chunks, f.tiles, f.codes_per_tile, f.rows_per_chunk)
        ws = lib.rq_codebook_ema_stats_workspace(B, D, K, L)
        if B:
            assert f.tiles * f.codes_per_tile >= K > (f.tiles - 1) * f.codes_per_tile
            assert f.chunks * f.rows_per_chunk >= B > (f.chunks - 1) * f.rows_per_chunk and f.rows_per_chunk % 1024 == 0
            assert f.codes_per_tile * D <= 16384 and f.lds_bytes <= 96 * 1024
            assert ws >= L * f.chunks * K * (D + 1) * 4
    NONE, LDS, TILED = 0, 1, 2
    assert {v[0] for v in forms.values()} == {NONE, LDS, TILED}   # the table reaches every form the library has
    assert forms["empty"][0] == NONE and forms["ml32m"][:3] == (LDS, 1, 1) and forms["collapsed"][:3] == (LDS, 5, 1)
    assert forms["wide"][0] == LDS and forms["k5"][0] == LDS and forms["chunks"][:2] == (LDS, 3)
    assert forms["tiled"][0] == TILED and forms["tiled"][2:4] == (16, 256)
    assert forms["subblocks"][0] == TILED and forms["subblocks"][4] == 2048
    # the LDS form covers K D <= 16,384 for every legal D >= 8, the ML-32M training shape included
    for D in range(8, 1025, 4):
        assert lib.rq_codebook_ema_stats_plan(65536, D, min(4096, 16384 // D), 3, ctypes.byref(f)) == 0 and f.form == LDS
    assert lib.rq_codebook_ema_stats_plan(65536, 32, 256, 3, ctypes.byref(f)) == 0 and (f.form, f.chunks) == (LDS, 64)
    for B, D, K, L in ((1, 6, 4, 1), (1, 1028, 4, 1), (1, 8, 4097, 1), (1, 8, 4, 17), (1 << 31, 8, 4, 1), (-1, 8, 4, 1)):
        assert lib.rq_codebook_ema_stats_plan(B, D, K, L, ctypes.byref(f)) == -22
        assert lib.rq_codebook_ema_stats_workspace(B, D, K, L) == 0
    # host-side refusals never touch the device
    assert lib.rq_codebook_ema_stats(None, None, 0, 8, 4, 1, None, None, None, 0, None) == 0   # B = 0: no-op
    assert lib.rq_codebook_ema_stats(None, None, 4, 8, 4, 1, None, None, None, 0, None) == -22
    assert b"null pointer" in lib.rq_last_error()
    for decay, eps in ((1.0, 1e-5), (-0.5, 1e-5), (0.99, 0.0), (float("nan"), 1e-5)):
        assert lib.rq_codebook_ema_apply(None, 1, 4, 8, None, None, None, None, decay, eps, None) == -22
        assert b"decay" in lib.rq_last_error()
    assert lib.rq_codebook_ema_apply(None, 1, 4, 8, None, None, None, None, 0.99, 1e-5, None) == -22
    assert b"null pointer" in lib.rq_last_error()


# ------------------------------------------------------------------------------------ two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_DP = dict(L=2, K=8, D=4, B=24, decay=0.9, eps=1e-5)


def _dp_inputs():
    g = np.random.Generator(np.random.PCG64(9))
    L, K, D, B = _DP["L"], _DP["K"], _DP["D"], _DP["B"]
    w = g.standard_normal((L, K, D), dtype=np.float32)
    res = g.standard_normal((L, B, D), dtype=np.float32)
    ids = g.integers(0, K, size=(B, L)).astype(np.int64)
    return w, res, ids


def _dp_run(w, res, ids, lo, hi):
    """-> (W, N, S, n, s after the update; the shard's own n, s before it)."""
    from modules.codebook_ema import ema_apply_, ema_stats_, initial_state
    tw = [torch.from_numpy(w[l].copy()) for l in range(_DP["L"])]
    N, Sx, n, s = initial_state(tw)
    ema_stats_(torch.from_numpy(res[:, lo:hi].copy()), torch.from_numpy(ids[lo:hi].copy()), n, s)
    own = (n.numpy().copy(), s.numpy().copy())
    ema_apply_(tw, N, Sx, n, s, decay=_DP["decay"], eps=_DP["eps"])   # sums n, s over the ranks first
    return (np.stack([t.numpy() for t in tw]), N.numpy().copy(), Sx.numpy().copy(), n.numpy().copy(),
            s.numpy().copy()) + own


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    from rqvae_hip import dp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    try:
        dp.init_from_env(backend="gloo")
        w, res, ids = _dp_inputs()
        lo, hi = dp.shard_range(_DP["B"], rank, world)
        q.put((rank,) + _dp_run(w, res, ids, lo, hi))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_agree_bitwise_and_with_single_process():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=180) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for a, b in zip(out[0][1:6], out[1][1:6]):   # W, N, S, n, s: the ranks agree bit for bit
        assert a.tobytes() == b.tobytes()
    w, res, ids = _dp_inputs()
    g, eps = _DP["decay"], _DP["eps"]
    N0, S0 = np.ones((_DP["L"], _DP["K"]), np.float32), w
    # each rank applied the sum of the shards' statistics (fp32 a + b is one rounding, the same on every rank)
    n_sum, s_sum = out[0][6] + out[1][6], out[0][7] + out[1][7]
    S.check_apply(N0, S0, n_sum, s_sum, g, eps, out[0][2], out[0][3], out[0][1], out[0][4], out[0][5])
    # a single process on the concatenated batch
    one = _dp_run(w, res, ids, 0, _DP["B"])
    n, s, a = S.stats_ref(res, ids, _DP["K"])
    assert np.array_equal(one[5], n) and np.array_equal(n_sum, n)
    sum_bound = n[:, :, None] * S.U * a + S.U * np.abs(s)   # a sum of n rows in any order (+ the shards' add)
    assert (np.abs(one[6] - s) <= sum_bound).all() and (np.abs(s_sum - s) <= sum_bound).all()
    S.check_apply(N0, S0, one[5], one[6], g, eps, one[1], one[2], one[0], one[3], one[4])
    # the two runs agree within the summation bound carried through the update
    upd = 4 * S.U * (np.abs(g * S0) + np.abs((1 - g) * s))
    assert (np.abs(out[0][3].astype(np.float64) - one[2]) <= (1 - g) * 2 * sum_bound + 2 * upd).all()
    assert np.array_equal(out[0][2], one[1])   # N' comes from exact counts
