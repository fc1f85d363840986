"""Dead-code revival on the host: the plain-torch CPU path of modules.codebook_revival.revive_ against the numpy
restatement (bitwise), the argument errors, the state-dict contract of RqVae.track_usage, the declared C entry
points, and the two-rank protocol over gloo (summed counts, rank 0's donors, identical parameters)."""
import os
import re
import socket

import numpy as np
import pytest
import torch

import codebook_support as S
from conftest import ROOT


def _torch_inputs(case):
    w = [torch.from_numpy(case["weights"][l].copy()) for l in range(case["L"])]
    m = v = None
    if case["exp_avg"] is not None:
        m = [torch.from_numpy(case["exp_avg"][l].copy()) for l in range(case["L"])]
        v = [torch.from_numpy(case["exp_avg_sq"][l].copy()) for l in range(case["L"])]
    return w, torch.from_numpy(case["counts"].copy()), torch.from_numpy(case["res"].copy()), m, v


def _stack(ts):
    return None if ts is None else np.stack([t.detach().numpy() for t in ts])


@pytest.mark.parametrize("name", [c[0] for c in S.REVIVE_CASES])
def test_cpu_path_matches_restatement(name):
    from modules.codebook_revival import revive_
    case = S.revive_case(name)
    w, counts, res, m, v = _torch_inputs(case)
    n = revive_(w, counts, res, min_count=case["min_count"], seed=case["seed"], exp_avg=m, exp_avg_sq=v)
    assert n.dtype == torch.int64
    S.check_revived(case, _stack(w), _stack(m), _stack(v), None, n.numpy())
    assert not counts.any()   # the next usage window starts at zero


def test_restatement_cases_cover_the_edges():
    wrap = S.revive_case("wrap")["ref"]
    assert wrap["n_revived"][0] == 32 and wrap["n_revived"][1] == 0 and 0 < wrap["n_revived"][2] < 32
    rows = S.donor_rows(S.revive_case("wrap")["seed"], 0, 32, 32)
    assert sorted(rows.tolist()) == list(range(32))   # n_dead = K = B: every row used once
    chunk = S.revive_case("chunk")["ref"]["revived"]
    assert chunk[:, 255].all() and chunk[:, 256].all() and not chunk[:, 254].any() and not chunk[:, 258].any()
    min3 = S.revive_case("min3")
    assert min3["ref"]["n_revived"][2] == (min3["counts"][2] < 3).sum() > (min3["counts"][2] < 1).sum()
    assert S.revive_case("min3")["ref"]["n_revived"][1] == 0


def test_min_count_zero_revives_nothing():
    from modules.codebook_revival import revive_
    case = S.revive_case("wrap")
    w, counts, res, m, v = _torch_inputs(case)
    n = revive_(w, counts, res, min_count=0, seed=1, exp_avg=m, exp_avg_sq=v)
    assert n.tolist() == [0, 0, 0]
    assert np.array_equal(S.bits(_stack(w)), S.bits(case["weights"]))
    assert np.array_equal(S.bits(_stack(m)), S.bits(case["exp_avg"]))


def test_revive_argument_errors():
    from modules.codebook_revival import revive_

    def args(L, K, D, B):
        return ([torch.zeros(K, D) for _ in range(L)], torch.zeros(L, K, dtype=torch.int64), torch.zeros(L, B, D))
    with pytest.raises(ValueError, match="B=4 < K=8"):
        revive_(*args(1, 8, 4, 4), seed=0)
    with pytest.raises(ValueError, match="L <= 16"):
        revive_(*args(17, 2, 4, 2), seed=0)
    with pytest.raises(ValueError, match="D % 4"):
        revive_(*args(1, 2, 6, 2), seed=0)
    with pytest.raises(ValueError, match="min_count"):
        revive_(*args(1, 2, 4, 2), seed=0, min_count=-1)
    with pytest.raises(ValueError, match="go together"):
        revive_(*args(1, 2, 4, 2), seed=0, exp_avg=[torch.zeros(2, 4)])


def test_ops_refuse_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.code_usage(torch.zeros(4, 2, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int64))
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.codebook_revive([torch.zeros(2, 4)], torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, 4), 1, 0)


def _model(**kw):
    from modules.quantize import QuantizeForwardMode
    from modules.rqvae import RqVae
    cfg = dict(input_dim=24, embed_dim=8, hidden_dims=[16], codebook_size=4, codebook_kmeans_init=False,
               codebook_mode=QuantizeForwardMode.ROTATION_TRICK, n_layers=2, n_cat_features=0)
    cfg.update(kw)
    return RqVae(**cfg)


def test_revive_dead_codes_refuses_unsupported_models():
    from modules.quantize import QuantizeDistance
    x = torch.zeros(4, 24)
    with pytest.raises(ValueError, match="track_usage"):
        _model().revive_dead_codes(x, seed=0)
    for kw in (dict(codebook_sim_vq=True), dict(codebook_normalize=True)):
        m = _model(**kw)
        m.track_usage()
        with pytest.raises(ValueError, match="out_proj"):
            m.revive_dead_codes(x, seed=0)
    m = _model(codebook_kmeans_init=True)
    m.track_usage()
    with pytest.raises(ValueError, match="k-means"):
        m.revive_dead_codes(x, seed=0)
    m = _model()
    m.track_usage()
    m.layers[1].distance_mode = QuantizeDistance.COSINE
    with pytest.raises(ValueError, match="L2"):
        m.revive_dead_codes(x, seed=0)
    m = _model()
    m.track_usage()
    with pytest.raises(ValueError, match="at least K = 4 rows"):
        m.revive_dead_codes(x[:3], seed=0)
    assert m.training   # the checks come before the mode switch


def test_track_usage_keeps_state_dict_keys():
    m = _model()
    keys = list(m.state_dict().keys())
    m.track_usage()
    assert m.code_usage.shape == (2, 4) and m.code_usage.dtype == torch.int64 and not m.code_usage.any()
    assert list(m.state_dict().keys()) == keys and not any("code_usage" in k for k in keys)
    assert "code_usage" not in dict(m.named_buffers())
    m.code_usage[0, 1], m.code_usage[0, 2] = 3, 3
    used, ppl = m.usage_stats()
    assert used == [0.5, 0.0] and ppl[0] == pytest.approx(2.0) and ppl[1] == 0.0
    m.track_usage(False)
    assert m.code_usage is None and list(m.state_dict().keys()) == keys


def test_entry_points_declared_and_typed():
    from rqvae_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rqvae_hip.h")).read(), flags=re.S)
    for name, nargs in (("rq_code_usage", 6), ("rq_codebook_revive_workspace", 2), ("rq_codebook_revive", 16)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib._SIGS and name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGS[name][0]) == nargs
    import train_rqvae
    assert train_rqvae.REVIVE_EVERY == 0 and train_rqvae.REVIVE_MIN_COUNT == 1   # off by default


# ------------------------------------------------------------------------------------ two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_DP = dict(L=2, K=8, D=4, B=9, seed=12345)


def _dp_inputs(rank):
    """Same weights and moments on every rank (the data-parallel invariant); counts and res per rank. The counts
    are chosen so that neither rank's own dead set is the summed one."""
    g = np.random.Generator(np.random.PCG64(5))
    L, K, D, B = _DP["L"], _DP["K"], _DP["D"], _DP["B"]
    w, m, v = (g.standard_normal((L, K, D), dtype=np.float32) for _ in range(3))
    counts = np.zeros((2, L, K), np.int64)
    counts[0, :, [0, 2, 4]] = 1
    counts[1, :, [1, 2, 5]] = 2
    res = g.standard_normal((2, L, B, D), dtype=np.float32)
    return w, m, v, counts[rank], res[rank], counts.sum(0), res[0]


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    from modules.codebook_revival import revive_
    from rqvae_hip import dp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    try:
        dp.init_from_env(backend="gloo")
        w, m, v, counts, res, _, _ = _dp_inputs(rank)
        tw, tm, tv = ([torch.from_numpy(a[l].copy()) for l in range(_DP["L"])] for a in (w, m, v))
        tc = torch.from_numpy(counts.copy())
        n = revive_(tw, tc, torch.from_numpy(res.copy()), seed=_DP["seed"], exp_avg=tm, exp_avg_sq=tv)
        q.put((rank, _stack(tw), _stack(tm), _stack(tv), n.numpy().copy(), tc.numpy().copy()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_agree_with_single_process():
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
    w, m, v, _, _, total, res0 = _dp_inputs(0)
    ref = S.revive_ref(w, total, res0, 1, _DP["seed"], m, v)
    assert 0 < ref["n_revived"][0] < _DP["K"] - 3   # the summed dead set is smaller than either rank's own
    for _, gw, gm, gv, n, counts in out:
        assert np.array_equal(S.bits(gw), S.bits(ref["weights"]))
        assert np.array_equal(S.bits(gm), S.bits(ref["exp_avg"]))
        assert np.array_equal(S.bits(gv), S.bits(ref["exp_avg_sq"]))
        assert np.array_equal(n, ref["n_revived"]) and not counts.any()
